"""Who crosses a line on a tile mesh (cs_mesh_gate_crossings; NativeTileMesh.gate_crossings / count_gate_crossings): every
tile runs all gates against the agents it owns, its walk clipped to its owned cells; the counts add and the rows are
merged by (gate, id); the mesh gives the single engine's answer byte for byte, which is also the restatement's
(tests/gates_reference.py).  The cuts are even (2 x 2) and uneven: the crowd's own, at creation or after a re-cut.  No
halo exchange is made for it: the next steps of the mesh are those of a mesh that never asked."""
import numpy as np
import pytest

import odd_grids as og
from rmf_crowdsim_amd import LocationHash2D, NoLocalPlan, Simulation, StubHighLevelPlan, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from gates_reference import SIZE_MAX, agree, call, crossings, gates_array, last_error
from select_reference import selection
from test_gpu_gate_crossings import crowd_gates

pytestmark = pytest.mark.gpu
INF = float("inf")


def cut_gates(sc, rects, rec, t1=3.0):
    """the gates of the single-engine tests and gates along and astride every cut of `rects`: on the cut itself in both
    senses, half a cell to either side of it, across it at the twelve agents nearest to it, and a diagonal over the
    crossing of the cuts"""
    gates = [crowd_gates(rec, sc.grid, each=30, t1=t1)]
    ox, oy = sc.grid["offset"]
    cell = sc.cell
    rows, cols = og.cuts_of(rects)
    y_lo, y_hi, x_lo, x_hi = oy, oy + sc.cols * cell, ox, ox + sc.rows * cell
    seg = []
    for r in rows:
        x = ox + r * cell
        seg += [(x, y_lo, x, y_hi), (x, y_hi, x, y_lo), (x - 0.5 * cell, y_lo, x - 0.5 * cell, y_hi),
                (x + 0.5 * cell, y_hi, x + 0.5 * cell, y_lo)]
    for c in cols:
        y = oy + c * cell
        seg += [(x_lo, y, x_hi, y), (x_hi, y, x_lo, y), (x_lo, y - 0.5 * cell, x_hi, y - 0.5 * cell),
                (x_hi, y + 0.5 * cell, x_lo, y + 0.5 * cell)]
    for r in rows:
        for c in cols or [sc.cols // 2]:
            x, y = ox + r * cell, oy + c * cell
            seg += [(x - 9.0, y - 7.0, x + 8.0, y + 9.5), (x + 6.0, y - 6.0, x - 6.0, y + 6.0)]
    row, col = sc.cells_of(rec)
    for r in rows:  # across the cut beside the twelve agents nearest to it
        for a in rec[np.argsort(np.abs(row - r), kind="stable")[:12]]:
            seg.append((ox + r * cell - 3.1, float(a["y"]) + 0.4, ox + r * cell + 3.3, float(a["y"]) + 0.6))
    for c in cols:
        for a in rec[np.argsort(np.abs(col - c), kind="stable")[:12]]:
            seg.append((float(a["x"]) + 0.4, oy + c * cell - 3.1, float(a["x"]) + 0.6, oy + c * cell + 3.3))
    gates.append(gates_array(seg, 0.0, t1))
    return np.concatenate(gates)


def both_sides(sc, rects, rec, rows):
    """how many gates have rows of agents of more than one tile"""
    owner = dict(zip(rec["id"].tolist(), og.owners(rects, sc, rec).tolist()))
    tiles = {}
    for g, i in zip(rows["gate"].tolist(), rows["id"].tolist()):
        tiles.setdefault(g, set()).add(owner[i])
    return sum(1 for t in tiles.values() if len(t) > 1)


def _walkers_on(make, grid, n=2000, seed=3):
    """n standing agents, some exactly on the tile borders of a 2 x 2 cut, written random velocities by id"""
    rng = np.random.default_rng(seed)
    pts = np.column_stack([rng.uniform(0.5, grid["width"] - 0.5, n), rng.uniform(0.5, grid["height"] - 0.5, n)])
    half_x, half_y = 0.5 * grid["width"], 0.5 * grid["height"]
    pts[:40, 0] = np.tile([half_x, np.nextafter(half_x, -INF), np.nextafter(half_x, INF), half_x - 0.5], 10)
    pts[40:80, 1] = np.tile([half_y, np.nextafter(half_y, -INF), np.nextafter(half_y, INF), half_y + 0.5], 10)
    pts[80] = (half_x, half_y)
    sim = make(grid)
    sim.add_agents(pts, StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 2.0)
    sim.step(0.05)
    w = sim.read_agents()
    phi, speed = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(0.0, 2.5, n)
    w = w[np.argsort(w["id"])]
    w["vx"], w["vy"] = (speed * np.cos(phi)).astype(np.float32), (speed * np.sin(phi)).astype(np.float32)
    sim.write_agents(w, fields=("velocity",))
    return sim


def test_a_2_by_2_mesh_with_agents_on_the_tile_borders():
    """16 x 16 cells cut evenly into 2 x 2 tiles, walkers everywhere and exactly on both cuts, gates across and along the
    cuts: the mesh's rows and counts are the single engine's."""
    grid = dict(width=32.0, height=32.0, cell_size=2.0, offset=(0.0, 0.0))
    mesh = _walkers_on(lambda g: NativeTileMesh(LocationHash2D(**g), (2, 2), 1), grid)
    single = _walkers_on(lambda g: Simulation(LocationHash2D(**g)), grid)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes() and (mesh.tile_counts() > 300).all()
    on_cut = int(((rec["x"] == 16.0) | (rec["y"] == 16.0)).sum())
    assert on_cut >= 20
    seg = [(16.0, -5.0, 16.0, 40.0), (40.0, 16.0, -5.0, 16.0), (-3.0, -2.0, 35.0, 33.0), (10.0, 22.0, 22.0, 10.0),
           (15.0, 15.0, 17.0, 17.5), (16.0, 16.0, 16.0, 16.0)]
    rng = np.random.default_rng(8)
    c = np.column_stack([rng.uniform(0.0, 32.0, 300), rng.uniform(0.0, 32.0, 300)])
    d = rng.uniform(-4.0, 4.0, (300, 2))
    gates = np.concatenate([gates_array(seg, 0.0, 2.0), gates_array(np.column_stack([c - d, c + d]), rng.choice([0.0, 0.5], 300), 2.5),
                            crowd_gates(rec, grid)])
    for speed_max in (INF, 1.5):
        stats = {}
        want = agree(single, rec, grid, gates, speed_max, name=f"the engine, speed_max {speed_max}", stats=stats)
        print(f"    {stats}")
        assert min(stats.values()) > 0
        rows, counts = agree(mesh, rec, grid, gates, speed_max, name=f"2 x 2 tiles, speed_max {speed_max}", want=want)
    assert counts[:4].sum(axis=1).min() > 0 and not counts[5].any()  # (the cuts and the diagonals are crossed, A == B is not)
    for cap in (1, len(rows) // 2):
        got, per, out = call(mesh, gates, 1.5, cap=cap)
        assert got == len(rows) and per.tobytes() == counts.tobytes()
        assert out[:cap].tobytes() == rows[:cap].tobytes() and (out[cap:].view(np.uint8) == 0xAB).all()
    assert mesh.read_agents().tobytes() == rec.tobytes()


def test_a_mesh_on_uneven_cuts_and_after_a_recut_lists_the_crossings_of_one_engine():
    sc = og.scene("lopsided")
    weights = np.concatenate([p for p, _ in sc.parts])
    make = lambda grid: NativeTileMesh(LocationHash2D(**grid), (2, 2), 1, weights=weights)
    mesh, twin = og.stepped(sc, make), og.stepped(sc, make)
    recut = og.stepped(sc, lambda grid: NativeTileMesh(LocationHash2D(**grid), (2, 2), 1))
    single = og.stepped(sc, lambda grid: Simulation(LocationHash2D(**grid)))
    with og.released(mesh, twin, recut, single):
        rec = single.read_agents()
        rects = mesh.tile_rects()
        assert rec.tobytes() == mesh.read_agents().tobytes() and (mesh.tile_counts() > 0).sum() >= 3
        assert rects.tolist() != og.rects_of([0, sc.rows // 2, sc.rows], [0, sc.cols // 2, sc.cols]).tolist()  # (uneven)
        gates = cut_gates(sc, rects, rec)
        stats = {}
        want = agree(single, rec, sc.grid, gates, INF, name="the engine", stats=stats)
        print(f"    {stats}")
        assert min(stats.values()) > 0
        rows, counts = agree(mesh, rec, sc.grid, gates, INF, name="2 x 2 tiles", want=want)
        across = both_sides(sc, rects, rec, rows)
        print(f"{across} gates with agents of more than one tile")
        assert across >= 5  # (no tile alone gives their rows)
        # a prefix: cap below the count, nothing written beyond it, the counts whole
        for cap in (1, len(rows) // 2):
            got, per, out = call(mesh, gates, INF, cap=cap)
            assert got == len(rows) and per.tobytes() == counts.tobytes()
            assert out[:cap].tobytes() == rows[:cap].tobytes() and (out[cap:].view(np.uint8) == 0xAB).all()
        # a filter: the far side of both cuts
        far = selection(_abi.CS_SEL_RECT, x0=float(np.median(rec["x"])), y0=float(np.median(rec["y"])), x1=INF, y1=INF)
        f_want = agree(single, rec, sc.grid, gates, INF, far, name="a filter (engine)")
        agree(mesh, rec, sc.grid, gates, INF, far, name="a filter (mesh)", want=f_want)
        assert 0 < len(f_want[0]) < len(rows)
        # refusals agree with the engine's, leave the mesh usable and write nothing
        bad = gates.copy()
        bad["t1"][5] = -1.0
        nan = gates.copy()
        nan["by"][7] = float("nan")
        for g, speed_max, text in ((bad, 2.0, "gate_crossings: gate 5"), (nan, 2.0, "gate_crossings: gate 7"),
                                   (gates, -1.0, "gate_crossings: speed_max")):
            texts = []
            for t in (mesh, single):
                n, per, out = call(t, g, speed_max, cap=8)
                assert n == SIZE_MAX and (out.view(np.uint8) == 0xAB).all() and (per.view(np.uint8) == 0xAB).all()
                texts.append(last_error(t))
            assert texts[0] == texts[1] and text in texts[0]
        # the Python surface of the mesh
        got, per = mesh.gate_crossings(gates, INF)
        assert got.tobytes() == rows.tobytes() and per.tobytes() == counts.tobytes()
        assert mesh.gate_crossings(gates, INF, limit=9)[0].tobytes() == rows[:9].tobytes()
        assert mesh.count_gate_crossings(gates, INF).tobytes() == counts.tobytes()
        assert mesh.gate_crossings(gates[:0], 2.0)[0].shape == (0,)
        assert mesh.read_agents().tobytes() == rec.tobytes()
        # after a re-cut: a mesh created on even cuts, moved to the crowd's own
        before = recut.tile_rects().tolist()
        recut.recut()
        assert recut.tile_rects().tolist() != before and recut.read_agents().tobytes() == rec.tobytes()
        agree(recut, rec, sc.grid, cut_gates(sc, recut.tile_rects(), rec), INF, name="after a re-cut")
        # the next steps are those of a mesh that never asked
        for t in (mesh, twin):
            for _ in range(5):
                t.step(og.DT)
        assert mesh.read_agents().tobytes() == twin.read_agents().tobytes()


def _two_rank_gates(sc, rec, cut):
    return cut_gates(sc, og.rects_of([0, cut, sc.rows], [0, sc.cols]), rec)


def _two_rank_answers(t, sc, rec, cut):
    """per query: (the count listing everything, the rows' bytes, the counts' bytes, the count of a prefix, its bytes, the
    count and the counts of the count-only form); then whether the two refusals were refused, and their texts"""
    gates = _two_rank_gates(sc, rec, cut)
    low = selection(_abi.CS_SEL_RECT, x0=-INF, y0=-INF, x1=sc.grid["offset"][0] + cut * sc.cell, y1=INF)  # one rank's side
    out = []
    for sel in (None, low):
        total = call(t, gates, INF, sel, cap=0, rows=False)[0]
        n, per, rows = call(t, gates, INF, sel, cap=total, fill=0xEE)
        m, _, head = call(t, gates, INF, sel, cap=total // 3, fill=0xEE)
        k, only, _ = call(t, gates, INF, sel, cap=0, rows=False)
        out.append((n, rows.tobytes(), per.tobytes(), m, head.tobytes(), k, only.tobytes()))
    bad = gates.copy()
    bad["t0"][4] = -2.0
    refused = []
    for g, sel in ((bad, None), (gates, selection(1 << 9))):
        n, per, rows = call(t, g, INF, sel, cap=4)
        refused.append((n == SIZE_MAX, last_error(t), bool((rows.view(np.uint8) == 0xAB).all() and (per.view(np.uint8) == 0xAB).all())))
    return out, refused


def _rank_lists_gate_crossings(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import TorchHostTransport
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sc = og.scene("lopsided")
        mesh = og.stepped(sc, lambda grid: NativeTileMesh(LocationHash2D(**grid), (2, 1), 1, device=0, rank=rank, n_ranks=world,
                                                          host_transport=TorchHostTransport(dist)))
        mesh.recut()  # (collective: the cut moves to the crowd's own)
        cut = int(mesh.tile_rects().tolist()[0][rank ^ 1])  # (a rank lists its own tile: its edge towards the other)
        before = mesh.read_agents()
        notes = {"cut": cut, "before": before, "answers": _two_rank_answers(mesh, sc, before, cut)}
        gates = _two_rank_gates(sc, before, cut)
        notes["python"] = mesh.gate_crossings(gates, INF)
        for _ in range(5):
            mesh.count_gate_crossings(gates, 2.0)
            mesh.step(og.DT)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_give_the_rows_of_one_engine(tmp_path):
    """Two ranks (2 x 1 tiles, re-cut to the crowd's own uneven cut) over torch.distributed / gloo sharing the GPU: the
    counts and the rows travel through the host transport's gathers, every rank gets the whole answer, the single
    engine's, refuses what it refuses with its words, and steps on as it."""
    import pickle
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "gates.pkl")
    procs = [ctx.Process(target=_rank_lists_gate_crossings, args=(r, 2, 29831, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    notes = []
    for r in range(2):
        with open(f"{out}.{r}", "rb") as f:
            notes.append(pickle.load(f))
    sc = og.scene("lopsided")
    single = og.stepped(sc, lambda grid: Simulation(LocationHash2D(**grid)))
    with og.released(single):
        before = single.read_agents()
        cut = notes[0]["cut"]
        assert notes[1]["cut"] == cut and 2 <= cut < sc.rows - 2 and cut != sc.rows // 2  # (uneven)
        want, refused = _two_rank_answers(single, sc, before, cut)
        gates = _two_rank_gates(sc, before, cut)
        rows, counts = crossings(before, sc.grid, gates, INF)
        assert want[0][0] == len(rows) > 300 and want[0][1][:rows.nbytes] == rows.tobytes()
        assert want[0][2] == counts.tobytes() == want[0][6] and want[0][3] == want[0][5] == len(rows)
        assert 0 < want[1][0] < len(rows) and all(r[0] and r[2] for r in refused) and "gate 4" in refused[0][1]
        assert both_sides(sc, og.rects_of([0, cut, sc.rows], [0, sc.cols]), before, rows) >= 5  # (rows of both ranks in one gate)
        for _ in range(5):
            single.step(og.DT)
        end = single.read_agents()
        for n in notes:
            assert n["before"].tobytes() == before.tobytes()
            assert n["answers"] == (want, refused)
            assert n["python"][0].tobytes() == rows.tobytes() and n["python"][1].tobytes() == counts.tobytes()
            assert len(end) > 400 and n["agents"].tobytes() == end.tobytes()
