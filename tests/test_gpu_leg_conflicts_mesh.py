"""Paths against the moving crowd on a tile mesh (cs_mesh_leg_conflicts; NativeTileMesh.leg_conflicts /
count_leg_conflicts / path_conflict): every tile runs all legs against the agents it owns, its walk clipped to its owned
cells, and the rows are merged by the minimum of (s, id); the mesh gives the single engine's answer byte for byte, which
is also the restatement's (tests/legs_reference.py), whatever distance, speed_max and t1 are.  No halo exchange is made for
it: the next steps of the mesh are those of a mesh that never asked."""
import numpy as np
import pytest

from rmf_crowdsim_amd import CS_CFG_WIDE_IDS, LocationHash2D, Simulation, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from legs_reference import NO_HIT, SIZE_MAX, agree, call, conflicts, last_error, legs_array
from select_reference import selection
from test_gpu_agent_write import _add_crossing
from test_gpu_encounters_mesh import _crowd
from test_gpu_leg_conflicts import leg_sets

pytestmark = pytest.mark.gpu
INF = float("inf")


def _same(mesh, single, rec, grid, legs, distance, speed_max, sel=None, name=""):
    """mesh == single engine == restatement; `sel` is a rectangle (no ledger needed)"""
    want = agree(single, rec, grid, legs, distance, speed_max, sel, name=name + " (engine)")
    agree(mesh, rec, grid, legs, distance, speed_max, sel, name=name + " (mesh)", want=want)
    return want


def _cut_legs(cuts_x, cuts_y):
    """Legs along every cut (on it, and 0.3 m to either side), legs across every cut in both senses, and waits standing
    on the cuts, all through the crowd (40 m to 127 m)"""
    at = np.linspace(42.0, 126.0, 29)
    start, vel = [], []
    for c in cuts_x:
        for d in (-0.3, 0.0, 0.3):
            start += [(c + d, y) for y in at]
            vel += [(0.0, 1.5 if k % 2 else -1.5) for k in range(len(at))]
        start += [(c - 3.0, y) for y in at] + [(c + 3.0, y + 0.4) for y in at] + [(c, y + 0.7) for y in at]
        vel += [(1.5, 0.0)] * len(at) + [(-1.5, 0.25)] * len(at) + [(0.0, 0.0)] * len(at)
    for c in cuts_y:
        for d in (-0.3, 0.0, 0.3):
            start += [(x, c + d) for x in at]
            vel += [(1.5 if k % 2 else -1.5, 0.0) for k in range(len(at))]
        start += [(x, c - 3.0) for x in at] + [(x + 0.4, c + 3.0) for x in at] + [(x + 0.7, c) for x in at]
        vel += [(0.0, 1.5)] * len(at) + [(0.25, -1.5)] * len(at) + [(0.0, 0.0)] * len(at)
    assert start
    return legs_array(start, vel, 0.5, 4.5)


@pytest.mark.parametrize("shape,halo", [((2, 2), 1), ((1, 3), 1)])
def test_a_mesh_answers_the_legs_as_one_engine(shape, halo):
    pts, group, grid = _crowd()
    mesh = NativeTileMesh(LocationHash2D(**grid), shape, halo)
    single = Simulation(LocationHash2D(**grid))
    for t in (mesh, single):
        _add_crossing(t, pts, group)
        for _ in range(40):
            t.step(0.05)
    rec = single.read_agents()
    # a few agents written far beyond the crowd, so that every tile of three holds somebody: x and y in [150, 200]
    w = rec[50:90].copy()
    rng = np.random.default_rng(5)
    w["x"], w["y"] = rng.uniform(150.0, 200.0, len(w)), rng.uniform(150.0, 200.0, len(w))
    w["x"][:10] = rng.uniform(42.0, 100.0, 10)
    for t in (mesh, single):
        t.write_agents(w, fields=("position",))
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    assert (mesh.tile_counts() > 0).sum() >= 3
    cell = grid["cell_size"]
    rows_, cols_ = int(grid["height"] / cell), int(grid["width"] / cell)
    cuts_x = [round(k * rows_ / shape[0]) * cell for k in range(1, shape[0])]
    cuts_y = [round(k * cols_ / shape[1]) * cell for k in range(1, shape[1])]
    pace = float(np.median(np.hypot(rec["vx"].astype(np.float64), rec["vy"].astype(np.float64))))
    legs = leg_sets(rec, grid)
    for distance, speed_max in ((0.5, INF), (1.0, pace), (3.0, 2.0), (0.2, INF)):  # (3 m: wider than a halo of one cell)
        _same(mesh, single, rec, grid, legs, distance, speed_max, name=f"{shape}, the leg sets, {(distance, speed_max)}")
    legs = _cut_legs(cuts_x, cuts_y)
    pos = {int(r["id"]): (float(r["x"]), float(r["y"])) for r in rec}
    sides = 0  # winners that stand on the far side of a cut from the leg's start
    for distance, speed_max in ((0.5, 2.0), (0.2, INF)):
        want = _same(mesh, single, rec, grid, legs, distance, speed_max, name=f"{shape}, legs at the cuts, {(distance, speed_max)}")
        hit = want["id"] != NO_HIT
        for l, h in zip(legs[hit], want[hit]):
            x, y = pos[int(h["id"])]
            sides += any((l["x0"] < c) != (x < c) for c in cuts_x) or any((l["y0"] < c) != (y < c) for c in cuts_y)
        print(f"{shape}, {(distance, speed_max)}: {int(hit.sum())} of {len(legs)} legs at the cuts conflict, {sides} so far beyond a cut")
    assert sides >= 20
    # the first to arrive stands two tiles away: only the agents beyond 144 m are targets, the legs start below 72 m
    far = selection(_abi.CS_SEL_RECT, x0=144.0, y0=144.0, x1=INF, y1=INF)
    there = rec[(rec["x"] >= 144.0) & (rec["y"] >= 144.0)]
    assert len(there) >= 20
    meet = np.column_stack([there["x"] + 4.0 * there["vx"], there["y"] + 4.0 * there["vy"]])  # where each is in 4 s
    chase = legs_array(np.column_stack([np.full(len(there), 50.0), np.full(len(there), 45.0)]),
                       (meet - np.array([50.0, 45.0])) / 4.0, 0.0, 4.5)
    want = _same(mesh, single, rec, grid, chase, 0.3, 2.0, far, name=f"{shape}, two tiles away")
    assert (want["id"] != NO_HIT).sum() >= len(there) // 2 and np.isin(want["id"][want["id"] != NO_HIT], there["id"]).all()
    everyone = _same(mesh, single, rec, grid, chase, 0.3, 2.0, None, name=f"{shape}, the same through the crowd")
    assert (everyone["s"] <= want["s"]).all()
    # refusals leave the mesh usable and write nothing
    bad = legs.copy()
    bad["vy"][5] = float("nan")
    for legs_, distance in ((bad, 0.2), (legs, -1.0)):
        n, out = call(mesh, legs_, distance, 2.0, fill=0xAB)
        assert n == SIZE_MAX and "leg_conflicts" in last_error(mesh) and (out.view(np.uint8) == 0xAB).all()
    assert "leg 5" in (call(mesh, bad, 0.2, 2.0), last_error(mesh))[1]
    # the Python surface of the mesh
    want = conflicts(rec, grid, legs, 0.5, 2.0)
    assert mesh.leg_conflicts(legs, 0.5, 2.0).tobytes() == want.tobytes()
    assert mesh.count_leg_conflicts(legs, 0.5, 2.0) == int((want["id"] != NO_HIT).sum())
    assert mesh.leg_conflicts(legs[:0], 0.5, 2.0).shape == (0,)
    at = rec[len(rec) // 2]
    path = ([(at["x"], at["y"]), (at["x"] + 3.0, at["y"]), (at["x"] + 3.0, at["y"]), (at["x"] + 3.0, at["y"] + 4.0)], [0.0, 2.0, 3.0, 6.0])
    assert mesh.path_conflict(*path, 0.5, 2.0, ignore=int(at["id"])) == single.path_conflict(*path, 0.5, 2.0, ignore=int(at["id"]))
    got = mesh.path_conflict(*path, 0.5, 2.0)
    assert got is not None and got[1] == 0.0 and got[2] == 0 and got[0] <= int(at["id"])
    assert mesh.read_agents().tobytes() == rec.tobytes()


def test_twins_and_wide_ids(monkeypatch):
    """2 x 2 tiles with 64-bit ids from 2^40 on: `ignore` in external ids, ids above 2^32 back; and the next steps of the
    mesh that asked are those of the mesh that never did."""
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(2 ** 40 + 1))
    pts, group, grid = _crowd()
    meshes = [NativeTileMesh(LocationHash2D(**grid), (2, 2), 1, flags=CS_CFG_WIDE_IDS) for _ in range(2)]
    single = Simulation(LocationHash2D(**grid), flags=CS_CFG_WIDE_IDS)
    monkeypatch.delenv("CS_FIRST_AGENT_ID")
    mesh, twin = meshes
    for t in (mesh, twin, single):
        _add_crossing(t, pts, group)
        for _ in range(10):
            t.step(0.05)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes() and int(rec["id"].min()) > 2 ** 40
    for k in range(10):
        legs = leg_sets(rec, grid)
        if k in (0, 9):
            want = _same(mesh, single, rec, grid, legs, 0.5, 2.0, name=f"wide ids, step {k}")
            hit = want["id"] != NO_HIT
            assert hit.sum() > 60 and int(want["id"][hit].min()) > 2 ** 40
            assert (want["id"][:48] != legs["ignore"][:48]).all() and int(legs["ignore"][:48].min()) > 2 ** 40
            first = np.arange(48, 96, 6)
            assert (want["s"][first] == 0.0).all() and (want["id"][first] <= legs["ignore"][first - 48]).all()
        else:
            assert 0 < call(mesh, legs, 0.5, 2.0, rows=False)[0] < len(legs)
        for t in (mesh, twin, single):
            t.step(0.05)
        rec = single.read_agents()
    assert mesh.read_agents().tobytes() == twin.read_agents().tobytes() == rec.tobytes()


def _two_rank_legs(rec, grid):
    legs = leg_sets(rec, grid)
    comb = np.linspace(5.0, 55.0, 26)
    across = legs_array(np.column_stack([np.full_like(comb, 20.0), comb]), (2.5, 0.0), 0.0, 8.0)  # over the cut at 30 m
    on_cut = legs_array(np.column_stack([np.full_like(comb, 30.0), comb]), (0.0, 0.0), 0.0, 6.0)
    return np.concatenate([legs, across, on_cut])


def _two_rank_answers(t, rec, grid):
    legs = _two_rank_legs(rec, grid)
    left = selection(_abi.CS_SEL_RECT, x0=0.0, y0=0.0, x1=30.0, y1=60.0)  # one rank's side
    out = []
    for distance, speed_max, sel in ((0.5, 2.0, None), (0.2, INF, None), (0.5, 2.0, left), (0.0, 2.0, None)):
        n, rows = call(t, legs, distance, speed_max, sel, fill=0xEE)
        out.append((n, rows.tobytes(), call(t, legs, distance, speed_max, sel, rows=False)[0]))
    return out


def _rank_checks_legs(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import TorchHostTransport
    from test_gpu_agent_write_mesh import GRID, _scene
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 1), 1, device=0, rank=rank, n_ranks=world,
                              host_transport=TorchHostTransport(dist))
        _scene(mesh)
        for _ in range(25):
            mesh.step(0.05, report=False)
        before = mesh.read_agents()
        notes = {"before": before, "answers": _two_rank_answers(mesh, before, GRID)}
        legs = _two_rank_legs(before, GRID)
        notes["refused"] = call(mesh, legs, float("nan"), 2.0)[0] == SIZE_MAX
        notes["python"] = mesh.leg_conflicts(legs, 0.5, 2.0)
        for _ in range(10):
            mesh.count_leg_conflicts(legs, 0.5, 2.0)
            mesh.step(0.05, report=False)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_give_the_rows_of_one_engine(tmp_path):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU: the rows travel through the host transport's
    gather, every rank gets the whole answer, the single engine's, and steps on as it."""
    import pickle
    import torch.multiprocessing as mp
    from test_gpu_agent_write_mesh import GRID, _scene
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "legs.pkl")
    procs = [ctx.Process(target=_rank_checks_legs, args=(r, 2, 29819, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    notes = []
    for r in range(2):
        with open(f"{out}.{r}", "rb") as f:
            notes.append(pickle.load(f))
    single = Simulation(LocationHash2D(**GRID))
    _scene(single)
    for _ in range(25):
        single.step(0.05, report=False)
    before = single.read_agents()
    want = _two_rank_answers(single, before, GRID)
    legs = _two_rank_legs(before, GRID)
    rows = conflicts(before, GRID, legs, 0.5, 2.0)
    assert want[0][1] == rows.tobytes() and 0 < want[0][0] < len(legs) and want[3][0] == 0
    x_of = dict(zip(before["id"].tolist(), before["x"].tolist()))
    hit = rows["id"] != NO_HIT
    assert any((float(l["x0"]) < 30.0) != (x_of[int(h["id"])] < 30.0) for l, h in zip(legs[hit], rows[hit]))  # (the other rank's)
    for _ in range(10):
        single.step(0.05, report=False)
    end = single.read_agents()
    for n in notes:
        assert n["before"].tobytes() == before.tobytes()
        assert n["answers"] == want and n["refused"]
        assert n["python"].tobytes() == rows.tobytes()
        assert len(end) > 400 and n["agents"].tobytes() == end.tobytes()
