"""Agents in polygon zones on a tile mesh (cs_mesh_zone_agents; NativeTileMesh.zone_agents / count_zone_agents): every
tile runs all zones against the agents it owns, its cell ranges clipped to its owned cells; the per-zone counts add and
the rows are merged by (zone, id); the mesh gives the single engine's answer byte for byte, which is also the
restatement's (tests/zones_reference.py).  The cuts are uneven: the crowd's own, at creation or after a re-cut.  No halo
exchange is made for it: the next steps of the mesh are those of a mesh that never asked."""
import numpy as np
import pytest

import odd_grids as og
from rmf_crowdsim_amd import LocationHash2D, Simulation, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from select_reference import selection
from test_gpu_zone_agents import room, zone_rings
from zones_reference import SIZE_MAX, agree, call, last_error, rect_ring, zone_agents, zones_array

pytestmark = pytest.mark.gpu
INF = float("inf")


def cut_rings(sc, rects, rec):
    """the zones of the single-engine tests and zones astride every cut of `rects`: a band of two cells along each cut,
    rooms and triangles over the crossing of the cuts, one ring per tile that is exactly its rectangle"""
    rings = zone_rings(rec, sc.grid, each=30)
    ox, oy = sc.grid["offset"]
    cell = sc.cell
    rows, cols = og.cuts_of(rects)
    for r in rows:
        rings += [rect_ring(ox + (r - 1) * cell, oy, ox + (r + 1) * cell, oy + sc.cols * cell),
                  rect_ring(ox + r * cell, oy, ox + (r + 1) * cell, oy + sc.cols * cell, reverse=True)]
    for c in cols:
        rings += [rect_ring(ox, oy + (c - 1) * cell, ox + sc.rows * cell, oy + (c + 1) * cell),
                  rect_ring(ox, oy + (c - 1) * cell, ox + sc.rows * cell, oy + c * cell, reverse=True)]
    for r in rows:
        for c in cols or [sc.cols // 2]:
            x, y = ox + r * cell, oy + c * cell
            rings += [room(x - 6.3, y - 5.1, 12.9, 11.7), np.array([(x - 9.0, y - 2.0), (x + 7.0, y - 6.0), (x + 1.0, y + 8.0)])]
    row, col = sc.cells_of(rec)
    for r in rows:  # rooms of about nine cells a side, centred on the cut beside the twelve agents nearest to it
        for a in rec[np.argsort(np.abs(row - r), kind="stable")[:12]]:
            rings.append(room(ox + r * cell - 3.1, float(a["y"]) - 3.3, 6.3, 6.7))
    for c in cols:
        for a in rec[np.argsort(np.abs(col - c), kind="stable")[:12]]:
            rings.append(room(float(a["x"]) - 3.3, oy + c * cell - 3.1, 6.7, 6.3))
    for x0, x1, y0, y1 in np.asarray(rects, dtype=np.int64).tolist():
        rings.append(rect_ring(ox + x0 * cell, oy + y0 * cell, ox + x1 * cell, oy + y1 * cell))
    return rings


def both_sides(sc, rects, rec, rows, zones):
    """how many zones have rows of agents of more than one tile"""
    owner = dict(zip(rec["id"].tolist(), og.owners(rects, sc, rec).tolist()))
    tiles = {}
    for z, i in zip(rows["zone"].tolist(), rows["id"].tolist()):
        tiles.setdefault(z, set()).add(owner[i])
    return sum(1 for t in tiles.values() if len(t) > 1)


def test_a_mesh_on_uneven_cuts_lists_the_zone_agents_of_one_engine():
    sc = og.scene("lopsided")
    weights = np.concatenate([p for p, _ in sc.parts])
    make = lambda grid: NativeTileMesh(LocationHash2D(**grid), (2, 2), 1, weights=weights)
    mesh, twin = og.stepped(sc, make), og.stepped(sc, make)
    single = og.stepped(sc, lambda grid: Simulation(LocationHash2D(**grid)))
    with og.released(mesh, twin, single):
        rec = single.read_agents()
        rects = mesh.tile_rects()
        assert rec.tobytes() == mesh.read_agents().tobytes() and (mesh.tile_counts() > 0).sum() >= 3
        assert rects.tolist() != og.rects_of([0, sc.rows // 2, sc.rows], [0, sc.cols // 2, sc.cols]).tolist()  # (uneven)
        zones, vertices = zones_array(cut_rings(sc, rects, rec))
        want = agree(single, rec, sc.grid, zones, vertices, name="the engine")
        rows, counts = agree(mesh, rec, sc.grid, zones, vertices, name="2 x 2 tiles", want=want)
        across = both_sides(sc, rects, rec, rows, zones)
        print(f"{across} zones with agents of more than one tile")
        assert across >= 20  # (no tile alone gives their rows)
        # a ring that is a tile's rectangle holds what the tile owns
        own = mesh.tile_counts().reshape(-1)
        assert counts[-len(own):].tolist() == own.tolist()
        # a prefix: cap below the count, nothing written beyond it, the counts whole
        for cap in (1, len(rows) // 2):
            got, per_zone, out = call(mesh, zones, vertices, cap=cap)
            assert got == len(rows) and per_zone.tobytes() == counts.tobytes()
            assert out[:cap].tobytes() == rows[:cap].tobytes() and (out[cap:].view(np.uint8) == 0xAB).all()
        # a filter: the far side of both cuts
        far = selection(_abi.CS_SEL_RECT, x0=float(np.median(rec["x"])), y0=float(np.median(rec["y"])), x1=INF, y1=INF)
        f_want = agree(single, rec, sc.grid, zones, vertices, far, name="a filter (engine)")
        agree(mesh, rec, sc.grid, zones, vertices, far, name="a filter (mesh)", want=f_want)
        assert 0 < len(f_want[0]) < len(rows)
        # refusals agree with the engine's, leave the mesh usable and write nothing
        bad = zones.copy()
        bad["count"][5] = 2
        nan = vertices.copy()
        nan[int(zones["first"][7]) + 1, 1] = float("nan")
        for (z, v), which in (((bad, vertices), 5), ((zones, nan), 7)):
            texts = []
            for t in (mesh, single):
                n, per_zone, out = call(t, z, v, cap=8)
                assert n == SIZE_MAX and (out.view(np.uint8) == 0xAB).all() and (per_zone.view(np.uint8) == 0xAB).all()
                texts.append(last_error(t))
            assert texts[0] == texts[1] and f"zone_agents: zone {which}" in texts[0]
        # the Python surface of the mesh
        got, per_zone = mesh.zone_agents((zones, vertices))
        assert got.tobytes() == rows.tobytes() and per_zone.tobytes() == counts.tobytes()
        assert mesh.zone_agents((zones, vertices), limit=9)[0].tobytes() == rows[:9].tobytes()
        assert mesh.count_zone_agents((zones, vertices)).tobytes() == counts.tobytes()
        assert mesh.zone_agents([])[0].shape == (0,) and mesh.zones_array([rect_ring(0, 0, 1, 1)])[0]["count"].tolist() == [4]
        assert mesh.read_agents().tobytes() == rec.tobytes()
        # the next steps are those of a mesh that never asked
        for t in (mesh, twin):
            for _ in range(5):
                t.step(og.DT)
        assert mesh.read_agents().tobytes() == twin.read_agents().tobytes()


def _two_rank_zones(sc, rec, cut):
    return zones_array(cut_rings(sc, og.rects_of([0, cut, sc.rows], [0, sc.cols]), rec))


def _two_rank_answers(t, sc, rec, cut):
    """per query: (the count listing everything, the rows' bytes, the counts' bytes, the count of a prefix, its bytes, the
    count and the counts of the count-only form); then whether the two refusals were refused, and their texts"""
    zones, vertices = _two_rank_zones(sc, rec, cut)
    low = selection(_abi.CS_SEL_RECT, x0=-INF, y0=-INF, x1=sc.grid["offset"][0] + cut * sc.cell, y1=INF)  # one rank's side
    out = []
    for sel in (None, low):
        total = call(t, zones, vertices, sel, cap=0, rows=False)[0]
        n, per_zone, rows = call(t, zones, vertices, sel, cap=total, fill=0xEE)
        m, _, head = call(t, zones, vertices, sel, cap=total // 3, fill=0xEE)
        k, only, _ = call(t, zones, vertices, sel, cap=0, rows=False)
        out.append((n, rows.tobytes(), per_zone.tobytes(), m, head.tobytes(), k, only.tobytes()))
    bad = zones.copy()
    bad["flags"][4] = 8
    refused = []
    for z, sel in ((bad, None), (zones, selection(1 << 9))):
        n, per_zone, rows = call(t, z, vertices, sel, cap=4)
        refused.append((n == SIZE_MAX, last_error(t), bool((rows.view(np.uint8) == 0xAB).all() and (per_zone.view(np.uint8) == 0xAB).all())))
    return out, refused


def _rank_lists_zone_agents(rank, world, port, out_path):
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
        zones = _two_rank_zones(sc, before, cut)
        notes["python"] = mesh.zone_agents(zones)
        for _ in range(5):
            mesh.count_zone_agents(zones)
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
    out = str(tmp_path / "zones.pkl")
    procs = [ctx.Process(target=_rank_lists_zone_agents, args=(r, 2, 29827, out)) for r in range(2)]
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
        zones, vertices = _two_rank_zones(sc, before, cut)
        rows, counts = zone_agents(before, sc.grid, zones, vertices)
        assert want[0][0] == len(rows) > 1000 and want[0][1][:rows.nbytes] == rows.tobytes()
        assert want[0][2] == counts.tobytes() == want[0][6] and want[0][3] == want[0][5] == len(rows)
        assert 0 < want[1][0] < len(rows) and all(r[0] and r[2] for r in refused) and "zone 4" in refused[0][1]
        assert both_sides(sc, og.rects_of([0, cut, sc.rows], [0, sc.cols]), before, rows, zones) >= 10  # (rows of both ranks in one zone)
        for _ in range(5):
            single.step(og.DT)
        end = single.read_agents()
        for n in notes:
            assert n["before"].tobytes() == before.tobytes()
            assert n["answers"] == (want, refused)
            assert n["python"][0].tobytes() == rows.tobytes() and n["python"][1].tobytes() == counts.tobytes()
            assert len(end) > 400 and n["agents"].tobytes() == end.tobytes()
