"""The between-step device calls on a tile mesh whose cuts are neither even nor where they were: weighted and placed cuts
at creation (cs_mesh_desc::weights_xy) and cuts moved under a running crowd (cs_mesh_recut, which empties every tile,
gives it a new origin, extent, row stride, cell tables and halo buffers, and fills it again from exported records).  After
every change of geometry the mesh answers every call as the single engine and as the numpy restatement on the engine's
OWN read_agents(), byte for byte (the raster's velocity sums within field_reference.tolerance): write_agents, the by-id
reads, selections and counts, remove_selected, rasters, close pairs, clusters, neighbours, encounters, rays, leg
conflicts and leg intervals (odd_grids.ask_mesh_as_engine), set_targets, the owners of spawned agents and 64-bit ids.

The scenes (odd_grids.scene): "lopsided", three lattices of 1,800, 900 and 400 agents in an L on 172 x 118 cells of
0.7 m, so that with even 2 x 2 cuts one tile holds nobody and the crowd's own cuts pass through the largest lattice, far
from the middle; "diagonal", two lattices of 1,000, so that two tiles hold nobody before and after a re-cut.  Their floors
are counted by tiles.TileLayout and numpy alone (odd_grids.recut_floors) before a mesh is asked.  Needs an MI355X."""
import numpy as np
import pytest

import odd_grids as og
from rmf_crowdsim_amd import (CS_CFG_WIDE_IDS, LocationHash2D, MonotonicCrowd, NoLocalPlan, Simulation, SourceSink,
                              StubHighLevelPlan, _abi)
from rmf_crowdsim_amd.tiles import NativeTileMesh
from select_reference import Ledger, count, drain, keep_events, select, selection
from set_targets_scenes import Host, lattice

pytestmark = pytest.mark.gpu
CS_CFG_TILE_OVERLAP = _abi.CS_CFG_TILE_OVERLAP
BOOKED, PLANNED = 1, 2


def _twins(sc, make_mesh, steps=og.STEPS):
    return og.stepped(sc, make_mesh, steps=steps), og.stepped(sc, lambda grid: Simulation(LocationHash2D(**grid)), steps=steps)


def _same(mesh, single):
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    return rec


def _write_astride(mesh, single, sc, rects):
    """agents written astride every cut of `rects` on both twins and read back by id -> (written, records)"""
    w = og.astride_cuts(sc, single.read_agents(), rects, apart=True)
    for t in (mesh, single):
        t.write_agents(w, fields=("position",))
    rec = _same(mesh, single)
    for t in (mesh, single):
        og.ask_by_id(t, rec, w["id"][::-1], sc.name)
    return w, rec


# ---- a. weighted and placed cuts at creation ------------------------------------------------------------------------------
# (shape, halo, the rows or columns of the placed cuts; None: weights = the crowd's own points).  Row and column 24 pass
# through the densest part of the largest lattice (rows 8-40, columns 10-38); the middle tile is two halo rings thick.
PLACED = [((2, 2), 1, None), ((3, 1), 1, (24, 26)), ((3, 1), 2, (24, 28)), ((1, 3), 1, (24, 26)), ((1, 3), 2, (24, 28))]


@pytest.mark.parametrize("shape,halo,placed", PLACED, ids=[f"{s[0]}x{s[1]}-halo{h}" for s, h, _ in PLACED])
def test_weighted_and_placed_cuts_answer_every_call_as_one_engine(shape, halo, placed, monkeypatch):
    sc = og.scene("lopsided")
    if placed is None:
        weights = np.concatenate([p for p, _ in sc.parts])
        lay = og.layout(sc, shape, halo, points=weights)
        want = og.rects_of(lay.x_edges, lay.y_edges)
        assert lay.x_edges[1] <= 51 and lay.y_edges[1] <= 78  # (both cuts at least 8 cells from the even ones: 59 and 86)
    else:
        rows, cols = (placed, ()) if shape[1] == 1 else ((), placed)
        weights = og.placed_cut_weights(sc, shape, rows, cols, halo)
        want = og.rects_of([0, *rows, sc.rows], [0, *cols, sc.cols])
    mesh, single = _twins(sc, lambda grid: NativeTileMesh(LocationHash2D(**grid), shape, halo, weights=weights))
    with og.released(mesh, single):
        rects = mesh.tile_rects()
        assert rects.tolist() == want.tolist()
        assert all(int(r[1]) - int(r[0]) != int(r[3]) - int(r[2]) for r in rects)  # (no tile is square)
        _same(mesh, single)
        w = og.astride_cuts(sc, single.read_agents(), rects)
        for t in (mesh, single):
            t.write_agents(w, fields=("position",))
        rec = _same(mesh, single)
        if placed is None:
            assert (mesh.tile_counts() >= 100).all()
            og.cut_floor(sc, rec, rects, halo * sc.cell)
        else:
            og.thin_tile_floors(sc, rec, rects, 1, halo)
        # (at halo 2 the distance queries also run at 2.0 cells, the limit)
        og.ask_mesh_as_engine(mesh, single, sc, rec, f"lopsided, cuts {og.cuts_of(rects)}, halo {halo}", halo, 1.0, monkeypatch,
                              cells=(0.6, 1.0, 2.0) if halo == 2 else None, by_id=w["id"][::-1])


# ---- b. every call, a re-cut, every call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, CS_CFG_TILE_OVERLAP], ids=["plain", "overlap"])
def test_every_call_a_recut_every_call(flags, monkeypatch):
    sc = og.scene("lopsided")
    mesh, single = _twins(sc, lambda grid: NativeTileMesh(LocationHash2D(**grid), (2, 2), 1, flags=flags))
    with og.released(mesh, single):
        rec = _same(mesh, single)
        even, cut, n_after = og.recut_floors(sc, rec)  # (TileLayout and numpy alone)
        assert mesh.tile_rects().tolist() == even.tolist() and mesh.tile_counts().ravel().tolist().count(0) == 1
        empty = int(np.argmin(mesh.tile_counts().ravel()))
        # 2. the whole body on the even cuts: every scratch of every engine exists at the old geometry (the 130 x 130
        #    raster and a pair list among them)
        w, rec = _write_astride(mesh, single, sc, even)
        og.cut_floor(sc, rec, even, sc.cell)
        og.ask_mesh_as_engine(mesh, single, sc, rec, "lopsided, even cuts", 1, 1.0, monkeypatch, by_id=w["id"], removal=False)
        # 3. the re-cut (the agents astride the old cuts have moved the histograms: the floors once more, on these records;
        #    four of them stand in the tile that held nobody)
        even, cut, n_after = og.recut_floors(sc, rec, empty_before=0)
        assert mesh.tile_counts().ravel()[empty] == 4
        counts = mesh.recut()
        rects = mesh.tile_rects()
        print(f"re-cut: {even.tolist()} -> {rects.tolist()}, tiles hold {counts.ravel().tolist()}")
        assert counts.sum() == len(rec) and (counts >= 100).all() and counts.ravel()[empty] >= 100
        assert rects.tolist() == cut.tolist() and counts.ravel().tolist() == n_after.tolist()
        assert mesh.read_agents().tobytes() == rec.tobytes()
        # 4. no step in between: agents astride the NEW cuts, read by id, the whole body
        w, rec = _write_astride(mesh, single, sc, rects)
        og.cut_floor(sc, rec, rects, sc.cell)
        og.ask_mesh_as_engine(mesh, single, sc, rec, "lopsided, after the re-cut", 1, 1.0, monkeypatch, by_id=w["id"][::-1],
                              removal=False)
        # 5. a step, the body again
        for t in (mesh, single):
            t.step(og.DT)
        rec = _same(mesh, single)
        assert np.isfinite(rec["x"]).all() and np.isfinite(rec["vy"]).all()
        og.ask_mesh_as_engine(mesh, single, sc, rec, "lopsided, a step after the re-cut", 1, 1.0, monkeypatch, by_id=w["id"],
                              removal=False)
        # 6. the high quadrant leaves both
        for t, who in ((single, "engine"), (mesh, "mesh")):
            og.ask_removal(t, sc, rec, f"lopsided, after the re-cut ({who})")
        # 7. five steps, a second re-cut
        for _ in range(5):
            for t in (mesh, single):
                t.step(og.DT)
        rec = _same(mesh, single)
        second = og.layout(sc, (2, 2), 1, rec=rec)
        counts = mesh.recut()
        assert mesh.tile_rects().tolist() == og.rects_of(second.x_edges, second.y_edges).tolist() != rects.tolist()
        assert counts.sum() == len(rec) and mesh.read_agents().tobytes() == rec.tobytes()
        # 8. the distance queries, the rays and both leg calls once more
        og.ask_mesh_as_engine(mesh, single, sc, rec, "lopsided, after the second re-cut", 1, 1.0, monkeypatch, removal=False,
                              families=("near", "rays", "legs", "intervals"))
        # 9. and on
        for _ in range(5):
            for t in (mesh, single):
                t.step(og.DT)
        rec = _same(mesh, single)
        assert np.isfinite(rec["x"]).all()


# ---- c. tiles that hold nobody --------------------------------------------------------------------------------------------
def test_tiles_that_hold_nobody_before_and_after_a_recut(monkeypatch):
    sc = og.scene("diagonal")
    mesh, single = _twins(sc, lambda grid: NativeTileMesh(LocationHash2D(**grid), (2, 2), 1))
    with og.released(mesh, single):
        rec = _same(mesh, single)
        even, cut, n_after = og.recut_floors(sc, rec, empty_before=2, empty_after=2)
        assert mesh.tile_rects().tolist() == even.tolist() and mesh.tile_counts().ravel().tolist().count(0) == 2
        some = rec["id"][::97]
        og.ask_mesh_as_engine(mesh, single, sc, rec, "diagonal, even cuts", 1, 1.0, monkeypatch, by_id=some, removal=False)
        counts = mesh.recut()
        assert mesh.tile_rects().tolist() == cut.tolist() and counts.ravel().tolist() == n_after.tolist()
        assert counts.ravel().tolist().count(0) == 2 and mesh.read_agents().tobytes() == rec.tobytes()
        og.ask_mesh_as_engine(mesh, single, sc, rec, "diagonal, after the re-cut", 1, 1.0, monkeypatch, by_id=some[::-1],
                              removal=False)
        # 16 agents, eight of either lattice, into a tile that has never held anybody: a 4 x 4 lattice 0.6 cell apart
        k = int(np.flatnonzero(counts.ravel() == 0)[0])
        x0, x1, y0, y1 = (int(v) for v in cut[k])
        w = rec[np.linspace(0, len(rec) - 1, 16).astype(np.int64)].copy()
        ox, oy = sc.grid["offset"]
        j = np.arange(16)
        w["x"] = ox + ((x0 + x1) // 2 + 0.2 + 0.6 * (j % 4)) * sc.cell
        w["y"] = oy + ((y0 + y1) // 2 + 0.2 + 0.6 * (j // 4)) * sc.cell
        w["vx"], w["vy"] = 0.0, 0.0
        for t in (mesh, single):
            t.write_agents(w, fields=("position", "velocity"))
        rec = _same(mesh, single)
        assert mesh.tile_counts().ravel()[k] == 16 and mesh.tile_counts().ravel().tolist().count(0) == 1
        og.ask_mesh_as_engine(mesh, single, sc, rec, "diagonal, 16 agents in an empty tile", 1, 1.0, monkeypatch,
                              by_id=w["id"][::-1])
        for t in (mesh, single):
            t.step(og.DT)
        _same(mesh, single)


# ---- d. routes across a re-cut --------------------------------------------------------------------------------------------
GOALS = [(62.0, 22.0), (64.0, 66.0), (22.0, 64.0), (74.0, 44.0)]
SPEED, ARRIVE = 3.0, 0.2  # (a step is 0.3 m: under two arrival radii, so no waypoint is stepped over and circled)


def _routed(sim_cls):
    """900 route followers in the low corner of the 80 x 80 cells of set_targets_scenes.Host (a 2 x 2 mesh cuts at 80 m);
    routes are booked by hash cells of 1 m, the spacing of the crowd: most agents plan a route of their own"""
    h = Host(sim_cls, False, scale=1.0, arrive=ARRIVE, speed=SPEED)
    h.ids = h.sim.add_agents(lattice(30, 30, 1.0, (10.0, 10.0), 0.15, 5), h.hlp, NoLocalPlan(), 2.0)
    return h


def test_routes_travel_with_their_agents_across_a_recut():
    """set_targets, a few steps, a re-cut while everybody is under way, set_targets for a second batch that includes agents
    whose tile has changed, then on to arrival: the route cache entry and meta (group | waypoint) travel in the exported
    record.  Positions, velocities and next_waypoint are the single engine's byte for byte at every tenth step."""
    mesh, one = _routed(lambda index, **kw: NativeTileMesh(index, (2, 2), 1, **kw)), _routed(Simulation)
    ids = one.ids
    assert mesh.ids == ids
    for h in (mesh, one):
        h.send(ids, [GOALS[i % 4] for i in ids])
        for _ in range(30):
            h.sim.step(0.1)
    rec = one.sim.read_agents()
    assert rec.tobytes() == mesh.sim.read_agents().tobytes()
    before = mesh.sim.tile_rects()
    counts = mesh.sim.recut()
    after = mesh.sim.tile_rects()
    assert mesh.sim.read_agents().tobytes() == rec.tobytes()
    row, col = np.floor(rec["x"] / 2.0).astype(np.int64), np.floor(rec["y"] / 2.0).astype(np.int64)

    def owner(rects):
        r = rects.astype(np.int64)
        inside = (row[:, None] >= r[:, 0]) & (row[:, None] < r[:, 1]) & (col[:, None] >= r[:, 2]) & (col[:, None] < r[:, 3])
        return inside.argmax(axis=1)
    changed = owner(before) != owner(after)
    some = [i for i in ids if i % 3 == 0]
    sent_changed = int(changed[np.isin(rec["id"], np.asarray(some, dtype=np.uint64))].sum())
    print(f"re-cut under way: {before.tolist()} -> {after.tolist()}, tiles hold {counts.ravel().tolist()}; {int(changed.sum())} "
          f"agents changed tile, {sent_changed} of them are sent again")
    assert abs(int(after[3][0]) - 40) >= 8 and abs(int(after[3][2]) - 40) >= 8 and (counts >= 100).all()
    assert sent_changed >= 20
    for h in (mesh, one):
        h.send(some, [GOALS[(i + 1) % 4] for i in some])
    assert mesh.statuses == one.statuses and len(one.statuses) == 1200 and set(one.statuses) <= {BOOKED, PLANNED}
    print(f"planned routes: {one.statuses[:900].count(PLANNED)} of 900, after the re-cut {one.statuses[900:].count(PLANNED)} of 300")
    assert one.statuses[900:].count(PLANNED) > 100  # (routes planned after the re-cut, by every tile alike)
    lo_m = lo_1 = 0
    for hi_m, hi_1 in zip(mesh.marks, one.marks):  # (every tile plans what the single engine plans, after the re-cut too)
        assert hi_1 > lo_1 and mesh.routes.calls[lo_m:hi_m] == 4 * one.routes.calls[lo_1:hi_1]
        lo_m, lo_1 = hi_m, hi_1
    # the longest route: a dogleg (2 m aside at the midpoint) from the far corner of the crowd, then another from wherever
    # the agent was when it was sent again: under 2 x 80 m
    steps = int(160.0 / (SPEED * 0.1))
    under_way = 0
    for k in range(steps):
        for h in (mesh, one):
            h.sim.step(0.1)
        if k % 10 == 9:
            a = one.sim.read_agents()
            assert a.tobytes() == mesh.sim.read_agents().tobytes(), k
            under_way += int((np.hypot(a["vx"], a["vy"]) > 0.5 * SPEED).sum() > 100)
    assert under_way >= 5  # (compared while they walk, not only at rest)
    a = one.sim.read_agents()
    goal = np.array([GOALS[(i + 1) % 4] if i % 3 == 0 else GOALS[i % 4] for i in a["id"].tolist()])
    away = np.hypot(a["x"] - goal[:, 0], a["y"] - goal[:, 1])
    print(f"after {steps} steps the agents are at most {away.max():.3f} m from their goals")
    assert away.max() <= ARRIVE + SPEED * 0.1  # (arrived: inside `arrive`, or one step's walk past it)


# ---- e. owners across a re-cut --------------------------------------------------------------------------------------------
def _owned_scene(t):
    """the scene of test_gpu_select_mesh.py, a second source-sink whose first waypoint lies 0.6 m from the source (its
    agents are past it within a second: their waypoint counter travels in the exported record's meta word), and 400
    standers in the low corner, which pull the crowd's cuts away from the middle"""
    from test_gpu_agent_write_mesh import _scene
    _scene(t)
    lp = NoLocalPlan()
    t.walkers = StubHighLevelPlan((0.0, 1.0))
    t.sink2 = t.add_source_sink(SourceSink(source=np.array([50.0, 8.0]), radius_sink=0.5, crowd_generator=MonotonicCrowd(20.0),
                                           high_level_planner=t.walkers, local_planner=lp,
                                           waypoints=[np.array([50.0, 8.6]), np.array([50.0, 52.0])], loop_forever=False,
                                           agent_eyesight_range=2.0))
    t.standers = StubHighLevelPlan((0.0, 0.0))
    t.add_agents(lattice(20, 20, 0.5, (2.0, 2.0), 0.0, 0), t.standers, lp, 2.0)


def test_owners_across_a_recut():
    from test_gpu_agent_write_mesh import GRID
    mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 2), 1)
    single = Simulation(LocationHash2D(**GRID))
    led = Ledger(single).watch()
    for t in (mesh, single):
        _owned_scene(t)
        keep_events(t)
    for _ in range(25):
        for t in (mesh, single):
            t.step(0.05)
    led.hear(drain(single))
    drain(mesh)
    rec = _same(mesh, single)
    # (asked once before the re-cut: the group tables of every tile's selections exist at the old geometry)
    assert mesh.select_agents(source_sink=0).tolist() == single.select_agents(source_sink=0).tolist()
    past = rec[np.isin(rec["id"], single.select_agents(source_sink=1)) & (rec["next_waypoint"] > 0)]
    print(f"{len(past)} agents of the second sink are past their first waypoint")
    assert len(past) >= 2
    before = mesh.tile_rects()
    counts = mesh.recut()
    after = mesh.tile_rects()
    print(f"re-cut: {before.tolist()} -> {after.tolist()}, tiles hold {counts.ravel().tolist()}")
    assert int(after[3][0]) <= 13 and int(after[3][2]) <= 13 and (counts > 0).all()  # (from 15: both cuts moved)
    assert mesh.read_agents().tobytes() == rec.tobytes()
    assert mesh.sink2 == single.sink2 == 1
    # (selection by the C entry point, the keywords of the Python surface on twin t)
    sels = [("sink 0", selection(_abi.CS_SEL_SOURCE_SINK, source_sink=0), lambda t: dict(source_sink=0)),
            ("sink 1", selection(_abi.CS_SEL_SOURCE_SINK, source_sink=1), lambda t: dict(source_sink=1))]
    for name in ("walkers", "standers"):
        handle = led._handles(getattr(single, name))[0]
        assert mesh._handles[id(getattr(mesh, name))] == handle  # (both number their planners in the order given)
        sels.append((name, selection(_abi.CS_SEL_HLP, hlp=handle), lambda t, name=name: dict(high_level_planner=getattr(t, name))))
    for name, sel, terms in sels:
        want = led.expected(sel, rec).tolist()
        print(f"{name}: {len(want)}")
        assert len(want) >= 2
        for t in (mesh, single):
            n, ids = select(t, sel)
            assert n == len(want) and ids.tolist() == want, name
            assert t.select_agents(**terms(t)).tolist() == want, name
    for t in (mesh, single):
        rc, counts = count(t, [s for _, s, _ in sels])
        assert rc == 0 and counts.tolist() == [len(led.expected(s, rec)) for _, s, _ in sels]
    assert len(led.expected(sels[3][1], rec)) == 400
    for t in (mesh, single):
        t.remove_source_sink(0, with_agents=True)
    assert len(_same(mesh, single)) < len(rec)
    n_before = len(single)
    for _ in range(10):
        for t in (mesh, single):
            t.step(0.05)
    led.hear(drain(single))
    drain(mesh)
    rec = _same(mesh, single)
    assert len(rec) > n_before  # (the second sink went on spawning, alike on both)
    for t in (mesh, single):
        assert len(t.select_agents(source_sink=0)) == 0
        assert t.select_agents(source_sink=int(single.sink2)).tolist() == led.expected(sels[1][1], rec).tolist()


# ---- f. wide ids ----------------------------------------------------------------------------------------------------------
def test_wide_ids_across_a_recut(monkeypatch):
    """64-bit ids from 2^40 on (CS_CFG_WIDE_IDS): after a re-cut close pairs, rays and leg intervals answer by external id"""
    sc = og.scene("lopsided")
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(2 ** 40 + 1))
    mesh = sc.populate(NativeTileMesh(LocationHash2D(**sc.grid), (2, 2), 1, flags=CS_CFG_WIDE_IDS))
    single = sc.populate(Simulation(LocationHash2D(**sc.grid), flags=CS_CFG_WIDE_IDS))
    monkeypatch.delenv("CS_FIRST_AGENT_ID")
    with og.released(mesh, single):
        for _ in range(og.STEPS):
            for t in (mesh, single):
                t.step(og.DT)
        rec = _same(mesh, single)
        assert int(rec["id"].min()) > 2 ** 40
        even, cut, n_after = og.recut_floors(sc, rec)
        counts = mesh.recut()
        assert mesh.tile_rects().tolist() == cut.tolist() and counts.ravel().tolist() == n_after.tolist()
        assert mesh.read_agents().tobytes() == rec.tobytes()
        w, rec = _write_astride(mesh, single, sc, cut)
        og.cut_floor(sc, rec, cut, sc.cell)
        og.ask_mesh_as_engine(mesh, single, sc, rec, "lopsided, wide ids, after the re-cut", 1, 1.0, monkeypatch,
                              by_id=w["id"][::-1], removal=False, families=("near", "rays", "intervals"))
        for t in (mesh, single):
            t.step(og.DT)
        _same(mesh, single)


# ---- g. two ranks over a host transport -----------------------------------------------------------------------------------
def _rank_recuts(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import TorchHostTransport
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    patch = pytest.MonkeyPatch()
    try:
        sc = og.scene("lopsided")
        mesh = og.stepped(sc, lambda grid: NativeTileMesh(LocationHash2D(**grid), (2, 1), 1, device=0, rank=rank, n_ranks=world,
                                                          host_transport=TorchHostTransport(dist)))
        notes = {"before": mesh.tile_rects().tolist(), "stepped": mesh.read_agents()}
        mesh.recut()
        notes["after"] = mesh.tile_rects().tolist()
        rec = mesh.read_agents()
        w = og.astride_cuts(sc, rec, og.rects_of([0, notes["after"][0][rank ^ 1], sc.rows], [0, sc.cols]), apart=True)
        mesh.write_agents(w, fields=("position",))
        notes["written"] = rec = mesh.read_agents()
        # one call of each family (the distance queries at one cell, no roles), each against the restatement on `rec`
        og.ask_mesh_as_engine(mesh, None, sc, rec, f"lopsided, rank {rank}", 1, 1.0, patch, cells=(1.0,), roles=False,
                              by_id=w["id"][::-1], removal=False)
        for _ in range(5):
            mesh.step(og.DT, report=False)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        patch.undo()
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_recut_and_answer_as_one_engine(tmp_path, monkeypatch):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU: a collective recut(), one write astride the
    new cut, one call of each family, which every rank compares with the restatement on the records it reads (a failed
    comparison ends the rank with a non-zero exit code), five steps.  The parent asks the single engine the same and
    compares what the ranks read with what it holds."""
    import pickle
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "recut.pkl")
    procs = [ctx.Process(target=_rank_recuts, args=(r, 2, 29871, out)) for r in range(2)]
    for p in procs:
        p.start()
    sc = og.scene("lopsided")  # (the single engine's part, while the ranks run)
    single = og.stepped(sc, lambda grid: Simulation(LocationHash2D(**grid)))
    with og.released(single):
        stepped = single.read_agents()
        cut = og.layout(sc, (2, 1), 1, rec=stepped)
        w = og.astride_cuts(sc, stepped, og.rects_of(cut.x_edges, cut.y_edges), apart=True)
        single.write_agents(w, fields=("position",))
        written = single.read_agents()
        og.cut_floor(sc, written, og.rects_of(cut.x_edges, cut.y_edges), sc.cell)
        og.ask_mesh_as_engine(None, single, sc, written, "lopsided, the single engine", 1, 1.0, monkeypatch, cells=(1.0,),
                              roles=False, by_id=w["id"][::-1], removal=False)
        for _ in range(5):
            single.step(og.DT, report=False)
        end = single.read_agents()
    for p in procs:
        p.join(240)
    stuck = [p for p in procs if p.is_alive()]
    for p in stuck:
        p.terminate()
        p.join(10)
    assert not stuck and [p.exitcode for p in procs] == [0, 0]
    notes = []
    for r in range(2):
        with open(f"{out}.{r}", "rb") as f:
            notes.append(pickle.load(f))
    assert abs(cut.x_edges[1] - 59) >= 8
    for r, n in enumerate(notes):
        assert n["before"] == [[0, 59, 0, sc.cols], [59, sc.rows, 0, sc.cols]][r:r + 1]
        assert n["after"] == [[0, cut.x_edges[1], 0, sc.cols], [cut.x_edges[1], sc.rows, 0, sc.cols]][r:r + 1]
        assert n["stepped"].tobytes() == stepped.tobytes() and n["written"].tobytes() == written.tobytes()
        assert len(end) == 3100 and n["agents"].tobytes() == end.tobytes()
