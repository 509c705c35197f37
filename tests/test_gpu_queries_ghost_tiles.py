"""The between-step device calls on tile engines whose arrays HOLD GHOSTS: the state between a halo unpack (or a ghost
spawn) and the step, which a host reaches by driving the split calls (cs_halo_pack*, move the buffers, cs_halo_unpack*,
ask), as tiles.LocalTileMesh and DistributedTiles do.  There `owned_only = tile && ghosts_present` is set, and
include/crowdstep_state.h promises for every call that only owned agents match, count or take part.  After a step a tile
holds exactly the agents it stepped, so no other module takes these branches.

The truth comes from a single engine stepped alike: tile k owns rec[owners(rects, sc, rec) == k], its ring holds the
records in its rectangle grown by `halo` cells (odd_grids.held_by_tiles: TileLayout and numpy alone).  Every answer of a
tile engine is the numpy restatement's on the records it owns, byte for byte (odd_grids.ask_tile_with_ghosts); before each
call the restatement alone shows that the ghosts would change the answer (the floors).  Needs an MI355X."""
import numpy as np
import pytest

import odd_grids as og
from rmf_crowdsim_amd import (CrowdSimError, LocationHash2D, MonotonicCrowd, NoLocalPlan, Simulation, SourceSink,
                              StubHighLevelPlan, Zanlungo, _abi, scenes)
from rmf_crowdsim_amd.tiles import LocalTileMesh
from select_reference import count, pred, select, selection
from test_oracle_reference_kats import MockEventListener

pytestmark = pytest.mark.gpu
CS_CFG_FORCE_TILED = _abi.CS_CFG_FORCE_TILED
# The 20 further steps of a test are 0.025 s long.  The lattice scenes are made for the ten steps of 0.1 s they are asked
# after: the slower files drift towards their neighbours, and 2.1 s into the scene (step 22 of 0.1 s, in the f64 oracle as
# well) two walkers meet inside the model's collision distance, the force throws one out of the grid and the step fails with
# "Index out of bounds".  Eleven steps of 0.1 s and twenty of 0.025 s end at 1.6 s.
DT_ON = 0.025


def _release(tiles, single):
    return og.released(single, *[e for mesh in tiles for e in mesh.engines])


# ---- a. every read on every tile --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", og.GHOST_CASES, ids=og.GHOST_IDS)
def test_a_tile_that_holds_ghosts_answers_every_read_for_the_agents_it_owns(case, monkeypatch):
    sc, (mesh,), single, rec, rects, held, handle_of = og.ghost_state(case)
    with _release([mesh], single):
        halo = case[2]
        for k, (engine, (own, ghosts)) in enumerate(zip(mesh.engines, held)):
            elsewhere = rec[~np.isin(rec["id"], np.concatenate([own["id"], ghosts["id"]]))]
            asked = og.ask_tile_with_ghosts(engine, sc, rects[k], own, ghosts, elsewhere, halo,
                                            f"{og.GHOST_IDS[og.GHOST_CASES.index(case)]}, tile {k}", monkeypatch, handle_of)
            print(f"tile {k}: {len(asked)} floors met, no call left out")
        # the mesh's own merged reads in this state: nobody twice
        assert len(mesh) == len(rec) and mesh.read_agents().tobytes() == rec.tobytes()
        # spatial queries: discs round agents all over the crowd and on the cuts themselves, beside the agents nearest to
        # them; merged over the tiles they are the single engine's lists
        cut_rows, cut_cols = og.cuts_of(rects)
        ox, oy = sc.grid["offset"]
        pts = [(float(a["x"]), float(a["y"])) for a in rec[np.linspace(0, len(rec) - 1, 40).astype(np.int64)]]
        row, col = sc.cells_of(rec)
        for c in cut_rows:
            pts += [(ox + c * sc.cell, float(a["y"])) for a in rec[np.argsort(np.abs(row - c), kind="stable")[:6]]]
        for c in cut_cols:
            pts += [(float(a["x"]), oy + c * sc.cell) for a in rec[np.argsort(np.abs(col - c), kind="stable")[:6]]]
        radii = [halo * sc.cell * (0.5 + (j % 3)) for j in range(len(pts))]
        want = single.query_radius_batch(radii, pts)
        got = mesh.get_neighbours_in_radius_batch(radii, pts)
        owner_of = dict(zip(rec["id"].tolist(), og.owners(rects, sc, rec).tolist()))
        across = sum(1 for w in want if len({owner_of[i] for i in w}) > 1)
        print(f"{len(pts)} discs list {sum(len(w) for w in want)} agents; {across} discs list agents of more than one tile")
        assert across >= 5 and sum(len(w) for w in want) > 100
        assert got == want
        assert all(len(set(g)) == len(g) for g in got)  # (a ghost listed beside its owner's copy would be there twice)
        assert mesh.get_nearest_neighbours_batch(7, pts) == single.query_knn_batch(7, pts)


# ---- b. asking changes nothing ----------------------------------------------------------------------------------------------
def _ask_a_little(engine, sc, own, ghosts, rect, halo):
    """one call of every family on a tile that holds ghosts (each may sort the arrays, ghosts included); what they answer is
    compared in test a"""
    both = og._join(own, ghosts)
    assert len(engine) == len(engine.read_agents()) == len(own)
    engine.count_agents([dict(speed=(0.0, 0.3))])
    engine.agent_field((float(both["x"].min()), float(both["y"].min())), sc.cell, (16, 16), velocity=True)
    engine.close_pairs(halo * sc.cell)
    engine.agent_clusters(halo * sc.cell)
    engine.agent_neighbours(halo * sc.cell)
    engine.encounters(0.5, 3.0, halo * sc.cell)
    rays = og.ghost_rays(sc, rect, own, ghosts, halo)
    engine.cast_rays(np.column_stack([rays["ox"], rays["oy"]]), np.column_stack([rays["ux"], rays["uy"]]), 0.2,
                     t_max=rays["t_max"], ignore=rays["ignore"])
    engine.leg_conflicts(og.ghost_legs(sc, rect, own, ghosts, halo), 0.4 * sc.cell, 2.0)
    engine.leg_intervals(og.ghost_legs(sc, rect, own, ghosts, halo, intervals=True), 0.4 * sc.cell, 2.0)
    engine.read_agents_by_id(both["id"][::7], missing_ok=True)
    engine.query_radius_batch([sc.cell] * 4, [(float(a["x"]), float(a["y"])) for a in both[:4]], details=True)


@pytest.mark.parametrize("case,flags", [(og.GHOST_CASES[0], 0), (og.GHOST_CASES[1], CS_CFG_FORCE_TILED), (og.GHOST_CASES[3], 0)],
                         ids=["2x2-halo1-phases1", "2x2-halo2-phases2-tiled", "3x1-halo2-phases1"])
def test_asking_a_tile_that_holds_ghosts_changes_nothing(case, flags):
    """Two meshes make the same exchange; one is asked a call of every family on every tile, the other nothing; both take
    the rest of the step and 20 more: the asking mesh, the quiet mesh and the single engine hold the same bytes."""
    sc, (asking, quiet), single, rec, rects, held, _ = og.ghost_state(case, meshes=2, flags=flags)
    with _release([asking, quiet], single):
        for k, (engine, (own, ghosts)) in enumerate(zip(asking.engines, held)):
            _ask_a_little(engine, sc, own, ghosts, rects[k], case[2])
        for mesh in (asking, quiet):
            og.finish_step(mesh)
        single.step(og.DT, report=False)
        assert asking.read_agents().tobytes() == quiet.read_agents().tobytes() == single.read_agents().tobytes()
        for _ in range(20):
            for t in (asking, quiet, single):
                t.step(DT_ON)
        end = single.read_agents()
        assert np.isfinite(end["x"]).all() and end.tobytes() != rec.tobytes()
        assert asking.read_agents().tobytes() == quiet.read_agents().tobytes() == end.tobytes()


def _step_in_parts(mesh, dt, ask=None):
    """LocalTileMesh.step with the host-side spawn path, in its parts, `ask(engine)` between the spawn commit and the step"""
    mesh._exchange_all()
    flags = None
    for e in mesh.engines:
        f = e.spawn_probe(dt)
        flags = f if flags is None else (flags | f)
    for e in mesh.engines:
        e.spawn_commit(flags)
    if ask is not None:
        for k, e in enumerate(mesh.engines):
            ask(k, e)
    for e in mesh.engines:
        e.step(dt, report=True)
    return [e.last_report for e in mesh.engines]


def test_asking_route_followers_on_tiles_that_hold_ghosts_changes_nothing():
    """The lanes of route followers of test_gpu_tiles.py on a (3, 1) mesh (the route word travels in the ghost record), with
    a listener: 300 steps bring walkers to both cuts; then for 40 steps every tile of one mesh is asked between the unpack
    and the step, every other step.  Agents, events and reports are those of a mesh that is never asked, the agents and
    events those of the single engine."""
    from test_gpu_tiles import _route_scene
    grid = dict(width=160.0, height=160.0, cell_size=2.0, offset=(0.0, 0.0))
    twins = [LocalTileMesh(LocationHash2D(**grid), (3, 1), halo_cells=1), LocalTileMesh(LocationHash2D(**grid), (3, 1), halo_cells=1),
             Simulation(LocationHash2D(**grid))]
    asking, quiet, single = twins
    ears = []
    for t in twins:
        _route_scene(t, NoLocalPlan())
        ears.append(MockEventListener())
        t.add_event_listener(ears[-1])
    with _release([asking, quiet], single):
        for _ in range(300):
            for t in twins:
                t.step(0.1)
        rec = single.read_agents()
        assert asking.read_agents().tobytes() == quiet.read_agents().tobytes() == rec.tobytes()
        cuts = og.cuts_of(og.mesh_rects(asking))[0]
        row = np.floor(rec["x"] / 2.0).astype(np.int64)
        near = [int((np.abs(row - c) <= 1).sum()) for c in cuts]
        print(f"{len(rec)} route followers after 300 steps, {near} within a cell of the cuts at rows {cuts}")
        assert len(rec) > 100 and len(cuts) == 2 and min(near) >= 3
        legs = og.legs_ref.legs_array(np.column_stack([rec["x"][::9] + 0.2, rec["y"][::9]]), (0.0, 0.0), 0.0, 2.0)

        def ask(k, e):
            n = len(e)
            assert len(e.read_agents()) == n == len(e.select_agents())
            e.close_pairs(2.0)
            e.agent_clusters(2.0)
            e.agent_neighbours(2.0)
            e.encounters(0.5, 3.0, 2.0)
            e.cast_rays([(10.0, 10.0 + 7.5 * j) for j in range(16)], [(1.0, 0.02)] * 16, 0.3)
            e.leg_conflicts(legs, 0.5, 2.0)
            e.leg_intervals(legs, 0.5, 2.0)
            e.agent_field((0.0, 0.0), 4.0, (40, 40), velocity=True)

        for step in range(40):
            a = _step_in_parts(asking, 0.1, ask if step % 2 == 0 else None)
            q = _step_in_parts(quiet, 0.1)
            single.step(0.1)
            assert a == q, step
        end = single.read_agents()
        assert asking.read_agents().tobytes() == quiet.read_agents().tobytes() == end.tobytes()
        assert set(end["id"].tolist()) != set(rec["id"].tolist())  # (agents came and went meanwhile)
        assert ears[0].added == ears[1].added and sorted(ears[0].added) == sorted(ears[2].added)
        assert len(ears[2].added) >= len(end) > len(rec)
        assert ears[0].removed == ears[1].removed and sorted(ears[0].removed) == sorted(ears[2].removed)


# ---- c. by-id writes and removals with ids of ghosts -------------------------------------------------------------------------
def test_writes_and_removals_by_id_treat_a_ghost_as_nobody():
    """write_agents, remove_agents_by_id and set_targets given ids of ghosts of the tile refuse the batch ("unknown agent
    id", all or nothing) and leave every record of the tile as it was; remove_agents of a ghost's id finds nobody;
    remove_selected by a region over the ring removes owned agents only.  The test ends there: the neighbours' copies of
    removed agents are stale."""
    sc, (mesh,), single, rec, rects, held, _ = og.ghost_state(og.GHOST_CASES[0])
    with _release([mesh], single):
        for k, (engine, (own, ghosts)) in enumerate(zip(mesh.engines, held)):
            some = np.concatenate([own[:5], ghosts[:5]])
            moved = some.copy()
            moved["vx"] = 0.25
            goals = np.column_stack([some["x"], some["y"] + 5.0])
            for what, call in (("write_agents", lambda: engine.write_agents(moved, fields=("velocity",))),
                               ("write_agents, one ghost", lambda: engine.write_agents(moved[5:6], fields=("velocity",))),
                               ("remove_agents_by_id", lambda: engine.remove_agents_by_id(some["id"])),
                               ("remove_agents_by_id, one ghost", lambda: engine.remove_agents_by_id(some["id"][7:8])),
                               ("set_targets", lambda: engine.set_targets(some["id"], goals)),
                               ("remove_agents", lambda: engine.remove_agents(int(ghosts["id"][0])))):
                with pytest.raises(CrowdSimError, match="unknown agent id"):
                    call()
                assert len(engine) == len(own) and engine.read_agents().tobytes() == own.tobytes(), (k, what)
            assert engine.remove_agent_here(int(ghosts["id"][1])) is False
            out, found = engine.read_agents_by_id(some["id"], missing_ok=True)
            assert np.asarray(found, dtype=bool).tolist() == [True] * 5 + [False] * 5 and out[:5].tobytes() == own[:5].tobytes()
            # the same write without the ghosts is taken: the refusals were the ghosts'
            engine.write_agents(moved[:5], fields=("velocity",))
            want = own.copy()
            want["vx"][np.isin(want["id"], moved["id"][:5])] = 0.25
            assert engine.read_agents().tobytes() == want.tobytes(), k
        # remove_selected: a box over a tile's ring and the owned cells next to it
        for k, (engine, (own, ghosts)) in enumerate(zip(mesh.engines, held)):
            g = ghosts[len(ghosts) // 2]
            box = (float(g["x"]) - 3 * sc.cell, float(g["y"]) - 3 * sc.cell, float(g["x"]) + 3 * sc.cell, float(g["y"]) + 3 * sc.cell)
            sel = selection(_abi.CS_SEL_RECT, x0=box[0], y0=box[1], x1=box[2], y1=box[3])
            mine, theirs = pred(sel, own, None, None, None), pred(sel, ghosts, None, None, None)
            print(f"tile {k}: the box holds {int(mine.sum())} owned agents and {int(theirs.sum())} ghosts")
            assert mine.sum() >= 3 and theirs.sum() >= 3
            n, ids = select(engine, sel, cap=len(own))
            assert n == mine.sum() and ids.tolist() == own["id"][mine].tolist()
            gone = engine.remove_selected(rect=box)
            assert gone.tolist() == own["id"][mine].tolist()
            assert len(engine) == len(own) - int(mine.sum()) and engine.read_agents()["id"].tolist() == own["id"][~mine].tolist()
            rc, counts = count(engine, [sel])
            assert rc == 0 and counts.tolist() == [0]


def test_removing_an_agent_whose_ghost_sits_in_a_lower_tile_takes_it_from_its_owner():
    """LocalTileMesh.remove_agents asks the tiles in order and stops at the first that says "here".  With the ghosts
    unpacked tile 0 holds a copy of an agent that a later tile owns: the owner must lose it, and tile 0 nobody."""
    sc, (mesh,), single, rec, rects, held, _ = og.ghost_state(og.GHOST_CASES[0])
    with _release([mesh], single):
        owner_of = dict(zip(rec["id"].tolist(), og.owners(rects, sc, rec).tolist()))
        ghost = int(held[0][1]["id"][3])
        owner = owner_of[ghost]
        assert owner > 0
        mesh.remove_agents(ghost)
        assert [len(e) for e in mesh.engines] == [len(own) - (k == owner) for k, (own, _) in enumerate(held)]
        assert len(mesh) == len(rec) - 1
        assert mesh.read_agents().tobytes() == rec[rec["id"] != ghost].tobytes()
        with pytest.raises(CrowdSimError, match="unknown agent id"):
            mesh.remove_agents(ghost)  # (tile 0 still holds the stale copy: it is nobody's)


# ---- d. a re-cut with ghosts present -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("phases", [1, 2])
def test_a_recut_of_tiles_that_hold_ghosts(phases):
    """k_tile_histogram and k_tile_export with owned_only set, and tile_retile, which drops the ghosts: the new rectangles
    are TileLayout's of numpy histograms of the single engine's records, every tile holds the agents it owns, and 20
    further steps give the single engine's bytes."""
    sc = og.scene("lopsided")
    weights = og.placed_cut_weights(sc, (2, 2), og.RECUT_FROM[0], og.RECUT_FROM[1], 1)
    (mesh,), single, _ = og.ghost_twins(sc, (2, 2), 1, weights, phases)
    with _release([mesh], single):
        rec = single.read_agents()
        before = og.mesh_rects(mesh)
        cut, n_after = og.ghost_recut_floors(sc, rec, before)
        og.unpack_ghosts(mesh)
        counts = mesh.recut()
        assert og.mesh_rects(mesh).tolist() == cut.tolist() != before.tolist()
        assert counts.ravel().tolist() == n_after.tolist() == mesh.tile_counts().ravel().tolist()
        assert mesh.read_agents().tobytes() == rec.tobytes()
        for _ in range(20):
            for t in (mesh, single):
                t.step(DT_ON)
        end = single.read_agents()
        assert np.isfinite(end["x"]).all() and mesh.read_agents().tobytes() == end.tobytes()


# ---- e. ghosts made by a spawn -----------------------------------------------------------------------------------------------
def test_a_ghost_made_by_a_spawn_is_nobody_to_the_tile_across_the_cut():
    """The scene of test_an_agent_spawned_next_to_a_cut_is_seen_across_it_at_once: each source stands 0.1 m from the cut
    at x = 20 m, and the tile on the other side has it in its ring.  After the exchange and the host-side spawn_probe /
    spawn_commit that tile holds a ghost that no exchange brought.  Select, count, the raster and read_agents answer for the
    agents the tile owns: those of the single engine's state before the step on its side of the cut, and the agent just
    spawned at its own source."""
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    lp = Zanlungo(*scenes.METRIC_ZANLUNGO)
    watchers = np.array([(19.6, 10.0), (19.5, 10.7), (19.7, 9.4), (20.4, 30.3), (20.2, 29.5)])
    sources = ((20.1, 10.0), (19.9, 30.0))  # (owned by the upper tile, by the lower tile)
    single = Simulation(LocationHash2D(**grid))
    mesh = LocalTileMesh(LocationHash2D(**grid), (2, 1), halo_cells=1)
    for t in (single, mesh):
        t.add_agents(watchers[:3], StubHighLevelPlan((0.05, 0.0)), lp, 2.0)
        t.add_agents(watchers[3:], StubHighLevelPlan((-0.05, 0.0)), lp, 2.0)
        t.add_source_sink(SourceSink(sources[0], 1.0, MonotonicCrowd(20.0), StubHighLevelPlan((1.0, 0.0)), NoLocalPlan(),
                                     [(35.0, 10.0)], False, 2.0))
        t.add_source_sink(SourceSink(sources[1], 1.0, MonotonicCrowd(20.0), StubHighLevelPlan((-1.0, 0.0)), NoLocalPlan(),
                                     [(5.0, 30.0)], False, 2.0))
    with _release([mesh], single):
        everyone = selection(0)
        ring = selection(_abi.CS_SEL_RECT, x0=18.0, y0=0.0, x1=22.0, y1=40.0)  # (the cells either side of the cut)
        d = og.field_ref.desc(18.0, 0.0, 2.0, 2.0, 2, 20)
        spawned_ghosts = 0
        for step in range(12):
            before = single.read_agents()
            single.step(0.05)
            after = single.read_agents()
            new = after[~np.isin(after["id"], before["id"])]
            born = {int(a["id"]): sources[0] if a["y"] < 20.0 else sources[1] for a in new}

            def ask(k, e):
                nonlocal spawned_ghosts
                mine = lambda x: (x < 20.0) == (k == 0)  # noqa: E731
                want = sorted(before["id"][mine(before["x"])].tolist() + [i for i, s in born.items() if mine(s[0])])
                assert len(e) == len(want), (step, k)
                # the tile's own list: the single engine's rows for the agents that were there, the newborn at its source
                own = e.read_agents()
                assert own["id"].tolist() == want, (step, k)
                old = np.isin(own["id"], before["id"])
                assert own[old].tobytes() == before[np.isin(before["id"], own["id"])].tobytes(), (step, k)
                for a in own[~old]:
                    assert abs(a["x"] - born[int(a["id"])][0]) < 1e-6 and abs(a["y"] - born[int(a["id"])][1]) < 1e-6
                # every answer is the restatement's on that list
                for sel in (everyone, ring):
                    n, ids = select(e, sel, cap=64)
                    assert n == len(ids) and ids.tolist() == own["id"][pred(sel, own, None, None, None)].tolist(), (step, k)
                rc, counts = count(e, [everyone, ring])
                assert rc == 0 and counts.tolist() == [len(own), int(pred(ring, own, None, None, None).sum())], (step, k)
                rc, cnt, sums = og.field_ref.field(e, d, None, want="both")
                assert rc == 0, (step, k)
                og.field_ref.check(f"step {step}, tile {k}", cnt, sums, og.field_ref.raster(d, own))
                # the ghost the spawn made stands exactly on the other tile's source, where no exchanged ghost stands: a
                # circle of 3 cm round that source is empty, the one round the tile's own source lists the newborn
                for i, s in born.items():
                    here = selection(_abi.CS_SEL_CIRCLE, cx=s[0], cy=s[1], r=0.03)
                    assert not pred(here, before, None, None, None).any()  # (nobody else stands there: by the restatement)
                    n, ids = select(e, here, cap=8)
                    assert ids.tolist() == ([i] if mine(s[0]) else []) and n == len(ids), (step, k, i)
                    rc, cnt, _ = og.field_ref.field(e, og.field_ref.desc(s[0] - 0.03, s[1] - 0.03, 0.06, 0.06, 1, 1), None, want="count")
                    assert rc == 0 and int(cnt.sum()) == (1 if mine(s[0]) else 0), (step, k, i)
                    spawned_ghosts += not mine(s[0])

            _step_in_parts(mesh, 0.05, ask)
            assert mesh.read_agents().tobytes() == after.tobytes(), step
        print(f"{spawned_ghosts} ghosts were made by a spawn")
        assert spawned_ghosts >= 2
