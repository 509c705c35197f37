"""The flow-field planner on a tile mesh (cs_mesh_register_hlp_field; FieldPlanner through NativeTileMesh): every tile holds
the whole field, and an in-process mesh (2 x 2 and 3 x 1 tiles) whose crowd crosses the cuts, with a source-sink next to
one, steps to the single engine's bytes for both samplings: with reports and without, after a re-cut, after an update;
every tile launches the field kernel once per step and no Python planner is ever asked.  One case runs under
CS_CFG_TILE_OVERLAP."""
import numpy as np
import pytest

from rmf_crowdsim_amd import (FieldPlanner, LocationHash2D, MonotonicCrowd, Simulation, SourceSink, StubHighLevelPlan, _abi)
from rmf_crowdsim_amd.tiles import NativeTileMesh
from test_gpu_hlp_field import GRIDS, LP, crowd, swirl

pytestmark = pytest.mark.gpu

DT = 0.1
DRIFT = np.array([0.5, 0.35], dtype=np.float32)  # m/s on top of the swirl: the whole crowd drifts across the cuts


def _planners(corner, sampling, asked):
    """Two rasters that cover the crowd's window and a metre round it, 7 x 5 coarse bins and 64 x 64 fine ones, without
    holes (an agent that stands still, None, in a crowd that drifts at 0.6 m/s is walked into: the model's forces throw
    both off the grid); the walls and the agents outside a raster are the single engine's tests"""
    low = (corner[0] - 1.0, corner[1] - 1.0)
    small = FieldPlanner(low, (26.0 / 7.0, 26.0 / 5.0), np.float32(0.4) * swirl(5, 7) + DRIFT, sampling)
    large = FieldPlanner(low, 26.0 / 64.0, np.float32(0.4) * swirl(64, 64, -1.0) + DRIFT, sampling)
    for p in (small, large):
        p.get_desired_velocity = lambda agent, time, rule=p.get_desired_velocity: (asked.append(1), rule(agent, time))[1]
    uniform = np.zeros((8, 8, 2), dtype=np.float32)
    uniform[...] = (1.0, 0.2)
    return small, large, FieldPlanner((0.0, 0.0), 4.0, uniform, sampling)


def _scene(t, pts, small, large, lane):
    t.add_agents(pts[0::3], small, LP, 1.0)
    t.add_agents(pts[1::3], large, LP, 1.0)
    t.add_agents(pts[2::3], StubHighLevelPlan((float(DRIFT[0]), float(DRIFT[1]))), LP, 1.0)
    # a source 0.6 m before the cut of the 2 x 2 mesh at x = 16, in the free strip beside the crowd's window (y < 4): its
    # agents walk at (1.0, 0.2) m/s, a field over the whole grid, across the cut and through both waypoints
    t.add_source_sink(SourceSink((15.4, 2.0), 0.3, MonotonicCrowd(10.0), lane, LP, [(16.2, 2.16), (17.6, 2.44)], False, 1.0))


def _same(mesh, single, what):
    a, b = mesh.read_agents(), single.read_agents()
    assert a.tobytes() == b.tobytes(), what
    return b


@pytest.mark.parametrize("shape,flags,sampling", [((2, 2), 0, "nearest"), ((2, 2), 0, "bilinear"), ((3, 1), 0, "nearest"),
                                                  ((3, 1), 0, "bilinear"),
                                                  ((2, 2), _abi.CS_CFG_TILE_OVERLAP | _abi.CS_CFG_FORCE_TILED, "bilinear")],
                         ids=["2x2-nearest", "2x2-bilinear", "3x1-nearest", "3x1-bilinear", "2x2-overlap"])
def test_a_mesh_with_field_planners_steps_as_one_engine(shape, flags, sampling):
    grid, corner, _ = GRIDS["plain"]
    asked = []
    pts = crowd(corner)
    small, large, lane = _planners(corner, sampling, asked)
    mesh = NativeTileMesh(LocationHash2D(**grid), shape, 1, flags=flags)
    single = Simulation(LocationHash2D(**grid), flags=flags & _abi.CS_CFG_FORCE_TILED)
    try:
        for t in (mesh, single):
            _scene(t, pts, small, large, lane)
        first = _same(mesh, single, "before the first step")
        n_tiles = shape[0] * shape[1]
        steps = 0
        for step in range(12):  # with a report: compared after every step
            for t in (mesh, single):
                t.step(DT)
            now = _same(mesh, single, (shape, sampling, step))
            for key in ("n_agents", "n_spawned", "n_destroyed", "n_waypoint_hits"):
                assert mesh.last_report[key] == single.last_report[key], (step, key)
            steps += 1
        # the crowd crossed the cuts, and the sink's agents did
        rects = mesh.tile_rects()
        cuts = {"x": sorted(set(int(r[0]) for r in rects) - {0}), "y": sorted(set(int(r[2]) for r in rects) - {0})}
        at = {int(i): k for k, i in enumerate(now["id"])}
        old = first[np.isin(first["id"], now["id"])]
        new = now[[at[int(i)] for i in old["id"]]]
        crossed = sum(int(((old[axis] < c) != (new[axis] < c)).sum()) for axis in cuts for c in cuts[axis])  # (cells of 1 m)
        spawned = now[now["id"] >= len(pts)]
        print(f"{shape}, {sampling}: cuts at {cuts}, {crossed} agents crossed one, {len(spawned)} spawned")
        assert crossed >= 8 and len(spawned) >= 2
        assert shape != (2, 2) or (spawned["x"] > 16.0).any()
        for _ in range(6):  # without a report: nothing waits, nothing goes through the host
            for t in (mesh, single):
                t.step(DT, report=False)
            steps += 1
        _same(mesh, single, "six steps without a report")
        mesh.recut()
        for step in range(3):
            for t in (mesh, single):
                t.step(DT)
            _same(mesh, single, ("after the re-cut", step))
            steps += 1
        for p in (small, large):  # reaches the engine and every tile of the mesh
            p.update(p.vectors * np.float32(0.875))  # (everybody a little slower: nobody is walked into)
        for step in range(3):
            for t in (mesh, single):
                t.step(DT, report=bool(step % 2))
            last = _same(mesh, single, ("after the update", step))
            steps += 1
        assert (np.hypot(last["vx"], last["vy"]) > 0.0).sum() > 600
        launches = [mesh.tile(k).kernel_stat(_abi.CS_STAT_HLP_FIELD_LAUNCHES) for k in range(n_tiles)]
        assert launches == [steps] * n_tiles and single.kernel_stat(_abi.CS_STAT_HLP_FIELD_LAUNCHES) == steps
        assert not asked  # (no Python planner was asked: neither the engine nor the mesh stepped through the host)
    finally:
        single.close()
        mesh.__del__()
