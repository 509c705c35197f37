"""Solving a flow field on the device (include/crowdstep_state.h, cs_flow_field_solve; Simulation.solve_flow_field,
FieldPlanner.solve) on one engine.  The distances, the vectors and `reached` are compared with the sweeps of
tests/flow_solve_reference.py as BYTES: the smallest rasters a tiled solver can get wrong (one bin, one row, one column,
just under, exactly and just over the 32-bin tiles), random walls, a serpentine maze whose path crosses the tile borders
dozens of times, a spiral; three bin shapes; slowness rasters; the crowd's density with and without a filter and with an
agent the index never took; a planner solved on the device against one updated from the host; the refusals."""
import ctypes as C

import numpy as np
import pytest

import flow_solve_reference as ref
from rmf_crowdsim_amd import (CrowdSimError, FieldPlanner, LocationHash2D, Selection, Simulation, StubHighLevelPlan,
                              Zanlungo, _abi, flow_field_to_goals, scenes)

pytestmark = pytest.mark.gpu

GRID = dict(width=32.0, height=32.0, cell_size=1.0, offset=(0.0, 0.0))
LP = Zanlungo(*scenes.METRIC_ZANLUNGO)
CELLS = [(0.5, 0.5), (0.5, 0.25), (0.4, 0.4)]
SPEED = 1.3
WALK, DT = 0.1, 0.05  # m/s and s where a crowd follows a solved field: nobody closes the lattice gap in a test's steps
NO_PLANNER = 0xFFFFFFFF


@pytest.fixture(scope="module")
def empty():
    sim = Simulation(LocationHash2D(**GRID))
    yield sim
    sim.close()


def agree(sim, blocked, goals, cell, *, origin=(0.0, 0.0), counts=None, vectors=True, old=False, **how):
    """the device's solve equals the restatement's, byte for byte -> (dist, stats)"""
    want_vec, want_dist, reached, sweeps = ref.solve(blocked, goals, cell, SPEED, slowness=how.get("slowness"), counts=counts,
                                                     density_weight=how.get("density_weight", 0.0))
    vec, dist, stats = sim.solve_flow_field(origin, cell, goals, SPEED, blocked=blocked, distance=True, **how)
    print(f"{goals.shape[1]} x {goals.shape[0]}, cell {cell}: reached {stats['reached']} of {goals.size}, "
          f"{stats['rounds']} rounds on the device, {sweeps} sweeps in numpy")
    assert dist.dtype == np.float64 and dist.tobytes() == want_dist.tobytes()
    assert stats["reached"] == reached and 1 <= stats["rounds"] <= goals.size + 1
    if vectors:
        assert vec.dtype == np.float32 and vec.tobytes() == want_vec.tobytes()
    if old:  # where numpy's hypot is sqrt(w * w + h * h): the distances of flow_field_to_goals
        assert float(np.hypot(*cell)) == float(np.sqrt(np.float64(cell[0]) * cell[0] + np.float64(cell[1]) * cell[1]))
        assert flow_field_to_goals(blocked, goals, origin, cell, SPEED, return_distance=True)[1].tobytes() == dist.tobytes()
    return dist, stats


@pytest.mark.parametrize("cell", CELLS, ids=str)
@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 37), (37, 1), (31, 33), (64, 64), (65, 63), (130, 3)])
def test_small_and_tile_edge_rasters(empty, nx, ny, cell):
    blocked, goals = ref.random_walls(ny, nx, 100 * nx + ny, 0.25, [(0, 0), (nx - 1, ny - 1), (nx // 2, ny // 3)])
    dist, _ = agree(empty, blocked, goals, cell, old=cell != CELLS[2])
    assert dist[0, 0] == 0.0
    # without walls, and with every bin a goal
    agree(empty, None, goals, cell)
    _, stats = agree(empty, blocked, np.ones((ny, nx), dtype=bool), cell)
    assert stats["reached"] == int((~blocked).sum())


@pytest.mark.parametrize("cell", CELLS, ids=str)
def test_random_walls_with_two_goals(empty, cell):
    blocked, goals = ref.issue_case()
    _, stats = agree(empty, blocked, goals, cell, origin=(-3.0, 7.5), old=cell != CELLS[2])
    assert stats["reached"] == 2088 and int((~blocked).sum()) == 2192


@pytest.mark.parametrize("cell", CELLS, ids=str)
def test_a_serpentine_maze_takes_many_rounds(empty, cell):
    blocked, goals = ref.serpentine(40, 96, 4)
    dist, stats = agree(empty, blocked, goals, cell, old=cell != CELLS[2])
    assert stats["reached"] == int((~blocked).sum())
    # the path runs the raster's height once per corridor: far longer than the straight line, and it crosses the tiles'
    # borders again and again, so the solve needs more rounds than there are tiles along the raster
    assert dist.max() > 20 * 39 * cell[1]
    assert 96 // 32 < stats["rounds"] < 96 * 40 + 1


def test_a_spiral(empty):
    blocked, goals = ref.spiral(67)
    assert 2000 < int((~blocked).sum()) < 2400  # (a corridor of half the raster's bins)
    for cell in CELLS[:2]:
        _, stats = agree(empty, blocked, goals, cell, old=True)
        assert stats["reached"] == int((~blocked).sum())
    # no goal: nothing is reached, in one round
    _, stats = agree(empty, blocked, np.zeros_like(goals), CELLS[0])
    assert stats == {"reached": 0, "rounds": 1}
    # a blocked goal is ignored
    walled = goals.copy()
    walled[0, 1] = True
    both = blocked.copy()
    both[0, 1] = True
    agree(empty, both, walled, CELLS[0])


def test_slowness(empty):
    blocked, goals = ref.issue_case()
    rng = np.random.default_rng(3)
    slow = rng.uniform(0.5, 4.0, blocked.shape).astype(np.float32)
    assert slow.min() >= 0.5 and slow.max() < 4.0
    plain, _ = agree(empty, blocked, goals, CELLS[1])
    heavy, _ = agree(empty, blocked, goals, CELLS[1], slowness=slow)
    assert heavy.tobytes() != plain.tobytes()
    # zeros: steps out of those bins are free; the distances are promised, the vectors may circle
    slow[rng.random(blocked.shape) < 0.3] = 0.0
    agree(empty, blocked, goals, CELLS[1], slowness=slow, vectors=False)
    agree(empty, None, goals, CELLS[0], slowness=np.zeros(blocked.shape, dtype=np.float32), vectors=False)


@pytest.fixture(scope="module")
def crowded():
    """500 agents 0.9 m apart on a grid of 1 m cells, and one more beyond the grid's last row that the index never took (a
    negative coordinate would clamp into row 0); a raster of 0.45 x 0.4 bins from (-2.3, -1.7) that is aligned with neither"""
    sim = Simulation(LocationHash2D(**GRID))
    pts = scenes.jittered_lattice(500, 0.9, (3.0, 3.0), 0.1, 5)
    walkers, others = StubHighLevelPlan((0.1, 0.0)), StubHighLevelPlan((0.0, 0.1))
    sim.add_agents(pts[0::2], walkers, LP, 1.0)
    sim.add_agents(pts[1::2], others, LP, 1.0)
    with pytest.raises(CrowdSimError):  # created, then refused by the index (the pattern of test_gpu_select.py)
        sim.add_agents([(40.0, 5.0)], walkers, LP, 1.0)
    assert len(sim.read_agents()) == 501
    yield sim, walkers
    sim.close()


@pytest.mark.parametrize("filtered", [False, True], ids=["everyone", "filtered"])
def test_density(crowded, filtered):
    sim, walkers = crowded
    origin, cell, shape = (-2.3, -1.7), (0.45, 0.4), (66, 96)
    blocked, goals = ref.random_walls(shape[0], shape[1], 9, 0.1, [(2, 2), (90, 60)])
    sel = Selection(high_level_planner=walkers, rect=(10.0, 0.0, 45.0, 30.0)) if filtered else None
    counts = sim.agent_field(origin, cell, shape, sel)
    assert counts[int((5.0 + 1.7) / 0.4), int((40.0 + 2.3) / 0.45)] == 1  # the agent the index never took
    assert 100 < int(counts.sum()) < 400 if filtered else int(counts.sum()) == 501
    plain, _ = agree(sim, blocked, goals, cell, origin=origin)
    dense, _ = agree(sim, blocked, goals, cell, origin=origin, counts=counts, density_weight=0.25, density_filter=sel)
    assert dense.tobytes() != plain.tobytes()
    slow = np.random.default_rng(4).uniform(0.5, 4.0, shape).astype(np.float32)
    agree(sim, blocked, goals, cell, origin=origin, counts=counts, density_weight=3.0, density_filter=sel, slowness=slow)
    # the agent in limbo alone, behind a wall of weight: the bin it stands in is the only one that changes
    alone = Selection(rect=(39.0, 4.0, 41.0, 6.0))
    one = sim.agent_field(origin, cell, shape, alone)
    assert int(one.sum()) == 1
    agree(sim, blocked, goals, cell, origin=origin, counts=one, density_weight=2.0 ** 32, density_filter=alone)


def _door_scene():
    """64 x 64 bins of 0.5 m over the grid: a wall across the middle with two doors, exits on the right or the left edge"""
    blocked = np.zeros((64, 64), dtype=bool)
    blocked[:, 40] = True
    blocked[14:18, 40] = blocked[44:48, 40] = False
    right, left = np.zeros((64, 64), dtype=bool), np.zeros((64, 64), dtype=bool)
    right[:, 63] = True
    left[:, 0] = True
    return blocked, right, left


def test_a_planner_solved_on_the_device_steps_as_one_updated_from_the_host():
    blocked, right, left = _door_scene()
    origin, cell, speed, dt = (0.0, 0.0), 0.5, WALK, DT
    pts = scenes.jittered_lattice(400, 0.8, (2.0, 8.0), 0.1, 2)
    zeros = np.zeros((64, 64, 2), dtype=np.float32)
    a, b = Simulation(LocationHash2D(**GRID)), Simulation(LocationHash2D(**GRID))
    pa, pb = FieldPlanner(origin, cell, zeros), FieldPlanner(origin, cell, zeros)
    try:
        a.add_agents(pts, pa, LP, 1.0)
        b.add_agents(pts, pb, LP, 1.0)
        launches = 0
        for k in range(10):
            if k % 3 == 0:
                # A: solved on the device, straight into the planner's samples, nothing downloaded
                vec, dist, stats = pa.solve(right, speed, blocked=blocked, density_weight=0.25, vectors=False)
                assert vec is None and dist is None and stats["reached"] == int((~blocked).sum())
                # B: the counts down, the restatement on the host, the vectors up
                counts = b.agent_field(origin, cell, (64, 64))
                pb.update(ref.solve(blocked, right, (cell, cell), speed, counts=counts, density_weight=0.25)[0])
            a.step(dt, report=False)
            b.step(dt)
            launches += 1
        end = a.read_agents()
        assert end.tobytes() == b.read_agents().tobytes()
        assert end["vx"].mean() > 0.0  # (towards the exits on the right)
        # a solve queued right behind three unwaited steps must not change them ...
        for _ in range(3):
            a.step(dt, report=False)
            b.step(dt)
        _, _, stats = pa.solve(left, speed, blocked=blocked, vectors=False)
        assert stats["reached"] == int((~blocked).sum())
        middle = a.read_agents()
        assert middle.tobytes() == b.read_agents().tobytes() and middle["vx"].mean() > 0.0
        # ... and must change the next ones
        pb.update(ref.solve(blocked, left, (cell, cell), speed)[0])
        for _ in range(4):
            a.step(dt, report=False)
            b.step(dt)
        last = a.read_agents()
        assert last.tobytes() == b.read_agents().tobytes() and last["vx"].mean() < middle["vx"].mean()
        assert a.kernel_stat(_abi.CS_STAT_HLP_FIELD_LAUNCHES) == launches + 7
        # with the vectors asked for, the host's copy follows the device's
        vec, _, _ = pa.solve(right, speed, blocked=blocked)
        assert pa.vectors.tobytes() == vec.tobytes() == ref.solve(blocked, right, (cell, cell), speed)[0].tobytes()
        assert a.device_bytes > b.device_bytes  # (the solve's scratch is counted)
    finally:
        a.close()
        b.close()


def _raw(sim, goals, *, hlp=NO_PLANNER, blocked=None, slowness=None, speed=1.0, weight=0.0, sel=None, raster=None,
         null_desc=False, null_goals=False, outputs=True):
    """cs_flow_field_solve as a C host calls it -> (rc, the reason)"""
    ny, nx = goals.shape
    desc = _abi.FlowDesc()
    desc.raster = _abi.FieldDesc(0.0, 0.0, 0.5, 0.5, nx, ny) if raster is None else raster
    g = np.ascontiguousarray(goals, dtype=np.uint8)
    desc.goals = None if null_goals else g.ctypes.data_as(C.POINTER(C.c_uint8))
    if blocked is not None:
        bl = np.ascontiguousarray(blocked, dtype=np.uint8)
        desc.blocked = bl.ctypes.data_as(C.POINTER(C.c_uint8))
    if slowness is not None:
        sl = np.ascontiguousarray(slowness, dtype=np.float32)
        desc.slowness = sl.ctypes.data_as(C.POINTER(C.c_float))
    desc.speed, desc.density_weight = speed, weight
    if sel is not None:
        desc.density_filter = C.pointer(sel)
    dist = np.full((ny, nx), -7.0)
    stats = _abi.FlowStats(11, 12, 13)
    rc = sim._lib.cs_flow_field_solve(sim._engine, None if null_desc else C.byref(desc), hlp, None,
                                      dist.ctypes.data_as(C.POINTER(C.c_double)) if outputs else None, C.byref(stats))
    if rc != 0:  # nothing was written
        assert (dist == -7.0).all() and (stats.reached, stats.rounds, stats.reserved) == (11, 12, 13)
    return rc, sim._lib.cs_last_error(sim._engine).decode()


def test_refusals_change_nothing():
    blocked, right, left = _door_scene()
    pts = scenes.jittered_lattice(200, 0.8, (2.0, 8.0), 0.1, 2)
    zeros = np.zeros((64, 64, 2), dtype=np.float32)
    a, b = Simulation(LocationHash2D(**GRID)), Simulation(LocationHash2D(**GRID))
    pa, pb = FieldPlanner((0.0, 0.0), 0.5, zeros), FieldPlanner((0.0, 0.0), 0.5, zeros)
    other_a, other_b = FieldPlanner((1.0, 0.0), 0.5, zeros), FieldPlanner((1.0, 0.0), 0.5, zeros)
    const = StubHighLevelPlan((0.1, 0.0))
    try:
        for sim, p, o in ((a, pa, other_a), (b, pb, other_b)):
            sim.add_agents(pts[0::2], p, LP, 1.0)
            sim.add_agents(pts[1::4], o, LP, 1.0)
            sim.add_agents(pts[3::4], const, LP, 1.0)
            p.solve(right, WALK, blocked=blocked, vectors=False)
            sim.step(DT)
        h = a._planner_handles
        slow = np.ones((64, 64), dtype=np.float32)

        def bad(value):
            s = slow.copy()
            s[17, 5] = value
            return s
        unknown = _abi.Selection()
        unknown.terms = 1 << 30
        nan_rect = Selection(rect=(0.0, 0.0, float("nan"), 1.0)).struct()
        refused = {
            "null desc": dict(null_desc=True), "null goals": dict(null_goals=True),
            "cell_w 0": dict(raster=_abi.FieldDesc(0.0, 0.0, 0.0, 0.5, 64, 64)),
            "cell_h inf": dict(raster=_abi.FieldDesc(0.0, 0.0, 0.5, float("inf"), 64, 64)),
            "x0 nan": dict(raster=_abi.FieldDesc(float("nan"), 0.0, 0.5, 0.5, 64, 64)),
            "no bins": dict(raster=_abi.FieldDesc(0.0, 0.0, 0.5, 0.5, 0, 64)),
            "too many bins": dict(raster=_abi.FieldDesc(0.0, 0.0, 0.5, 0.5, 4096, 1025)),
            "not a planner": dict(hlp=12345), "a constant planner": dict(hlp=h[id(const)]),
            "a field of another raster": dict(hlp=h[id(other_a)]),
            "slowness nan": dict(slowness=bad(float("nan"))), "slowness inf": dict(slowness=bad(float("inf"))),
            "slowness negative": dict(slowness=bad(-0.5)),
            "speed nan": dict(speed=float("nan")), "speed inf": dict(speed=float("inf")), "speed negative": dict(speed=-1.0),
            "weight negative": dict(weight=-0.25), "weight nan": dict(weight=float("nan")), "weight huge": dict(weight=2.0 ** 33),
            "unknown selection terms": dict(weight=0.5, sel=unknown), "a NaN in the selection": dict(weight=0.5, sel=nan_rect),
            "nothing to write to": dict(outputs=False),
        }
        for name, how in refused.items():
            how = dict(how)
            how.setdefault("hlp", h[id(pa)] if name != "nothing to write to" else NO_PLANNER)
            rc, why = _raw(a, left, blocked=blocked, **how)
            assert rc == 3 and why, name
            print(f"{name}: {why}")
        with pytest.raises(CrowdSimError):
            a.solve_flow_field((0.0, 0.0), 0.5, left, -1.0, planner=pa)
        with pytest.raises(CrowdSimError):
            a.solve_flow_field((0.0, 0.0), 0.25, left, 1.0, planner=pa)  # (not the planner's raster)
        # the planner still holds the field to the right: the next steps are the twin's
        for _ in range(3):
            a.step(DT, report=False)
            b.step(DT)
        assert a.read_agents().tobytes() == b.read_agents().tobytes()
        # ... and a valid call then succeeds, -0.0 slowness and the largest weight included
        before = a.read_agents()
        rc, why = _raw(a, left, blocked=blocked, hlp=h[id(pa)], slowness=bad(-0.0), weight=2.0 ** 32, speed=WALK)
        assert rc == 0, why
        pb.solve(left, WALK, blocked=blocked, slowness=bad(0.0), density_weight=2.0 ** 32, vectors=False)
        for _ in range(2):
            a.step(DT)
            b.step(DT)
        end = a.read_agents()
        assert end.tobytes() == b.read_agents().tobytes() and end["vx"][:100].mean() < before["vx"][:100].mean()
    finally:
        a.close()
        b.close()
