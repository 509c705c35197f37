"""Paths against the moving crowd on one engine (include/crowdstep_state.h, Simulation.leg_conflicts / count_leg_conflicts /
path_conflict): the engine against the numpy restatement of the rule (tests/legs_reference.py) applied to its OWN
read_agents().  Equality is exact: the id and the bits of s of every leg, and the returned count; there is no tolerance
anywhere ("Paths against the moving crowd")."""
import ctypes as C

import numpy as np
import pytest

from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, LocationHash2D,
                              NoLocalPlan, Selection, Simulation, StubHighLevelPlan, Zanlungo, _abi, scenes)
from rmf_crowdsim_amd.simulation import paths_legs
from rmf_crowdsim_amd.tiles import NativeTileMesh
from close_pairs_reference import rectangle, roles, takes_part
from legs_reference import LEG_HIT_DTYPE, NO_HIT, SIZE_MAX, agree, call, classes, conflicts, last_error, legs_array
from select_reference import NO_SINK, drain, select, selection
from test_gpu_agent_write import _add_crossing, _steps
from test_gpu_encounters import _advance, _scene

pytestmark = pytest.mark.gpu
FLAGS = [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER]
INF = float("inf")
MEDIAN = "the median speed"
QUERIES = [(0.5, INF), (1.0, MEDIAN), (0.2, INF)]  # (distance, speed_max)
FLOORS = [20, 20, 5]  # of conflicts at s == 0, of conflicts at s > 0 and of misses, query by query


def speeds(rec):
    vx, vy = rec["vx"].astype(np.float32).astype(np.float64), rec["vy"].astype(np.float32).astype(np.float64)
    return np.sqrt(vx * vx + vy * vy)


def robot_paths(rec, grid, rng, robots=8, pieces=6, with_ignore=True):
    """`robots` paths of `pieces` legs of 1 s each from agents' positions (ids spread over the crowd), the headings random
    at 1 m/s, the third leg of each a wait; ignore: the agent the path starts on, or nobody."""
    part = rec[takes_part(rec, grid)]
    part = part[np.argsort(part["id"])]
    who = part[(np.arange(robots) * 2 + 1) * len(part) // (2 * robots)]
    out = []
    for a in who:
        phi = rng.uniform(0.0, 2.0 * np.pi, pieces)
        v = np.column_stack([np.cos(phi), np.sin(phi)])
        v[2] = 0.0
        p = np.array([a["x"], a["y"]]) + np.concatenate([[[0.0, 0.0]], np.cumsum(v[:-1] * 1.0, axis=0)])
        t0 = np.arange(pieces, dtype=np.float64)
        out.append(legs_array(p, v, t0, t0 + 1.0, a["id"] if with_ignore else None))
    return np.concatenate(out)


def leg_sets(rec, grid, seed=7, segments=500):
    """The legs of one check, from the engine's own records: eight robot paths with `ignore` set to the agent each starts
    on, the same paths without it (each first leg then conflicts with that agent at s == 0), and `segments` random legs:
    three in five start within a few metres of somebody, the others anywhere up to 10 m outside the grid's rectangle;
    speeds from {0, 0.5, 1, 2}, t0 from {0, 0.5, 2}, durations from {0.5, 1, 3}; every sixth leg parallel to an axis (vx == 0.0
    or vy == 0.0 exactly, at a speed that is not 0)."""
    rng = np.random.default_rng(seed)
    with_ignore = robot_paths(rec, grid, np.random.default_rng(seed + 1))
    without = robot_paths(rec, grid, np.random.default_rng(seed + 1), with_ignore=False)
    part = rec[takes_part(rec, grid)]
    crowd = np.column_stack([part["x"], part["y"]])
    gx0, gx1, gy0, gy1 = rectangle(grid)
    start = np.column_stack([rng.uniform(gx0 - 10.0, gx1 + 10.0, segments), rng.uniform(gy0 - 10.0, gy1 + 10.0, segments)])
    near = np.arange(segments) % 5 < 3
    start[near] = crowd[rng.integers(0, len(crowd), int(near.sum()))] + rng.normal(0.0, 2.0, (int(near.sum()), 2))
    start[0] = (gx0 - 10.0, gy0 - 10.0)
    phi = rng.uniform(0.0, 2.0 * np.pi, segments)
    speed = rng.choice([0.0, 0.5, 1.0, 2.0], segments)
    speed[0::6] = np.where(speed[0::6] == 0.0, 1.0, speed[0::6])
    v = np.column_stack([np.cos(phi), np.sin(phi)]) * speed[:, None]
    v[0::12] = np.column_stack([np.zeros(len(v[0::12])), np.where(v[0::12, 1] < 0.0, -1.0, 1.0) * speed[0::12]])
    v[6::12] = np.column_stack([np.where(v[6::12, 0] < 0.0, -1.0, 1.0) * speed[6::12], np.zeros(len(v[6::12]))])
    t0 = rng.choice([0.0, 0.5, 2.0], segments)
    legs = np.concatenate([with_ignore, without, legs_array(start, v, t0, t0 + rng.choice([0.5, 1.0, 3.0], segments))])
    assert ((legs["vx"] == 0.0) & (legs["vy"] != 0.0)).sum() >= segments // 13
    assert ((legs["vy"] == 0.0) & (legs["vx"] != 0.0)).sum() >= segments // 13
    assert ((legs["vx"] == 0.0) & (legs["vy"] == 0.0)).sum() >= 16 + segments // 8  # (waits)
    return legs


def check_query(sim, rec, grid, distance, speed_max, name, floor=20, sel=None, cols=(None, None, None), want_classes=True,
                legs=None):
    """One query on the leg sets: the class counts by the restatement ALONE (printed, then asserted), then the engine
    against it."""
    legs = leg_sets(rec, grid) if legs is None else legs
    if speed_max == MEDIAN:
        speed_max = float(np.median(speeds(rec)))
    stats = {}
    mask = None if sel is None else roles(sel, None, rec, *cols)[0]
    want = conflicts(rec, grid, legs, distance, speed_max, mask, stats=stats)
    moving, still, miss = classes(want)
    changed = 0
    if speed_max != INF:
        everyone = conflicts(rec, grid, legs, distance, INF, mask)
        changed = int(((everyone["id"] != want["id"]) | (everyone["s"].view(np.uint64) != want["s"].view(np.uint64))).sum())
    print(f"  {name}: restatement alone: {still} conflicts at s == 0, {moving} at s > 0, {miss} misses, "
          f"{stats['not_nearest']} winners that are not the candidate nearest the leg's start, "
          f"the speed filter changes {changed} answers")
    if want_classes:
        assert still >= floor and moving >= floor and miss >= floor and stats["not_nearest"] >= 5
        assert speed_max == INF or changed >= 20
    agree(sim, rec, grid, legs, distance, speed_max, sel, cols, name, want=want)
    return legs, want, speed_max


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", [1024, 4096])
def test_the_crossing_crowd_equals_the_restatement(n, flags):
    a, led, _, grid = _scene(flags, n)
    _advance(a, led, 40)
    rec = a.read_agents()
    assert len(rec) == n and takes_part(rec, grid).all()
    for (distance, speed_max), floor in zip(QUERIES, FLOORS):
        legs, want, speed_max = check_query(a, rec, grid, distance, speed_max,
                                            f"{n} agents, flags {flags}, {(distance, speed_max)}", floor)
        first = np.arange(48, 96, 6)  # the first legs of the paths without ignore: the agent itself, at once
        if speed_max == INF:
            assert (want["s"][first] == 0.0).all() and (want["id"][first] <= legs["ignore"][first - 48]).all()
    # the Python surface (the last query)
    got = a.leg_conflicts(legs, distance, speed_max)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert a.count_leg_conflicts(legs, distance, speed_max) == int((want["id"] != NO_HIT).sum())
    seven = legs_array(np.column_stack([legs["x0"], legs["y0"]])[100:107], (0.5, -0.25), 0.5, 2.0, int(legs["ignore"][0]))  # scalars
    assert len(seven) == 7 and a.leg_conflicts(seven, 0.5, 2.0).tobytes() == conflicts(rec, grid, seven, 0.5, 2.0).tobytes()
    assert a.leg_conflicts(np.zeros(0, dtype=legs.dtype), 0.5, 2.0).shape == (0,)
    # path_conflict: the first leg in path order with a conflict, by a reduction of the restatement's rows
    rng = np.random.default_rng(23)
    some, free = 0, 0
    for k in range(24):
        at = rec[rng.integers(0, len(rec))]
        pts = np.array([at["x"], at["y"]]) + np.cumsum(rng.normal(0.0, 1.0, (6, 2)), axis=0)
        pts[3] = pts[2]  # a wait
        times = np.array([0.0, 1.0, 2.0, 3.5, 3.5, 5.0]) + 0.25 * (k % 3)  # (a zero-duration piece is dropped)
        ignore = int(at["id"]) if k % 2 else None
        path, owner = paths_legs([(pts, times)])
        assert len(path) == 4 and owner.tolist() == [0] * 4
        if ignore is not None:
            path["ignore"] = ignore
        rows = conflicts(rec, grid, path, 0.5, 2.0)
        hit = np.nonzero(rows["id"] != NO_HIT)[0]
        got = a.path_conflict(pts, times, 0.5, 2.0, ignore=ignore)
        if not len(hit):
            free += 1
            assert got is None
            continue
        some += 1
        j = int(hit[0])
        s = float(rows["s"][j])
        assert got == (int(rows["id"][j]), float(path["t0"][j]) + s, j,
                       (float(path["x0"][j]) + float(path["vx"][j]) * s, float(path["y0"][j]) + float(path["vy"][j]) * s))
    print(f"  path_conflict: {some} paths with a conflict, {free} free")
    assert some >= 5
    # many paths in one call, reduced with numpy
    many, owner = paths_legs([(np.array([r["x"], r["y"]]) + np.array([[0.0, 0.3], [2.0, 0.3], [2.0, 2.3]]), [0.0, 2.0, 4.0])
                              for r in rec[::97]])
    assert a.leg_conflicts(many, 0.4, 2.0).tobytes() == conflicts(rec, grid, many, 0.4, 2.0).tobytes()
    assert a.read_agents().tobytes() == rec.tobytes()


def test_targets():
    a, led, sinks, grid = _scene(sinks=True)
    _advance(a, led, 40)
    rec = a.read_agents()
    cols = led.columns(rec)
    owners = np.asarray(cols[0])
    spawned = [int(s) for s in np.unique(owners) if int(s) != NO_SINK]
    assert spawned  # (agents of a source-sink are alive)
    half = selection(_abi.CS_SEL_RECT, x0=-INF, y0=-INF, x1=float(np.median(rec["x"])), y1=INF)
    of_planner = selection(_abi.CS_SEL_HLP, hlp=int(np.bincount(np.asarray(cols[1]).astype(np.int64)).argmax()))
    of_sink = selection(_abi.CS_SEL_SOURCE_SINK, source_sink=spawned[0])
    nobody = selection(_abi.CS_SEL_LP, lp=12345)
    legs, everyone, _ = check_query(a, rec, grid, 0.5, 2.0, "no targets", want_classes=False)
    for name, sel in (("a region", half), ("a planner", of_planner), ("a source-sink", of_sink)):
        _, want, _ = check_query(a, rec, grid, 0.5, 2.0, name, sel=sel, cols=cols, want_classes=False, legs=legs)
        hit = want["id"] != NO_HIT
        allowed = set(rec["id"][roles(sel, None, rec, *cols)[0]].tolist())
        assert set(want["id"][hit].tolist()) <= allowed and (want["s"] >= everyone["s"]).all()
        if sel is not of_sink:
            assert hit.any() and (want["id"] != everyone["id"]).any()  # (the others are transparent)
    # waits on top of the agents of that source-sink, through whoever stands nearer
    theirs = rec[owners == spawned[0]]
    waits = legs_array(np.column_stack([theirs["x"] + 0.1, theirs["y"]]), (0.0, 0.0), 0.0, 1.0)
    want = agree(a, rec, grid, waits, 0.3, INF, of_sink, cols, "waits on the agents of a source-sink")
    assert (want["s"] == 0.0).all() and set(want["id"].tolist()) <= set(theirs["id"].tolist())
    _, want, _ = check_query(a, rec, grid, 0.5, 2.0, "nobody", sel=nobody, cols=cols, want_classes=False, legs=legs)
    assert (want["id"] == NO_HIT).all() and np.isinf(want["s"]).all()
    # the Python surface: dicts and Selections
    x1 = float(np.median(rec["x"]))
    want = conflicts(rec, grid, legs, 0.5, 2.0, roles(half, None, rec, *cols)[0])
    assert a.leg_conflicts(legs, 0.5, 2.0, targets=dict(rect=(-INF, -INF, x1, INF))).tobytes() == want.tobytes()
    assert a.count_leg_conflicts(legs, 0.5, 2.0, targets=Selection(rect=(-INF, -INF, x1, INF))) == int((want["id"] != NO_HIT).sum())
    assert a.read_agents().tobytes() == rec.tobytes()


def test_reaches_far_starts_and_an_offset_grid():
    """A grid that is not square and does not start at 0 (30 rows of x from -3, 20 columns of y from 1.5), agents written up
    to its very edges and outside it, walking every way at up to 2 m/s: T == 0, distance == 0, an empty engine, a leg
    wholly outside the grid, a leg that spans more than 16 columns of one row and several rows, a reach that covers the
    whole grid, speed_max == +inf (the full walk), distance == +inf, and starts beyond 2^32 cells."""
    grid = dict(width=40.0, height=60.0, cell_size=2.0, offset=(-3.0, 1.5))
    rng = np.random.default_rng(3)
    a = Simulation(LocationHash2D(**grid))
    empty = legs_array([(0.0, 5.0), (10.0, 10.0)], [(1.0, 0.0), (0.0, 0.0)], 0.0, 5.0)
    assert a.leg_conflicts(empty, 0.5, INF).tolist() == [(_abi.CS_NO_HIT, INF)] * 2  # an empty engine
    assert a.count_leg_conflicts(empty, INF, INF) == 0 and a.path_conflict([(0.0, 5.0), (9.0, 5.0)], [0.0, 4.0], 0.5, 2.0) is None
    pts = np.column_stack([rng.uniform(-2.5, 56.5, 700), rng.uniform(2.0, 41.0, 700)])  # (a step stays inside the grid)
    pts[:8] = [(-3.0, 1.5), (56.99, 41.49), (-3.0, 41.4), (56.9, 1.5), (-3.5, 20.0), (20.0, 43.0), (20.0, 1.0), (20.0, 41.5)]
    a.add_agents(pts[:8], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 2.0)  # on the edges and outside: they stand still
    for k in range(7):  # seven planners: still, and six headings at 0.3 to 2 m/s
        v = (0.0, 0.0) if k == 0 else (0.33 * k * np.cos(k), 0.33 * k * np.sin(k))
        a.add_agents(pts[8 + k::7], StubHighLevelPlan(v), NoLocalPlan(), 2.0)
    a.step(0.05)
    rec = a.read_agents()
    part = takes_part(rec, grid)
    assert 690 <= part.sum() < 700 and speeds(rec).min() == 0.0 and speeds(rec).max() > 1.5  # (the outsiders never conflict)
    legs = leg_sets(rec, grid, seed=11)
    for speed_max in (0.0, 1.0, 2.5, INF):
        for distance in (0.0, 0.3, 1.0, 7.0, 100.0, INF):
            want = agree(a, rec, grid, legs, distance, speed_max, name=f"offset grid, distance {distance}, speed_max {speed_max}")
            if distance == 0.0 or speed_max == 0.0:
                assert (want["id"] == NO_HIT).all()
            assert not np.isin(want["id"], rec["id"][~part]).any()
    still = legs.copy()
    still["t1"] = still["t0"]
    assert (agree(a, rec, grid, still, 1.0, INF, name="T == 0")["id"] == NO_HIT).all()
    # wholly outside the grid, far enough not to be reached, and near enough to be
    out = legs_array([(-40.0, -30.0), (-40.0, 20.0), (70.0, 60.0), (20.0, -6.0)], [(1.0, 0.0), (0.0, 1.0), (0.0, -0.5), (1.0, 0.0)],
                     0.0, [5.0, 5.0, 4.0, 20.0])
    want = agree(a, rec, grid, out, 1.0, 2.5, name="legs outside the grid")
    assert (want["id"][:3] == NO_HIT).all()
    want = agree(a, rec, grid, out, 8.0, 2.5, name="legs outside the grid, 8 m")
    assert want["id"][3] != NO_HIT
    # long legs: across the whole grid along y (20 columns of one row) and along x (30 rows), diagonal, both senses
    at = np.linspace(-1.0, 55.0, 29)
    starts = np.concatenate([np.column_stack([at, np.full_like(at, -2.0)]), np.column_stack([at + 0.3, np.full_like(at, 45.0)]),
                             np.column_stack([np.full_like(at, -6.0), at * 0.7 + 2.0]), np.column_stack([np.full_like(at, -5.0), at * 0.7])])
    vel = np.concatenate([np.repeat([[0.0, 3.0]], 29, axis=0), np.repeat([[0.0, -3.0]], 29, axis=0),
                          np.repeat([[4.0, 0.0]], 29, axis=0), np.repeat([[4.0, 1.5]], 29, axis=0)])
    long_ = legs_array(starts, vel, 0.0, 16.0)
    for distance, speed_max in ((0.3, 2.5), (0.3, 0.5), (1.0, INF)):
        want = agree(a, rec, grid, long_, distance, speed_max, name=f"long legs {(distance, speed_max)}")
        assert 10 <= (want["id"] != NO_HIT).sum()
    # a reach that covers the whole grid: speed_max * t1 of 200 m, finite
    wide = legs_array(pts[98:147] + 0.3, (0.0, 0.0), 90.0, 100.0)  # (seven of them next to somebody who stands still)
    want = agree(a, rec, grid, wide, 0.5, 2.0, name="grow of 200 m")
    assert (want["id"] != NO_HIT).sum() >= 5
    # far starts: beyond 2^32 cells, and merely far; the probe rushes in and meets the crowd late in the leg
    start, vel, t1 = [], [], []
    for far in (1e5, 1e8, 1e10, 1e12, 1e300):
        for k in range(12):
            target = pts[20 + k]
            start += [(target[0] - far, target[1]), (target[0], target[1] + far), (target[0] - far, target[1] - far)]
            vel += [(far / 8.0, 0.0), (0.0, -far / 8.0), (far / 8.0, far / 8.0)]
            t1 += [9.0, 9.0, 9.0]
    far_legs = legs_array(start, vel, 0.0, t1)
    for distance in (0.3, 3.0):
        want = agree(a, rec, grid, far_legs, distance, 2.5, name=f"far starts, distance {distance}")
    assert (want["id"][:36] != NO_HIT).sum() >= 12
    assert a.read_agents().tobytes() == rec.tobytes()


def test_refusals():
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    a = Simulation(LocationHash2D(**grid))
    a.add_agents([(3.0, 4.0), (8.0, 4.0), (30.0, 30.0)], StubHighLevelPlan((0.1, 0.0)), NoLocalPlan(), 2.0)
    a.step(0.05)
    rec = a.read_agents()
    good = legs_array([(1.0, 4.0)] * 6, [(1.0, 0.0)] * 6, 0.0, 10.0)
    usable = conflicts(rec, grid, good, 0.5, 2.0)
    assert usable["id"].tolist() == [0] * 6 and agree(a, rec, grid, good, 0.5, 2.0, name="three agents").tobytes() == usable.tobytes()
    nan = float("nan")

    def bad(field, value, k=3):
        legs = good.copy()
        legs[field][k] = value
        return legs

    bad_terms = selection(1 << 9)
    nan_rect = selection(_abi.CS_SEL_RECT, x0=nan, y0=0.0, x1=1.0, y1=1.0)
    cases = [("NaN distance", good, nan, 2.0, None, None), ("negative distance", good, -0.5, 2.0, None, None),
             ("NaN speed_max", good, 0.5, nan, None, None), ("negative speed_max", good, 0.5, -1e-300, None, None),
             ("too many legs", good, 0.5, 2.0, None, _abi.CS_LEGS_MAX + 1),
             ("unknown terms", good, 0.5, 2.0, bad_terms, None), ("a NaN in the selection", good, 0.5, 2.0, nan_rect, None)]
    for field in ("x0", "y0", "vx", "vy", "t0", "t1"):
        cases += [(f"{field} {v}", bad(field, v), 0.5, 2.0, None, None) for v in (nan, INF, -INF)]
    cases += [("negative t0", bad("t0", -1e-300), 0.5, 2.0, None, None), ("t1 before t0", bad("t0", 11.0), 0.5, 2.0, None, None)]
    for name, legs, distance, speed_max, sel, n in cases:
        for rows in (True, False):
            got, out = call(a, legs, distance, speed_max, sel, rows=rows, fill=0xAB, n=n)
            assert got == SIZE_MAX and "leg_conflicts" in last_error(a), name
            if rows:
                assert (out.view(np.uint8) == 0xAB).all(), name
        if legs is not good:
            assert "leg 3" in last_error(a), (name, last_error(a))  # the first bad leg, by its index
        assert a.read_agents().tobytes() == rec.tobytes(), name
        assert call(a, good, 0.5, 2.0)[1].tobytes() == usable.tobytes(), name
    two = bad("vx", nan, 5)
    two["t1"][2] = -1.0
    assert call(a, two, 0.5, 2.0)[0] == SIZE_MAX and "leg 2" in last_error(a)
    out = np.zeros(4, dtype=LEG_HIT_DTYPE)
    assert a._lib.cs_leg_conflicts(a._engine, None, 4, 0.5, 2.0, None, out.ctypes.data_as(C.POINTER(_abi.LegHit))) == SIZE_MAX
    assert "leg_conflicts" in last_error(a) and not out.view(np.uint8).any()
    assert a._lib.cs_leg_conflicts(a._engine, None, 0, 0.5, 2.0, None, None) == 0  # no legs: nothing to do
    agree(a, rec, grid, bad("t1", 0.0), 0.5, 2.0, name="t1 == t0 == 0 is admitted")
    agree(a, rec, grid, good, INF, INF, name="+inf is admitted")
    # speed_max at an agent's own speed leaves it out (strict), its upper neighbour takes it: the squares are exact here
    v = float(rec["vx"][0])
    assert v == float(np.float32(0.1)) and (rec["vx"] == v).all() and (rec["vy"] == 0.0).all()
    assert (agree(a, rec, grid, good, 0.5, v, name="speed_max == the speed")["id"] == NO_HIT).all()
    assert (agree(a, rec, grid, good, 0.5, float(np.nextafter(v, INF)), name="speed_max just above")["id"] == 0).all()
    with pytest.raises(CrowdSimError, match="leg_conflicts"):
        a.leg_conflicts(legs_array([(1.0, 4.0)], [(0.0, 0.0)], 2.0, 1.0), 0.5, 2.0)
    with pytest.raises(CrowdSimError, match="leg_conflicts"):
        a.count_leg_conflicts(good, 0.5, 2.0, targets=dict(circle=(0.0, 0.0, -2.0)))
    with pytest.raises(ValueError):
        a.path_conflict([(1.0, 4.0), (2.0, 4.0)], [1.0, 0.5], 0.5, 2.0)
    assert a.read_agents().tobytes() == rec.tobytes()
    a.step(0.05)
    assert a.leg_conflicts(good, 0.5, 2.0)["id"].tolist() == [0] * 6


def test_after_removing_a_third_of_the_crowd():
    a, led, _, grid = _scene(0, 4096)
    _advance(a, led, 20)
    rec = a.read_agents()
    a.remove_agents_by_id(rec["id"][::3].tolist())
    left = a.read_agents()
    assert len(left) == len(rec) - len(rec[::3])
    legs = leg_sets(rec, grid)  # (from the crowd as it was: a third of the robots' agents are gone, their ids nobody's)
    for distance, speed_max in ((0.5, INF), (0.5, 2.0)):
        want = agree(a, left, grid, legs, distance, speed_max, name=f"a third removed, {(distance, speed_max)}")
        assert not np.isin(want["id"], rec["id"][::3]).any() and 40 <= (want["id"] != NO_HIT).sum()
    _advance(a, led, 5)
    left = a.read_agents()
    agree(a, left, grid, legs, 0.5, 2.0, name="five steps later")


def test_wide_ids_by_external_id(monkeypatch):
    """Ids above 2^32 come back, and `ignore` is taken in external ids, before and after a renumbering."""
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(2 ** 40 + 1))
    monkeypatch.setenv("CS_DEVICE_ID_LIMIT", "4096")
    pts, grid, extent, group = scenes.uniform_crowd(600, seed=9, cell_size=2.0, room=20.0)
    a = Simulation(LocationHash2D(**grid), flags=CS_CFG_WIDE_IDS)
    monkeypatch.delenv("CS_DEVICE_ID_LIMIT")
    monkeypatch.delenv("CS_FIRST_AGENT_ID")
    ids = scenes.add_counterflow(a, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    assert min(ids) > 2 ** 40
    spot = np.array([[extent + 15.0, extent + 15.0]])
    still, nolp = StubHighLevelPlan((0.0, 0.0)), NoLocalPlan()

    def check(when):
        rec = a.read_agents()
        legs = leg_sets(rec, grid)
        want = agree(a, rec, grid, legs, 0.5, 2.0, name=when)
        hit = want["id"] != NO_HIT
        assert hit.sum() >= 40 and int(want["id"][hit].min()) > 2 ** 32
        assert (want["id"][:48] != legs["ignore"][:48]).all() and int(legs["ignore"][:48].min()) > 2 ** 32
        first = np.arange(48, 96, 6)  # (no ignore: the agent itself, or one with a smaller id as near)
        assert (want["s"][first] == 0.0).all() and (want["id"][first] <= legs["ignore"][first - 48]).all()

    for r in range(6):
        more = a.add_agents(np.repeat(spot, 600, axis=0) + np.arange(600)[:, None] * 0.01, still, nolp, 1.0)
        a.step(0.05)
        if r in (0, 5):
            n_before = a.kernel_stat(_abi.CS_STAT_RENUMBERINGS)
            check(f"round {r}, {n_before} renumberings")
            assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) == n_before
        a.remove_agents_by_id(more[:-1])
    assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) >= 1
    check("at the end")


def test_a_tile_engine_holding_ghosts_answers_for_the_agents_it_owns():
    """The engines of a 2 x 2 mesh asked directly between two steps, 40 steps in: each answers for the agents it holds.
    (Despite the name no tile holds a ghost here: a step leaves a tile exactly the agents it stepped.  Tiles that do hold
    ghosts, after an unpack driven by the host, are asked in test_gpu_queries_ghost_tiles.py.)"""
    from test_gpu_encounters_mesh import _crowd
    pts, group, grid = _crowd()
    mesh = NativeTileMesh(LocationHash2D(**grid), (2, 2), 1)
    _add_crossing(mesh, pts, group)
    for _ in range(40):
        mesh.step(0.05)
    rec = mesh.read_agents()
    legs = leg_sets(rec, grid)
    counts = mesh.tile_counts().reshape(-1)
    whole = conflicts(rec, grid, legs, 0.5, 2.0)
    merged = np.zeros(len(legs), dtype=LEG_HIT_DTYPE)
    merged["id"], merged["s"] = NO_HIT, INF
    differ = 0
    for k in range(len(counts)):
        mine = select(mesh.tile(k), selection(0), cap=len(rec))[1]  # (a selection on a tile engine matches the agents it owns)
        owned = np.isin(rec["id"], np.asarray(mine, dtype=rec["id"].dtype))
        assert owned.sum() == len(mine) == counts[k] and 0 < counts[k] < len(rec)
        want = conflicts(rec[owned], grid, legs, 0.5, 2.0)
        n, got = call(mesh.tile(k), legs, 0.5, 2.0)
        assert n == (want["id"] != NO_HIT).sum() and got[:len(want)].tobytes() == want.tobytes(), k
        differ += int((want["id"] != whole["id"]).sum())
        better = (want["s"] < merged["s"]) | ((want["s"] == merged["s"]) & (want["id"] < merged["id"]))
        merged[better] = want[better]
    assert merged.tobytes() == whole.tobytes() and differ >= 100  # (no tile alone gives the answer)


@pytest.mark.parametrize("flags", [0, CS_CFG_FORCE_TILED])
def test_twins_one_of_which_asks_between_steps(flags):
    """One twin asks after every step from 20 to 30, the other never does: the same bytes, events and report."""
    twins = [_scene(flags, 4096, sinks=True) for _ in range(2)]
    (a, led_a, _, grid), (b, led_b, _, _) = twins
    for s, led, _, _ in twins:
        _advance(s, led, 20)
    rec = a.read_agents()
    assert rec.tobytes() == b.read_agents().tobytes()
    legs = leg_sets(rec, grid)
    for _ in range(10):
        hits = a.count_leg_conflicts(legs, 0.5, 2.0)
        assert 0 < hits < len(legs)
        a.leg_conflicts(legs, 0.3, INF, targets=dict(source_sink=0))
        _steps((a, b), 1)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert drain(a) == drain(b)
    assert a.last_report == b.last_report
