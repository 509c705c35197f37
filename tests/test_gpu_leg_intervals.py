"""Every agent that enters a timed leg on one engine (include/crowdstep_state.h, Simulation.leg_intervals /
count_leg_intervals / free_intervals): the engine against the numpy restatement of the rule
(tests/leg_intervals_reference.py) applied to its OWN read_agents().  Equality is exact: the leg, the id and the bits of
s_in and s_out of every row, the per-leg counts and the returned count; there is no tolerance anywhere (DESIGN.md
section 2, "Every agent that enters a leg")."""
import ctypes as C

import numpy as np
import pytest

from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, LocationHash2D,
                              NoLocalPlan, Selection, Simulation, StubHighLevelPlan, Zanlungo, _abi, scenes)
from rmf_crowdsim_amd.simulation import free_spans, merge_leg_intervals
from rmf_crowdsim_amd.tiles import NativeTileMesh
from close_pairs_reference import roles, takes_part
from leg_intervals_reference import LEG_INTERVAL_DTYPE, SIZE_MAX, agree, call, intervals, last_error, legs_array
from legs_reference import LEG_HIT_DTYPE, NO_HIT
from legs_reference import call as call_conflicts
from select_reference import drain, select, selection
from test_gpu_agent_write import _add_crossing, _steps
from test_gpu_encounters import _advance, _scene
from test_gpu_leg_conflicts import leg_sets, speeds

pytestmark = pytest.mark.gpu
FLAGS = [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER]
INF = float("inf")
MEDIAN = "the median speed"
QUERIES = [(0.5, INF), (1.0, MEDIAN), (0.2, INF)]  # (distance, speed_max)


def interval_legs(rec, grid, seed=7, segments=500):
    """The leg sets of the leg-conflict tests (`segments` random legs) and legs made for the rows of equal velocity: 64 legs
    that walk along with an agent (ids spread over the crowd), 0.1 m beside it with its widened velocity, and waits 0.1 m
    beside up to 20 agents that stand still."""
    part = rec[takes_part(rec, grid)]
    part = part[np.argsort(part["id"])]
    with_ = part[(np.arange(64) * 2 + 1) * len(part) // 128]
    v = np.column_stack([with_["vx"].astype(np.float32).astype(np.float64), with_["vy"].astype(np.float32).astype(np.float64)])
    t0 = np.where(np.arange(64) % 2, 0.5, 0.0)
    along = legs_array(np.column_stack([with_["x"] + v[:, 0] * t0 + 0.1, with_["y"] + v[:, 1] * t0]), v, t0, t0 + 2.0)
    still = part[speeds(part) == 0.0][:20]
    waits = legs_array(np.column_stack([still["x"], still["y"] + 0.1]), (0.0, 0.0), 0.0, 1.5) if len(still) else along[:0]
    return np.concatenate([leg_sets(rec, grid, seed, segments), along, waits])


def check_query(sim, rec, grid, distance, speed_max, name, sel=None, cols=(None, None, None), floors=True, legs=None):
    """One query on the legs: the class counts by the restatement ALONE (printed, then asserted), then the engine against
    it."""
    legs = interval_legs(rec, grid) if legs is None else legs
    if speed_max == MEDIAN:
        speed_max = float(np.median(speeds(rec)))
    stats = {}
    mask = None if sel is None else roles(sel, None, rec, *cols)[0]
    want = intervals(rec, grid, legs, distance, speed_max, mask, stats=stats)
    print(f"  {name}: restatement alone: {len(want[0])} rows, {stats}")
    if floors:
        assert min(stats["at_start"], stats["later"], stats["leaves"], stats["stays"], stats["same_velocity"],
                   stats["crowded_legs"]) >= 20 and stats["free_legs"] >= 5, stats
    agree(sim, rec, grid, legs, distance, speed_max, sel, cols, name, want=want)
    return legs, want, speed_max


def first_of_each_leg(rows, n_legs):
    """per leg the lexicographic minimum of (s_in, id) over its rows as LEG_HIT rows; (CS_NO_HIT, +inf) without rows"""
    out = np.zeros(n_legs, dtype=LEG_HIT_DTYPE)
    out["id"], out["s"] = NO_HIT, INF
    order = np.lexsort((rows["id"], rows["s_in"], rows["leg"]))
    leg = rows["leg"][order].astype(np.int64)
    head = np.nonzero(np.concatenate([[True], leg[1:] != leg[:-1]]))[0] if len(rows) else np.zeros(0, dtype=np.int64)
    out["id"][leg[head]], out["s"][leg[head]] = rows["id"][order][head], rows["s_in"][order][head]
    return out


MANY_LEGS = 2 ** 17 + 3  # leg indices of 18 bits: the sort of a listing runs five passes over the leg half of its keys


def many_legs(rec, grid, n=MANY_LEGS, seed=17):
    """n legs drawn from interval_legs(rec, grid): the same few hundred legs under indices up to n - 1"""
    pool = interval_legs(rec, grid)
    return pool[np.random.default_rng(seed).integers(0, len(pool), n)]


def thin(sim, rec, every):
    """Remove all agents but every `every`-th of `rec` by id -> the records left (the restatement is legs x agents)"""
    ids = np.sort(rec["id"])
    sim.remove_agents_by_id(np.setdiff1d(ids, ids[::every]).tolist())
    left = sim.read_agents()
    assert sorted(left["id"].tolist()) == ids[::every].tolist()
    return left


def long_listing_alone(left, grid, legs, distance, speed_max, name):
    """The restatement ALONE on a listing of many legs (printed, then asserted): at least 1,000 rows at legs from 2^16 on,
    rows in at least 16 of the groups leg >> 13.  -> (rows, counts)"""
    rows, counts = intervals(left, grid, legs, distance, speed_max)
    high, groups = int((rows["leg"] >= 2 ** 16).sum()), len(np.unique(rows["leg"].astype(np.int64) >> 13))
    print(f"  {name}: restatement alone: {len(legs)} legs against {len(left)} agents: {len(rows)} rows, {high} of them at "
          f"legs from 2^16 on, in {groups} groups of 2^13 legs")
    assert high >= 1000 and groups >= 16
    return rows, counts


def check_long_listing(sim, left, grid, legs, distance, speed_max, name, want):
    """An engine (or a mesh) against the restatement's (rows, counts) of a long listing: listing and counting, a cap at
    half the rows, the Python surface's counts, and cs_leg_conflicts on the same legs against the first row of each."""
    rows, counts = want
    agree(sim, left, grid, legs, distance, speed_max, name=name, want=want)
    cap = len(rows) // 2
    got, per_leg, out = call(sim, legs, distance, speed_max, cap=cap)
    assert got == len(rows) and per_leg.tobytes() == counts.tobytes()
    assert out[:cap].tobytes() == rows[:cap].tobytes() and (out[cap:].view(np.uint8) == 0xAB).all()
    assert sim.count_leg_intervals(legs, distance, speed_max).tobytes() == counts.tobytes()
    hits, first = call_conflicts(sim, legs, distance, speed_max)
    assert hits == int((counts > 0).sum())
    assert first[:len(legs)].tobytes() == first_of_each_leg(rows, len(legs)).tobytes()


@pytest.mark.parametrize("where", ["a square grid", "odd-cell"])
def test_a_listing_of_two_to_the_17_legs(where):
    """2^17 + 3 legs against about 300 agents: rows whose leg index needs bits 16 and 17 of the key's leg half (the other
    listings of this module have at most 700 legs, 10 bits), on the crossing crowd's grid of 2 m cells and on the 0.7 m
    cells of tests/odd_grids.py.  The legs are made from the whole crowd, which is then thinned."""
    if where == "odd-cell":
        import odd_grids as og
        sc = og.scene(where)
        a, grid, distance = og.stepped(sc, lambda g: Simulation(LocationHash2D(**g))), sc.grid, 0.4 * sc.cell
        every = 7
    else:
        a, led, _, grid = _scene(0, 1024)
        _advance(a, led, 40)
        distance, every = 0.5, 3
    rec = a.read_agents()
    legs = many_legs(rec, grid)
    left = thin(a, rec, every)
    assert 250 <= len(left) <= 350 and takes_part(left, grid).all()
    want = long_listing_alone(left, grid, legs, distance, 2.0, where)
    check_long_listing(a, left, grid, legs, distance, 2.0, where, want)
    assert a.read_agents().tobytes() == left.tobytes()


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", [1024, 4096])
def test_the_crossing_crowd_equals_the_restatement(n, flags):
    a, led, _, grid = _scene(flags, n)
    _advance(a, led, 40)
    rec = a.read_agents()
    assert len(rec) == n and takes_part(rec, grid).all()
    for distance, speed_max in QUERIES:
        legs, (rows, counts), speed_max = check_query(a, rec, grid, distance, speed_max,
                                                      f"{n} agents, flags {flags}, {(distance, speed_max)}")
        # consistency with cs_leg_conflicts: the first row of every leg by (s_in, id) is its answer, bit for bit, and the
        # legs with rows are exactly its conflicts
        hits, first = call_conflicts(a, legs, distance, speed_max)
        assert hits == int((counts > 0).sum()) and ((first["id"][:len(legs)] != NO_HIT) == (counts > 0)).all()
        assert first[:len(legs)].tobytes() == first_of_each_leg(rows, len(legs)).tobytes()
        T = (legs["t1"] - legs["t0"])[rows["leg"].astype(np.int64)]
        assert (0.0 <= rows["s_in"]).all() and (rows["s_in"] <= rows["s_out"]).all() and (rows["s_out"] <= T).all()
    # cap below the count: the prefix and nothing beyond it; out_counts sums to the returned count whatever cap is
    for cap in (1, len(rows) // 2, len(rows) - 1):
        got, per_leg, out = call(a, legs, distance, speed_max, cap=cap)
        assert got == len(rows) == int(per_leg.sum()) and per_leg.tobytes() == counts.tobytes()
        assert out[:cap].tobytes() == rows[:cap].tobytes() and (out[cap:].view(np.uint8) == 0xAB).all()
    # the Python surface (the last query)
    got = a.leg_intervals(legs, distance, speed_max)
    assert got.dtype == LEG_INTERVAL_DTYPE and got.tobytes() == rows.tobytes()
    assert a.leg_intervals(legs, distance, speed_max, limit=7).tobytes() == rows[:7].tobytes()
    per_leg = a.count_leg_intervals(legs, distance, speed_max)
    assert per_leg.dtype == np.uint64 and per_leg.tobytes() == counts.tobytes()
    assert a.leg_intervals(legs[:0], 0.5, 2.0).shape == (0,) and a.count_leg_intervals(legs[:0], 0.5, 2.0).shape == (0,)
    # free_intervals: when is each spot free, against the complement of the restatement's rows
    spots = np.column_stack([rec["x"][::37] + 0.4, rec["y"][::37]])
    waits = legs_array(spots, (0.0, 0.0), 1.0, 6.0, int(rec["id"][0]))
    want = free_spans(*merge_leg_intervals(intervals(rec, grid, waits, 0.5, 2.0)[0], len(waits)), waits["t0"], waits["t1"])
    assert a.free_intervals(spots, 1.0, 6.0, 0.5, 2.0, ignore=int(rec["id"][0])) == want
    kinds = [len(f) for f in want]
    print(f"  free_intervals: {kinds.count(0)} spots never free, {sum(k >= 2 for k in kinds)} free more than once")
    assert all(1.0 <= s < e <= 6.0 for f in want for s, e in f) and any(f != [(1.0, 6.0)] for f in want)
    assert a.read_agents().tobytes() == rec.tobytes()


def test_targets():
    a, led, sinks, grid = _scene(sinks=True)
    _advance(a, led, 40)
    rec = a.read_agents()
    cols = led.columns(rec)
    half = selection(_abi.CS_SEL_RECT, x0=-INF, y0=-INF, x1=float(np.median(rec["x"])), y1=INF)
    of_planner = selection(_abi.CS_SEL_HLP, hlp=int(np.bincount(np.asarray(cols[1]).astype(np.int64)).argmax()))
    nobody = selection(_abi.CS_SEL_LP, lp=12345)
    legs, (everyone, _), _ = check_query(a, rec, grid, 0.5, 2.0, "no targets", floors=False)
    keys = set(zip(everyone["leg"].tolist(), everyone["id"].tolist()))
    for name, sel in (("a region", half), ("a planner", of_planner)):
        _, (rows, _), _ = check_query(a, rec, grid, 0.5, 2.0, name, sel=sel, cols=cols, floors=False, legs=legs)
        allowed = rec["id"][roles(sel, None, rec, *cols)[0]]
        assert 0 < len(rows) < len(everyone) and np.isin(rows["id"], allowed).all()
        assert set(zip(rows["leg"].tolist(), rows["id"].tolist())) <= keys  # (the others are transparent, no more)
    _, (rows, counts), _ = check_query(a, rec, grid, 0.5, 2.0, "nobody", sel=nobody, cols=cols, floors=False, legs=legs)
    assert len(rows) == 0 and not counts.any()
    x1 = float(np.median(rec["x"]))
    want = intervals(rec, grid, legs, 0.5, 2.0, roles(half, None, rec, *cols)[0])
    assert a.leg_intervals(legs, 0.5, 2.0, targets=dict(rect=(-INF, -INF, x1, INF))).tobytes() == want[0].tobytes()
    assert a.count_leg_intervals(legs, 0.5, 2.0, targets=Selection(rect=(-INF, -INF, x1, INF))).tobytes() == want[1].tobytes()
    assert a.read_agents().tobytes() == rec.tobytes()


def test_reaches_far_starts_and_an_offset_grid():
    """The grid of the leg-conflict test of this name (30 rows of x from -3, 20 columns of y from 1.5), agents written up to
    its very edges and outside it, walking every way at up to 2 m/s: an empty engine, distance in {0, 0.3, 7, +inf},
    speed_max in {0, 1, +inf}, T == 0, long legs that span more than 16 columns, starts beyond 2^32 cells."""
    grid = dict(width=40.0, height=60.0, cell_size=2.0, offset=(-3.0, 1.5))
    rng = np.random.default_rng(3)
    a = Simulation(LocationHash2D(**grid))
    empty = legs_array([(0.0, 5.0), (10.0, 10.0)], [(1.0, 0.0), (0.0, 0.0)], 0.0, 5.0)
    assert a.leg_intervals(empty, INF, INF).shape == (0,) and a.count_leg_intervals(empty, 0.5, INF).tolist() == [0, 0]
    assert a.free_intervals([(0.0, 5.0)], 0.0, 5.0, 0.5, 2.0) == [[(0.0, 5.0)]]
    pts = np.column_stack([rng.uniform(-2.5, 56.5, 700), rng.uniform(2.0, 41.0, 700)])  # (a step stays inside the grid)
    pts[:8] = [(-3.0, 1.5), (56.99, 41.49), (-3.0, 41.4), (56.9, 1.5), (-3.5, 20.0), (20.0, 43.0), (20.0, 1.0), (20.0, 41.5)]
    a.add_agents(pts[:8], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 2.0)  # on the edges and outside: they stand still
    for k in range(7):  # seven planners: still, and six headings at 0.3 to 2 m/s
        v = (0.0, 0.0) if k == 0 else (0.33 * k * np.cos(k), 0.33 * k * np.sin(k))
        a.add_agents(pts[8 + k::7], StubHighLevelPlan(v), NoLocalPlan(), 2.0)
    a.step(0.05)
    rec = a.read_agents()
    part = takes_part(rec, grid)
    assert 690 <= part.sum() < 700 and speeds(rec).min() == 0.0 and speeds(rec).max() > 1.5  # (the outsiders are never rows)
    legs = interval_legs(rec, grid, seed=11)
    assert len(legs) == 596 + 64 + 20  # (somebody stands still: the waits are there)
    for speed_max in (0.0, 1.0, INF):
        for distance in (0.0, 0.3, 7.0, INF):
            stats = {}
            rows, counts = agree(a, rec, grid, legs, distance, speed_max, stats=stats,
                                 name=f"offset grid, distance {distance}, speed_max {speed_max}")
            if distance == 0.0 or speed_max == 0.0:
                assert len(rows) == 0
            elif distance == INF:  # [0, T] for every slow participant the leg does not ignore
                T = (legs["t1"] - legs["t0"])[rows["leg"].astype(np.int64)]
                slow = int((part & (speeds(rec) < speed_max)).sum())
                assert (rows["s_in"] == 0.0).all() and (rows["s_out"] == T).all() and slow - 1 <= counts.min() <= counts.max() == slow
            elif (distance, speed_max) == (0.3, INF):
                print(f"    {stats}")
                assert min(stats["at_start"], stats["later"], stats["leaves"], stats["stays"], stats["same_velocity"]) >= 20
            assert not np.isin(rows["id"], rec["id"][~part]).any()
    still = legs.copy()
    still["t1"] = still["t0"]
    assert len(agree(a, rec, grid, still, 1.0, INF, name="T == 0")[0]) == 0
    # long legs: across the whole grid along y (20 columns of one row) and along x (30 rows), diagonal, both senses
    at = np.linspace(-1.0, 55.0, 29)
    starts = np.concatenate([np.column_stack([at, np.full_like(at, -2.0)]), np.column_stack([at + 0.3, np.full_like(at, 45.0)]),
                             np.column_stack([np.full_like(at, -6.0), at * 0.7 + 2.0]), np.column_stack([np.full_like(at, -5.0), at * 0.7])])
    vel = np.concatenate([np.repeat([[0.0, 3.0]], 29, axis=0), np.repeat([[0.0, -3.0]], 29, axis=0),
                          np.repeat([[4.0, 0.0]], 29, axis=0), np.repeat([[4.0, 1.5]], 29, axis=0)])
    long_ = legs_array(starts, vel, 0.0, 16.0)
    for distance, speed_max in ((0.3, 2.5), (1.0, INF)):
        rows, counts = agree(a, rec, grid, long_, distance, speed_max, name=f"long legs {(distance, speed_max)}")
        assert (counts >= 2).sum() >= 10  # (a long leg meets several agents, one after the other)
    # a reach that covers the whole grid: speed_max * t1 of 200 m, finite
    wide = legs_array(pts[98:147] + 0.3, (0.0, 0.0), 90.0, 100.0)
    assert len(agree(a, rec, grid, wide, 0.5, 2.0, name="grow of 200 m")[0]) >= 5
    # far starts: beyond 2^32 cells, and merely far; the probe rushes in and meets the crowd late in the leg
    start, vel = [], []
    for far in (1e5, 1e8, 1e10, 1e12, 1e300):
        for k in range(12):
            target = pts[20 + k]
            start += [(target[0] - far, target[1]), (target[0], target[1] + far), (target[0] - far, target[1] - far)]
            vel += [(far / 8.0, 0.0), (0.0, -far / 8.0), (far / 8.0, far / 8.0)]
    far_legs = legs_array(start, vel, 0.0, 9.0)
    for distance in (0.3, 3.0):
        rows, counts = agree(a, rec, grid, far_legs, distance, 2.5, name=f"far starts, distance {distance}")
    assert (counts[:36] > 0).sum() >= 12
    assert a.read_agents().tobytes() == rec.tobytes()


def test_refusals():
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    a = Simulation(LocationHash2D(**grid))
    a.add_agents([(3.0, 4.0), (8.0, 4.0), (30.0, 30.0)], StubHighLevelPlan((0.1, 0.0)), NoLocalPlan(), 2.0)
    a.step(0.05)
    rec = a.read_agents()
    good = legs_array([(1.0, 4.0)] * 6, [(1.0, 0.0)] * 6, 0.0, 10.0)
    usable, counts = agree(a, rec, grid, good, 0.5, 2.0, name="three agents")
    assert usable["id"].tolist() == [0, 1] * 6 and counts.tolist() == [2] * 6
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
        for cap in (12, 0):
            got, per_leg, out = call(a, legs, distance, speed_max, sel, cap=cap, n=n)
            assert got == SIZE_MAX and "leg_intervals" in last_error(a), name
            assert (out.view(np.uint8) == 0xAB).all() and (per_leg.view(np.uint8) == 0xAB).all(), name  # (nothing written)
        if legs is not good:
            assert "leg 3" in last_error(a), (name, last_error(a))  # the first bad leg, by its index
        assert a.read_agents().tobytes() == rec.tobytes(), name
        assert call(a, good, 0.5, 2.0, cap=12)[2][:12].tobytes() == usable.tobytes(), name
    two = bad("vx", nan, 5)
    two["t1"][2] = -1.0
    assert call(a, two, 0.5, 2.0, cap=12)[0] == SIZE_MAX and "leg 2" in last_error(a)
    out = np.zeros(4, dtype=LEG_INTERVAL_DTYPE)
    assert a._lib.cs_leg_intervals(a._engine, None, 4, 0.5, 2.0, None, None, out.ctypes.data_as(C.POINTER(_abi.LegInterval)),
                                   4) == SIZE_MAX
    assert "leg_intervals" in last_error(a) and not out.view(np.uint8).any()
    assert a._lib.cs_leg_intervals(a._engine, None, 0, 0.5, 2.0, None, None, None, 0) == 0  # no legs: nothing to do
    agree(a, rec, grid, bad("t1", 0.0), 0.5, 2.0, name="t1 == t0 == 0 is admitted")
    agree(a, rec, grid, good, INF, INF, name="+inf is admitted")
    v = float(rec["vx"][0])  # speed_max at an agent's own speed leaves it out (strict), its upper neighbour takes it
    assert len(agree(a, rec, grid, good, 0.5, v, name="speed_max == the speed")[0]) == 0
    assert len(agree(a, rec, grid, good, 0.5, float(np.nextafter(v, INF)), name="speed_max just above")[0]) == 12
    with pytest.raises(CrowdSimError, match="leg_intervals"):
        a.leg_intervals(legs_array([(1.0, 4.0)], [(0.0, 0.0)], 2.0, 1.0), 0.5, 2.0)
    with pytest.raises(CrowdSimError, match="leg_intervals"):
        a.count_leg_intervals(good, 0.5, 2.0, targets=dict(circle=(0.0, 0.0, -2.0)))
    assert a.read_agents().tobytes() == rec.tobytes()
    a.step(0.05)
    assert a.leg_intervals(good, 0.5, 2.0)["id"].tolist() == [0, 1] * 6


def test_after_removing_a_third_of_the_crowd():
    a, led, _, grid = _scene(0, 4096)
    _advance(a, led, 20)
    rec = a.read_agents()
    a.remove_agents_by_id(rec["id"][::3].tolist())
    left = a.read_agents()
    assert len(left) == len(rec) - len(rec[::3])
    legs = interval_legs(rec, grid)  # (from the crowd as it was: a third of the agents the legs name are gone)
    for distance, speed_max in ((0.5, INF), (0.5, 2.0)):
        rows, _ = agree(a, left, grid, legs, distance, speed_max, name=f"a third removed, {(distance, speed_max)}")
        assert not np.isin(rows["id"], rec["id"][::3]).any() and len(rows) >= 100
    _advance(a, led, 5)
    agree(a, a.read_agents(), grid, legs, 0.5, 2.0, name="five steps later")


def test_wide_ids_by_external_id(monkeypatch):
    """Ids above 2^32 come back in ascending order, and `ignore` is taken in external ids, before and after a renumbering."""
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
        legs = interval_legs(rec, grid)
        rows, counts = agree(a, rec, grid, legs, 0.5, 2.0, name=when)
        assert len(rows) >= 100 and int(rows["id"].min()) > 2 ** 32 and (counts >= 2).sum() >= 5
        ignored = rows[rows["leg"] < 48]
        assert (ignored["id"] != legs["ignore"][ignored["leg"].astype(np.int64)]).all() and int(legs["ignore"][:48].min()) > 2 ** 32

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
    """The engines of a 2 x 2 mesh asked directly between two steps, 40 steps in: each lists the agents it holds, and the
    rows of the four together are the whole answer.  (Despite the name no tile holds a ghost here: a step leaves a tile
    exactly the agents it stepped.  Tiles that do hold ghosts, after an unpack driven by the host, are asked in
    test_gpu_queries_ghost_tiles.py.)"""
    from test_gpu_encounters_mesh import _crowd
    pts, group, grid = _crowd()
    mesh = NativeTileMesh(LocationHash2D(**grid), (2, 2), 1)
    _add_crossing(mesh, pts, group)
    for _ in range(40):
        mesh.step(0.05)
    rec = mesh.read_agents()
    legs = interval_legs(rec, grid)
    counts = mesh.tile_counts().reshape(-1)
    whole, whole_counts = intervals(rec, grid, legs, 0.5, 2.0)
    parts, total = [], np.zeros(len(legs), dtype=np.uint64)
    for k in range(len(counts)):
        mine = select(mesh.tile(k), selection(0), cap=len(rec))[1]  # (a selection on a tile engine matches the agents it owns)
        owned = np.isin(rec["id"], np.asarray(mine, dtype=rec["id"].dtype))
        assert owned.sum() == len(mine) == counts[k] and 0 < counts[k] < len(rec)
        rows, per_leg = agree(mesh.tile(k), rec[owned], grid, legs, 0.5, 2.0, name=f"tile {k}")
        assert 0 < len(rows) < len(whole)  # (no tile alone gives the answer)
        parts.append(rows)
        total += per_leg
    merged = np.concatenate(parts)
    merged = merged[np.lexsort((merged["id"], merged["leg"]))]
    assert merged.tobytes() == whole.tobytes() and total.tobytes() == whole_counts.tobytes()


@pytest.mark.parametrize("flags", [0, CS_CFG_FORCE_TILED])
def test_twins_one_of_which_asks_between_steps(flags):
    """One twin asks after every step from 20 to 30, the other never does: the same bytes, events and report."""
    twins = [_scene(flags, 4096, sinks=True) for _ in range(2)]
    (a, led_a, _, grid), (b, led_b, _, _) = twins
    for s, led, _, _ in twins:
        _advance(s, led, 20)
    rec = a.read_agents()
    assert rec.tobytes() == b.read_agents().tobytes()
    legs = interval_legs(rec, grid)
    for _ in range(10):
        assert 0 < int(a.count_leg_intervals(legs, 0.5, 2.0).sum())
        assert len(a.leg_intervals(legs, 0.3, INF, targets=dict(source_sink=0), limit=50)) <= 50
        a.free_intervals(np.column_stack([rec["x"][:16], rec["y"][:16]]), 0.0, 2.0, 0.5, 2.0)
        _steps((a, b), 1)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert drain(a) == drain(b)
    assert a.last_report == b.last_report


def test_a_total_beyond_32_bits_is_counted_and_not_listed():
    """2^20 waiting legs at distance +inf against 4,096 agents: every agent is a row of every leg, 2^32 rows in all.  The
    count-only form gives them exactly; a listing is refused, writes nothing and leaves the engine usable."""
    a, led, _, grid = _scene(0, 4096)
    _advance(a, led, 5)
    rec = a.read_agents()
    assert len(rec) == 4096 and takes_part(rec, grid).all()
    legs = legs_array(np.zeros((_abi.CS_LEGS_MAX, 2)), (0.0, 0.0), 0.0, 1.0)
    got, per_leg, none = call(a, legs, INF, INF, rows=False)
    assert got == 2 ** 32 and none is None and (per_leg == 4096).all()
    got, per_leg, out = call(a, legs, INF, INF, cap=3)
    assert got == SIZE_MAX and "too many intervals to list" in last_error(a)
    assert (out.view(np.uint8) == 0xAB).all() and (per_leg.view(np.uint8) == 0xAB).all()
    with pytest.raises(CrowdSimError, match="too many intervals to list"):
        a.leg_intervals(legs, INF, INF)
    assert int(a.count_leg_intervals(legs[:1000], INF, INF).sum()) == 4096000
    agree(a, rec, grid, interval_legs(rec, grid), 0.5, 2.0, name="after the refusal")
    assert a.read_agents().tobytes() == rec.tobytes()
