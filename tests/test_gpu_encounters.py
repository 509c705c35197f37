"""Encounters on one engine (include/crowdstep_state.h, Simulation.encounters / count_encounters): the engine against the
numpy restatement of the rule (tests/encounters_reference.py) applied to its OWN read_agents().  Equality is exact: rows,
order, count and the bits of t and d2; no case is left out of a comparison and there is no tolerance anywhere (DESIGN.md
section 2, "Encounters between steps")."""
import numpy as np
import pytest

from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, LocationHash2D,
                              NoLocalPlan, Selection, Simulation, StubHighLevelPlan, Zanlungo, _abi, scenes)
from close_pairs_reference import SIZE_MAX, last_error, pairs, takes_part
from encounters_reference import agree, call, encounters
from select_reference import Ledger, add_three_sinks, drain, keep_events, selection
from test_gpu_agent_write import _add_crossing, _crossing, _steps

pytestmark = pytest.mark.gpu
FLAGS = [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER]
INF = float("inf")
QUERIES = [(0.8, 2.0, 4.0), (1.5, 1.0, 4.0), (0.4, INF, 6.0)]  # (distance, horizon, range)


def _scene(flags=0, n=1024, sinks=False):
    """The crossing crowd (with the three source-sinks of the selection tests if asked) and the ledger of who owns whom."""
    pts, pref, group, grid, extent = _crossing(n)
    s = Simulation(LocationHash2D(**grid), flags=flags)
    led = Ledger(s).watch()
    keep_events(s)
    _add_crossing(s, pts, group)
    handles = add_three_sinks(s, extent) if sinks else []
    return s, led, handles, grid


def _advance(s, led, k):
    for _ in range(k):
        s.step(0.05)
    led.hear(drain(s))


def _classes(rows, horizon):
    t = rows["t"]
    return int((t == 0.0).sum()), int(((t > 0.0) & (t < horizon)).sum()), int((t == horizon).sum())


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", [1024, 4096])
def test_the_crossing_crowd_equals_the_restatement(n, flags):
    a, led, _, grid = _scene(flags, n)
    _advance(a, led, 40)
    rec = a.read_agents()
    assert len(rec) == n and takes_part(rec, grid).all()
    lhs = {} if n == 1024 else None  # (what no parameter enters, once for the three queries, where it fits in memory)
    for distance, horizon, range_ in QUERIES:
        stats = {}
        want = agree(a, rec, grid, distance, horizon, range_, name=f"{n} agents, flags {flags}, {(distance, horizon, range_)}",
                     stats=stats, cache=lhs)
        still, free, clamped = _classes(want, horizon)
        print(f"    t == 0: {still}, 0 < t < horizon: {free}, t == horizon: {clamped}; {stats['in_range']} pairs in range")
        assert (want["a"] < want["b"]).all() and (want["t"] >= 0.0).all() and (want["t"] <= horizon).all()
        if horizon < INF:  # (by the restatement alone: every branch of the rule is taken, and the rule selects)
            assert still >= 5 and free >= 5 and clamped >= 5 and len(want) < stats["in_range"]
    # the Python surface
    want = encounters(rec, grid, 0.8, 2.0, 4.0, cache=lhs)
    got = a.encounters(0.8, 2.0, 4.0)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert a.encounters(0.8, 2.0, 4.0, limit=5).tobytes() == want[:5].tobytes()
    assert a.count_encounters(0.8, 2.0, 4.0) == len(want)
    assert a.read_agents().tobytes() == rec.tobytes()


def test_identities_with_the_pairs():
    """horizon 0: the pairs of close_pairs(min(distance, range)) with their d2; distance +inf: the pairs in range."""
    a, led, _, grid = _scene()
    _advance(a, led, 40)
    rec = a.read_agents()
    for distance, range_ in ((0.8, 4.0), (4.0, 0.8), (3.0, 3.0), (INF, 2.5), (1.5, INF), (0.0, 4.0), (4.0, 0.0)):
        got = a.encounters(distance, 0.0, range_)
        listed, d2 = a.close_pairs(min(distance, range_), distances=True)
        print(f"  horizon 0, distance {distance}, range {range_}: {len(got)} encounters, {len(listed)} pairs")
        assert len(got) == len(listed) and (len(got) > 0) == (min(distance, range_) > 0.0)
        assert np.array_equal(got["a"], listed[:, 0]) and np.array_equal(got["b"], listed[:, 1])
        assert got["d2"].tobytes() == d2.tobytes() and not got["t"].any() and not np.signbit(got["t"]).any()
        assert a.count_encounters(distance, 0.0, range_) == len(listed)
    for horizon, range_ in ((0.0, 4.0), (2.0, 4.0), (INF, 4.0), (1.0, 0.7), (3.0, 7.5)):
        n = a.count_encounters(INF, horizon, range_)
        assert n == a.count_close_pairs(range_) > 0, (horizon, range_)
        rows = a.encounters(INF, horizon, range_)
        assert len(rows) == n and np.isfinite(rows["d2"]).all()
        want = encounters(rec, grid, INF, horizon, range_)
        assert np.array_equal(rows["a"], want["a"]) and np.array_equal(rows["b"], want["b"])
    assert a.read_agents().tobytes() == rec.tobytes()


def test_edges_to_the_bit():
    """For 40 sampled encounters: `distance` at sqrt(m2) and its two f64 neighbours, `horizon` at the pair's unclamped t
    and its two neighbours, `range` at sqrt(d2) and its two neighbours.  The engine and the restatement agree whichever
    way each case falls (a fused multiply-add, a reciprocal or an f32 shortcut would not)."""
    a, led, _, grid = _scene()
    _advance(a, led, 40)
    rec = a.read_agents()
    lhs = {}  # (what no parameter enters, computed once for all the queries on this crowd)
    distance, horizon, range_ = 0.8, 2.0, 4.0
    base = agree(a, rec, grid, distance, horizon, range_, name="the base query", cache=lhs)
    inner = np.nonzero((base["t"] > 0.0) & (base["t"] < horizon) & (base["d2"] > 0.0))[0]  # t is the unclamped time here
    assert len(inner) >= 40
    rng = np.random.default_rng(19)
    near, near_d2 = pairs(rec, grid, range_)
    d2_of = {(int(p), int(q)): s for (p, q), s in zip(near, near_d2)}
    fell = {True: 0, False: 0}

    def ask(row, d, h, r, what):
        want = agree(a, rec, grid, float(d), float(h), float(r), cache=lhs, capped=False,
                     name=f"pair ({row['a']}, {row['b']}), {what} {float({'distance': d, 'horizon': h, 'range': r}[what]).hex()}")
        fell[bool(((want["a"] == row["a"]) & (want["b"] == row["b"])).any())] += 1
        return want

    for k in rng.choice(inner, 40, replace=False):
        row = base[k]
        root = np.sqrt(row["d2"])
        for d in (np.nextafter(root, 0.0), root, np.nextafter(root, INF)):
            ask(row, d, horizon, range_, "distance")
        for h in (np.nextafter(row["t"], 0.0), row["t"], np.nextafter(row["t"], INF)):
            want = ask(row, distance, h, range_, "horizon")
            mine = want[(want["a"] == row["a"]) & (want["b"] == row["b"])]
            assert len(mine) == 1 and mine["t"][0] == min(h, row["t"])  # clamped below its time, free at and above it
        root = np.sqrt(d2_of[(int(row["a"]), int(row["b"]))])
        for r in (np.nextafter(root, 0.0), root, np.nextafter(root, INF)):
            ask(row, distance, horizon, r, "range")
    print(f"the pair itself was in {fell[True]} times and out {fell[False]} times")
    assert fell[True] >= 40 and fell[False] >= 40
    assert a.read_agents().tobytes() == rec.tobytes()


def _hand_cases(x0, y0):
    """The hand cases of tests/test_encounters_abi.py, each 20 m from the next, from (x0, y0) on -> (rows of (x, y, vx,
    vy), the index pairs that are an encounter of (0.8, 3.0, 4.0) with their (t, m2) where the values are plain)"""
    rows = [(x0, y0, 0.5, 0.0), (x0 + 2.0, y0, -0.5, 0.0),                     # head-on: t 2, m2 0
            (x0, y0 + 20.0, 0.25, 0.125), (x0 + 0.5, y0 + 20.0, 0.25, 0.125),   # equal velocities: t 0, m2 d2
            (x0, y0 + 40.0, -0.5, 0.0), (x0 + 0.5, y0 + 40.0, 0.5, 0.0),        # diverging: t 0, m2 d2
            (x0 + 20.0, y0, 0.5, 0.0), (x0 + 20.0, y0, -0.25, 0.25),            # on one point: t 0, m2 +0
            (x0 + 20.0, y0 + 20.0, 0.0, 0.0), (x0 + 21.0, y0 + 18.0, 0.0, 1.0),  # a perpendicular pass at 1 m: no encounter
            (x0 + 20.0, y0 + 40.0, 0.5, 0.0), (x0 + 20.0, y0 + 40.0, 0.0, 0.5), (x0 + 20.0, y0 + 40.0, -0.5, -0.5)]  # three
    expected = {(0, 1): (2.0, 0.0), (2, 3): (0.0, 0.25), (4, 5): (0.0, 0.25), (6, 7): (0.0, 0.0),
                (10, 11): (0.0, 0.0), (10, 12): (0.0, 0.0), (11, 12): (0.0, 0.0)}
    return rows, expected


def test_written_agents():
    """Positions and velocities written by id: the hand cases, three agents on one point, a cell with more agents than a
    workgroup next to one with 70, and outsiders, which never appear."""
    a, led, _, grid = _scene()
    _advance(a, led, 3)
    rec = a.read_agents()
    assert rec["x"].max() < 120.0 and rec["y"].max() < 120.0  # (the far corner of the 182 m grid is empty)
    rows, expected = _hand_cases(130.0, 128.0)
    w = rec[100:100 + len(rows)].copy()
    for k, (x, y, vx, vy) in enumerate(rows):
        w["x"][k], w["y"][k], w["vx"][k], w["vy"][k] = x, y, vx, vy
    a.write_agents(w, fields=("position", "velocity"))
    rec = a.read_agents()
    ids = [int(i) for i in w["id"]]
    for horizon in (3.0, 1.0):
        want = agree(a, rec, grid, 0.8, horizon, 4.0, name=f"hand cases, horizon {horizon}")
        got = {(int(r["a"]), int(r["b"])): (float(r["t"]), float(r["d2"])) for r in want}
        for (i, j), (t, m2) in expected.items():
            key = tuple(sorted((ids[i], ids[j])))
            if (i, j) == (0, 1) and horizon == 1.0:
                assert key not in got  # (1 m apart at the horizon's end: not closer than 0.8)
            else:
                assert got[key] == (t, m2) and not np.signbit(got[key][1]), (i, j)
        assert tuple(sorted((ids[8], ids[9]))) not in got
    want = agree(a, rec, grid, 1.5, 1.0, 4.0, name="hand cases, head-on clamped")
    assert (1.0, 1.0) in [(float(r["t"]), float(r["d2"])) for r in want if (int(r["a"]), int(r["b"])) == tuple(sorted(ids[:2]))]
    want = agree(a, rec, grid, 1.25, 3.0, 4.0, name="hand cases, the perpendicular pass")
    assert (2.0, 1.0) in [(float(r["t"]), float(r["d2"])) for r in want if (int(r["a"]), int(r["b"])) == tuple(sorted(ids[8:10]))]
    # a cell holding 300 agents with random velocities next to one holding 70
    rng = np.random.default_rng(23)
    cell = grid["cell_size"]
    w = rec[200:570].copy()
    w["x"][:300] = 70 * cell + rng.uniform(0.0, cell, 300)  # cell (70, 71)
    w["y"][:300] = 71 * cell + rng.uniform(0.0, cell, 300)
    w["x"][300:] = 71 * cell + rng.uniform(0.0, cell, 70)   # its diagonal neighbour (71, 72)
    w["y"][300:] = 72 * cell + rng.uniform(0.0, cell, 70)
    w["vx"], w["vy"] = rng.normal(0.0, 1.0, 370), rng.normal(0.0, 1.0, 370)
    a.write_agents(w, fields=("position", "velocity"))
    rec = a.read_agents()
    cx, cy = np.floor(rec["x"] / cell), np.floor(rec["y"] / cell)
    assert int(((cx == 70) & (cy == 71)).sum()) == 300 and int(((cx == 71) & (cy == 72)).sum()) == 70
    counts = []
    for distance, horizon, range_ in ((0.1, 0.5, 1.0), (0.3, 1.0, 2.0), (0.3, 1.0, 5.0), (1.0, 2.0, 5.0)):
        stats = {}
        want = agree(a, rec, grid, distance, horizon, range_, name=f"a full cell, {(distance, horizon, range_)}", stats=stats)
        counts.append(len(want))
        assert all(c >= 5 for c in _classes(want, horizon)) and len(want) < stats["in_range"]
    assert counts[0] > 300 and counts[3] > 300 * 299 // 8 and counts == sorted(counts)
    # outsiders, at least a cell outside and walking in: below the low edge (clamped into row / column 0) and beyond the
    # row stride (aliased into the next row)
    size = grid["width"]
    outside = [(-2.5 * cell, 50.0), (50.0, -1.5 * cell), (-3.0 * cell, -3.0 * cell), (10.0, size + 1.5 * cell),
               (30.0, size + 40.0)]
    out_ids = a.add_agents(outside, StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 2.0)
    led.hear(drain(a))
    inside = rec[:5].copy()  # five of the crowd put 3 m inside of each outsider, walking towards it
    inside["x"] = [0.5, 50.0, 0.5, 10.0, 30.0]
    inside["y"] = [50.0, 0.5, 0.5, size - 1.5, size - 1.0]
    inside["vx"], inside["vy"] = [-1.0, 0.0, -1.0, 0.0, 0.0], [0.0, -1.0, -1.0, 1.0, 1.0]
    a.write_agents(inside, fields=("position", "velocity"))
    rec = a.read_agents()
    part = takes_part(rec, grid)
    assert sorted(rec["id"][~part].tolist()) == sorted(int(i) for i in out_ids)
    m = int(part.sum())
    for distance, horizon, range_ in ((1.0, 5.0, 2.5 * cell), (1.0, 3.0, 6.0 * cell), (INF, 1.0, INF)):
        want = agree(a, rec, grid, distance, horizon, range_, name=f"with outsiders, {(distance, horizon, range_)}",
                     capped=range_ < INF)
        listed = np.concatenate([want["a"], want["b"]])
        assert not np.isin(listed, np.asarray(out_ids, dtype=np.uint64)).any()
    assert a.count_encounters(INF, 1.0, INF) == m * (m - 1) // 2


def test_roles():
    a, led, sinks, grid = _scene(sinks=True)
    _advance(a, led, 40)
    rec = a.read_agents()
    robots_at = rec[np.argsort(np.hypot(rec["x"] - 70.0, rec["y"] - 70.0))[:8]]
    nolp, still = NoLocalPlan(), StubHighLevelPlan((0.0, 0.0))
    robots = a.add_agents(np.stack([robots_at["x"] + 0.21, robots_at["y"] - 0.17], axis=1), still, nolp, 2.0)
    led.hear(drain(a))
    rec = a.read_agents()
    cols = led.columns(rec)
    lp_robots = led._handles(nolp)[0]
    lp_crowd = int(cols[2][0])
    assert lp_crowd != lp_robots
    is_robot = selection(_abi.CS_SEL_LP, lp=lp_robots)
    is_crowd = selection(_abi.CS_SEL_LP, lp=lp_crowd)
    half = selection(_abi.CS_SEL_RECT, x0=-INF, y0=-INF, x1=float(np.median(rec["x"])), y1=INF)
    disc = selection(_abi.CS_SEL_CIRCLE, cx=70.0, cy=70.0, r=12.0)
    slow = selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=1.25)
    nobody = selection(_abi.CS_SEL_LP, lp=12345)
    robot_ids = set(int(i) for i in robots)
    lhs = {}
    for numbers in ((0.5, 3.0, 4.0), (1.5, 1.0, 6.0)):
        def same(sa, sb, name):
            return agree(a, rec, grid, *numbers, sa, sb, cols, f"{name}, {numbers}", cache=lhs)
        # robots against everyone: every row holds a robot, and each robot stands 0.27 m from an agent
        want = same(is_robot, None, "robots x everyone")
        assert len(want) >= 8 and all(int(r["a"]) in robot_ids or int(r["b"]) in robot_ids for r in want)
        flipped = same(None, is_robot, "everyone x robots")
        assert flipped.tobytes() == want.tobytes()
        inside = same(disc, disc, "A == B")                  # the encounters inside the group
        across = same(is_robot, is_crowd, "disjoint")         # only rows across
        assert all((int(r["a"]) in robot_ids) != (int(r["b"]) in robot_ids) for r in across)
        same(half, disc, "overlapping roles")                 # an agent in both roles
        by_speed = same(slow, half, "a speed term")
        assert len(by_speed) <= len(same(None, half, "everyone x half"))
        assert len(same(nobody, None, "A selects nobody")) == 0
        if numbers[0] == 1.5:
            assert len(inside) > 10 and len(across) > 8
    # the Python surface: planner objects, dicts, Selections
    want = agree(a, rec, grid, 0.5, 3.0, 4.0, is_robot, None, cols, "robots x everyone", cache=lhs)
    assert a.encounters(0.5, 3.0, 4.0, Selection(local_planner=nolp)).tobytes() == want.tobytes()
    assert a.encounters(0.5, 3.0, 4.0, None, dict(local_planner=nolp)).tobytes() == want.tobytes()
    assert a.count_encounters(0.5, 3.0, 4.0, dict(local_planner=nolp), Selection()) == len(want)
    assert a.read_agents().tobytes() == rec.tobytes()


def test_degenerate_crowds_and_refusals():
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    a = Simulation(LocationHash2D(**grid))
    assert a.count_encounters(INF, INF, INF) == 0 and a.encounters(1.0, 1.0, 1.0).shape == (0,)  # an empty crowd
    a.add_agents([(3.0, 4.0)], StubHighLevelPlan((0.1, 0.0)), NoLocalPlan(), 2.0)
    assert a.count_encounters(INF, INF, INF) == 0 and a.encounters(INF, 1.0, INF).shape == (0,)  # one agent
    a.add_agents([(3.5, 4.0), (30.0, 30.0)], StubHighLevelPlan((0.1, 0.0)), NoLocalPlan(), 2.0)
    a.step(0.05)
    rec = a.read_agents()
    agree(a, rec, grid, 1.0, 2.0, 3.0, name="three agents")
    assert a.encounters(1.0, 2.0, 3.0)[["a", "b"]].tolist() == [(0, 1)]
    bad_terms = selection(1 << 9)
    bad_radius = selection(_abi.CS_SEL_CIRCLE, cx=1.0, cy=1.0, r=-1.0)
    nan_rect = selection(_abi.CS_SEL_RECT, x0=float("nan"), y0=0.0, x1=1.0, y1=1.0)
    nan = float("nan")
    for name, numbers, sa, sb in (("NaN distance", (nan, 2.0, 3.0), None, None), ("negative distance", (-0.5, 2.0, 3.0), None, None),
                                  ("NaN horizon", (1.0, nan, 3.0), None, None), ("negative horizon", (1.0, -1e-300, 3.0), None, None),
                                  ("NaN range", (1.0, 2.0, nan), None, None), ("negative range", (1.0, 2.0, -3.0), None, None),
                                  ("minus infinity", (1.0, -INF, 3.0), None, None),
                                  ("unknown terms in A", (1.0, 2.0, 3.0), bad_terms, None),
                                  ("a negative radius in B", (1.0, 2.0, 3.0), None, bad_radius),
                                  ("a NaN in A", (1.0, 2.0, 3.0), nan_rect, None)):
        for cap in (None, 4):
            n, out = call(a, *numbers, sa, sb, cap=cap, fill=0xAB)
            assert n == SIZE_MAX and "encounters" in last_error(a), name
            if cap:
                assert (out.view(np.uint8) == 0xAB).all(), name
        assert a.read_agents().tobytes() == rec.tobytes(), name
        assert a.encounters(1.0, 2.0, 3.0)[["a", "b"]].tolist() == [(0, 1)], name
    with pytest.raises(CrowdSimError, match="encounters"):
        a.encounters(1.0, -1.0, 3.0)
    with pytest.raises(CrowdSimError, match="encounters"):
        a.count_encounters(1.0, 2.0, 3.0, dict(circle=(0.0, 0.0, -2.0)))
    assert a.read_agents().tobytes() == rec.tobytes()
    a.step(0.05)
    assert a.encounters(1.0, 2.0, 3.0)[["a", "b"]].tolist() == [(0, 1)]


def test_the_listing_limit():
    """11,586 agents with all three numbers +inf: 67,111,905 encounters are more than CS_PAIRS_MAX, the listing is refused
    and the count-only form is exact."""
    n = 11586
    assert n * (n - 1) // 2 == 67111905 > _abi.CS_PAIRS_MAX
    pts = scenes.jittered_lattice(n, 1.0, (10.0, 10.0), 0.25, 3)
    side = float(np.ceil(pts.max() + 10.0))
    grid = dict(width=side, height=side, cell_size=2.0, offset=(0.0, 0.0))
    b = Simulation(LocationHash2D(**grid))
    b.add_agents(pts, StubHighLevelPlan((0.1, 0.0)), NoLocalPlan(), 2.0)
    b.step(0.05)
    rec = b.read_agents()
    assert takes_part(rec, grid).all()
    count, _ = call(b, INF, INF, INF)
    assert count == 67111905
    count, out = call(b, INF, INF, INF, cap=16, fill=0xAB)
    assert count == SIZE_MAX and "too many encounters to list" in last_error(b)
    assert (out.view(np.uint8) == 0xAB).all()
    with pytest.raises(CrowdSimError, match="too many encounters to list"):
        b.encounters(INF, INF, INF)
    assert b.count_encounters(INF, INF, INF) == 67111905
    assert b.read_agents().tobytes() == rec.tobytes()
    # the engine stays usable: the encounters among the agents of a box (the restatement on those agents alone)
    box = selection(_abi.CS_SEL_RECT, x0=20.0, y0=20.0, x1=50.0, y1=50.0)
    sub = rec[(20.0 <= rec["x"]) & (rec["x"] < 50.0) & (20.0 <= rec["y"]) & (rec["y"] < 50.0)]
    assert 500 < len(sub) < 1500 and len(agree(b, sub, grid, 0.9, 2.0, 1.2, box, box, name="the engine stays usable")) > 100
    b.step(0.05)


def test_wide_ids_by_external_id_across_renumberings(monkeypatch):
    """The recipe of tests/test_gpu_close_pairs.py: 10 x 600 ids through a 4096-id device space.  Rows of ids above 2^32
    come back, ascending, equal to the restatement before and after a renumbering; the call never renumbers."""
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(2 ** 40 + 1))
    monkeypatch.setenv("CS_DEVICE_ID_LIMIT", "4096")
    pts, grid, extent, group = scenes.uniform_crowd(600, seed=9, cell_size=2.0, room=20.0)
    a = Simulation(LocationHash2D(**grid), flags=CS_CFG_WIDE_IDS)
    monkeypatch.delenv("CS_DEVICE_ID_LIMIT")
    monkeypatch.delenv("CS_FIRST_AGENT_ID")
    led = Ledger(a).watch()
    ids = scenes.add_counterflow(a, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    assert min(ids) > 2 ** 40
    spot = np.array([[extent + 15.0, extent + 15.0]])
    still, nolp = StubHighLevelPlan((0.0, 0.0)), NoLocalPlan()

    def check(when):
        rec = a.read_agents()
        cols = led.columns(rec)
        late = selection(_abi.CS_SEL_LP, lp=led._handles(nolp)[0])
        for name, numbers, sa in (("everybody", (1.0, 5.0, 2.5), None), ("the late ones", (0.02, 1.0, 0.025), late),
                                  ("wide", (2.0, 30.0, 5.0), None)):
            want = agree(a, rec, grid, *numbers, sa, None, cols, f"{when}: {name}")
            assert len(want) > 0 and int(min(want["a"].min(), want["b"].min())) > 2 ** 32
            assert (want["a"] < want["b"]).all()

    for r in range(10):
        more = a.add_agents(np.repeat(spot, 600, axis=0) + np.arange(600)[:, None] * 0.01, still, nolp, 1.0)
        a.step(0.05)
        if r in (0, 6, 8):
            n_before = a.kernel_stat(_abi.CS_STAT_RENUMBERINGS)
            check(f"round {r}, {n_before} renumberings")
            assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) == n_before
        a.remove_agents_by_id(more[:-1])
    assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) >= 1
    check("at the end")


@pytest.mark.parametrize("flags", [0, CS_CFG_FORCE_TILED])
def test_twins_one_of_which_asks_between_steps(flags):
    """One twin asks for encounters after every step from 20 to 40, the other never does: the same bytes, events and
    report."""
    twins = [_scene(flags, 4096, sinks=True) for _ in range(2)]
    (a, led_a, _, grid), (b, led_b, _, _) = twins
    for s, led, _, _ in twins:
        _advance(s, led, 20)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    n0 = len(a.encounters(0.8, 2.0, 4.0))
    assert 0 < n0 < a.count_encounters(1.5, 2.0, 4.0)
    _steps((a, b), 1)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    for _ in range(19):
        a.encounters(0.8, 2.0, 4.0)
        a.count_encounters(0.5, 3.0, 4.0, dict(source_sink=0))
        _steps((a, b), 1)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert drain(a) == drain(b)
    assert a.last_report == b.last_report
