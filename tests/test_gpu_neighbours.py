"""The neighbours of each agent on one engine (include/crowdstep_state.h, Simulation.agent_neighbours /
count_agents_with_neighbours): the engine against the numpy restatement of the rules (tests/neighbours_reference.py) applied
to its OWN read_agents().  Equality is exact: the rows, their order, the counts, the nearest id and the bits of nearest_d2;
no case is left out of a comparison and there is no tolerance anywhere ("Neighbours of each agent
between steps")."""
import numpy as np
import pytest

from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, LocationHash2D,
                              NoLocalPlan, Selection, Simulation, StubHighLevelPlan, Zanlungo, _abi, scenes)
from rmf_crowdsim_amd.simulation import NEIGHBOUR_DTYPE
from neighbours_reference import NONE, SIZE_MAX, agent_neighbours, agree, last_error, neighbours, takes_part
from select_reference import Ledger, add_three_sinks, drain, keep_events, selection
from test_gpu_agent_write import _add_crossing, _crossing, _steps

pytestmark = pytest.mark.gpu
FLAGS = [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER]
INF = float("inf")
KEPT_SCRATCH = 16 << 20  # the scratch an engine keeps (include/crowdstep_state.h); a larger one is freed in the call


def _scene(flags=0, n=4096, sinks=True):
    """The crossing crowd (plus the three source-sinks of the selection tests) with the ledger of who owns whom."""
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


@pytest.mark.parametrize("flags", FLAGS)
def test_the_crossing_crowd_equals_the_restatement(flags):
    a, led, sinks, grid = _scene(flags)
    cell = grid["cell_size"]
    for steps, total in ((10, 10), (30, 40)):
        _advance(a, led, steps)
        rec = a.read_agents()
        m = int(takes_part(rec, grid).sum())
        print(f"flags {flags}, after {total} steps: {len(rec)} agents, {m} take part")
        assert m == len(rec) > 4096
        lhs = {}  # (the left-hand sides of this crowd, computed once for all its distances)
        for distance in (0.0, 0.3 * cell, cell, 2.5 * cell):
            want = agree(a, rec, grid, distance, name=f"distance {distance}", cache=lhs)
            isolated, most = int((want["count"] == 0).sum()), int(want["count"].max())
            print(f"  distance {distance}: {len(want)} subjects, {isolated} isolated, the largest count {most}")
            assert len(want) == m
            assert int(want["count"].sum()) == 2 * a.count_close_pairs(distance)
            if distance == 0.0:
                assert isolated == m
            elif distance == 0.3 * cell:
                assert most >= 1
            elif distance == cell:  # (both kinds, by the restatement alone)
                assert 0 < isolated < m
            else:
                assert isolated == 0 and most > 20
        # the Python surface
        want = neighbours(rec, grid, cell, cache=lhs)
        got = a.agent_neighbours(cell)
        assert got.dtype == NEIGHBOUR_DTYPE and got.shape == (m,) and got.tobytes() == want.tobytes()
        assert a.agent_neighbours(cell, limit=5).tobytes() == want[:5].tobytes()
        crowded = want[want["count"] >= 2]
        assert a.agent_neighbours(cell, min_count=2).tobytes() == crowded.tobytes()
        assert a.count_agents_with_neighbours(cell) == int((want["count"] >= 1).sum())
        assert a.count_agents_with_neighbours(cell, min_count=2) == len(crowded)
        assert a.read_agents().tobytes() == rec.tobytes()


def test_roles():
    a, led, sinks, grid = _scene(n=1024)
    _advance(a, led, 20)
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
    slow = selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=1.0)
    nobody = selection(_abi.CS_SEL_LP, lp=12345)
    robot_ids = sorted(int(i) for i in robots)
    lhs = {}
    for distance in (0.5, 2.0, 5.0):
        # robots against everyone: one row per robot, and each robot stands 0.27 m from an agent
        want = agree(a, rec, grid, distance, is_robot, None, cols, f"robots x everyone, {distance}", lhs)
        assert want["id"].tolist() == robot_ids and (want["count"] >= 1).all()
        # robots against the crowd only: no robot is another robot's neighbour
        crowd = agree(a, rec, grid, distance, is_robot, is_crowd, cols, f"robots x crowd, {distance}", lhs)
        assert crowd["id"].tolist() == robot_ids and not np.isin(crowd["nearest"], robots).any()
        assert (crowd["count"] <= want["count"]).all()
        # a rect as subjects against a speed term as others (the velocity column is read)
        agree(a, rec, grid, distance, half, slow, cols, f"a rect x a speed term, {distance}", lhs)
        # overlapping selections: agents that are subject and other do not count themselves
        agree(a, rec, grid, distance, half, disc, cols, f"overlapping selections, {distance}", lhs)
        agree(a, rec, grid, distance, disc, disc, cols, f"subjects == others, {distance}", lhs)
        # subjects that select nobody: no row
        none = agree(a, rec, grid, distance, nobody, None, cols, f"nobody x everyone, {distance}", lhs)
        assert len(none) == 0
        # others that select nobody: every subject is isolated
        alone = agree(a, rec, grid, distance, None, nobody, cols, f"everyone x nobody, {distance}", lhs)
        assert len(alone) == len(rec) and (alone["count"] == 0).all() and (alone["nearest"] == NONE).all()
    # the Python surface: planner objects, dicts, Selections
    want = agree(a, rec, grid, 2.0, is_robot, None, cols, "robots x everyone", lhs)
    assert a.agent_neighbours(2.0, Selection(local_planner=nolp)).tobytes() == want.tobytes()
    assert a.agent_neighbours(2.0, dict(local_planner=nolp), Selection()).tobytes() == want.tobytes()
    assert a.count_agents_with_neighbours(2.0, dict(local_planner=nolp), None) == int((want["count"] >= 1).sum())
    assert a.read_agents().tobytes() == rec.tobytes()


def test_the_nearest_to_the_bit():
    """Distances at sqrt(nearest_d2) of a subject and its two f64 neighbours: the nearest drops out or stays exactly as the
    restatement says (a fused multiply-add or an f32 shortcut would not follow it)."""
    a, led, _, grid = _scene(n=1024, sinks=False)
    _advance(a, led, 25)
    rec = a.read_agents()
    rng = np.random.default_rng(17)
    lhs = {}
    near = neighbours(rec, grid, 6.0, cache=lhs)
    near = near[near["count"] > 0]
    assert len(near) > 400
    fell = {True: 0, False: 0}
    for k in rng.choice(len(near), 40, replace=False):
        subject, root = near[k], np.sqrt(near[k]["nearest_d2"])
        for distance in (np.nextafter(root, 0.0), root, np.nextafter(root, INF)):
            want = agree(a, rec, grid, float(distance), name=f"subject {int(subject['id'])}, distance {float(distance).hex()}",
                         cache=lhs)
            row = want[want["id"] == subject["id"]][0]
            stays = bool(row["nearest"] == subject["nearest"])
            assert stays == bool(row["count"] > 0) and (not stays or row["nearest_d2"] == subject["nearest_d2"])
            fell[stays] += 1
    print(f"the nearest stayed {fell[True]} times and dropped out {fell[False]} times")
    assert fell[True] >= 40 and fell[False] >= 40


def test_ties_coincidences_and_outsiders():
    """Written positions: three agents on one point; one agent at (61, 59) and four on the corners of its cell, all at
    d2 == 2.0, where the smallest of the four ids is the nearest; one agent on the grid's low corner.  Then agents below the
    low edge and beyond the row stride, which are neither subject nor other nor anybody's nearest."""
    a, led, _, grid = _scene(n=1024, sinks=False)
    _advance(a, led, 25)
    rec = a.read_agents()
    cell = grid["cell_size"]
    # the agents closest to (61, 59) are the ones moved: the first five become the centre and the corners, everybody else
    # within 4 m of the centre (and at least three) goes onto one point, the next one onto the grid's low corner
    by_distance = np.argsort(np.hypot(rec["x"] - 61.0, rec["y"] - 59.0), kind="stable")
    crowded = int((np.hypot(rec["x"] - 61.0, rec["y"] - 59.0) < 4.0).sum())
    on_point = max(crowded - 5, 3)
    w = rec[by_distance[:5 + on_point + 1]].copy()
    w["x"][0], w["y"][0] = 61.0, 59.0
    w["x"][1:5] = [60.0, 62.0, 60.0, 62.0]
    w["y"][1:5] = [58.0, 58.0, 60.0, 60.0]
    w["x"][5:5 + on_point], w["y"][5:5 + on_point] = 81.37, 58.21
    w["x"][-1], w["y"][-1] = 0.0, 0.0
    a.write_agents(w, fields=("position",))
    rec = a.read_agents()
    assert takes_part(rec, grid).all()
    centre, corners, point, corner0 = int(w["id"][0]), w["id"][1:5], w["id"][5:5 + on_point], int(w["id"][-1])
    root2 = float(np.sqrt(2.0))
    lhs = {}
    for distance in (1e-9, root2, float(np.nextafter(root2, INF)), 2.5 * cell):
        want = agree(a, rec, grid, distance, name=f"written agents, distance {float(distance).hex()}", cache=lhs)
        row = want[want["id"] == centre][0]
        if distance * distance > 2.0:  # the four corners at exactly 2.0 and nobody closer: the smallest id
            assert row["count"] >= 4 and row["nearest_d2"] == 2.0 and row["nearest"] == corners.min()
        else:
            assert row["count"] == 0 and row["nearest"] == NONE and row["nearest_d2"] == INF
        for i in point:  # on one point: d2 == +0.0 at any distance > 0, the smallest id of the others
            row = want[want["id"] == i][0]
            assert row["count"] >= on_point - 1 and row["nearest_d2"] == 0.0 and not np.signbit(row["nearest_d2"])
            assert row["nearest"] == point[point != i].min()
        assert want[want["id"] == corner0][0]["id"] == corner0  # (on the low corner: a subject)
    assert root2 * root2 > 2.0 or np.nextafter(root2, INF) ** 2 > 2.0
    # outsiders, at least a cell outside: below the low edge (clamped into row / column 0) and beyond the row stride
    # (aliased into the next row)
    size = grid["width"]
    outside = [(-2.5 * cell, 50.0), (50.0, -1.5 * cell), (-3.0 * cell, -3.0 * cell), (10.0, size + 1.5 * cell),
               (30.0, size + 40.0)]
    ids = np.asarray(a.add_agents(outside, StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 2.0), dtype=np.uint64)
    led.hear(drain(a))
    rec = a.read_agents()
    part = takes_part(rec, grid)
    assert sorted(rec["id"][~part].tolist()) == sorted(int(i) for i in ids)
    m = int(part.sum())
    lhs = {}
    for distance in (cell, 2.5 * cell, 4.0 * cell, INF):
        want = agree(a, rec, grid, distance, name=f"with outsiders, distance {distance}", cache=lhs)
        assert len(want) == m and not np.isin(want["id"], ids).any() and not np.isin(want["nearest"], ids).any()
    assert (want["count"] == m - 1).all()  # (+inf: every participant but itself, no outsider)
    # ... nor through a selection that names them, as subjects and as others
    cols = led.columns(rec)
    box = selection(_abi.CS_SEL_RECT, x0=-INF, y0=-INF, x1=INF, y1=INF)
    assert len(agree(a, rec, grid, INF, box, box, cols, "an all-embracing rect", lhs)) == m


def test_all_and_nothing_and_the_scratch_it_leaves():
    """1024 agents, a distance beyond the grid and +inf: every count is 1023.  The device memory the engine holds grows by
    no more than the scratch it documents, also after a crowd whose rows need more than that."""
    a, led, _, grid = _scene(n=1024, sinks=False)
    _advance(a, led, 5)
    rec = a.read_agents()
    assert len(rec) == 1024 and takes_part(rec, grid).all()
    a.select_agents()  # (the selections' group table and the by-id scratch exist from here on: not this call's memory)
    before = a.device_bytes
    lhs = {}
    for distance in (2.0 * grid["width"], INF):
        want = agree(a, rec, grid, distance, name=f"distance {distance}", cache=lhs, min_counts=(0, 1, 3, 1023, 1024))
        assert len(want) == 1024 and (want["count"] == 1023).all()
    after = a.device_bytes
    print(f"cs_device_bytes: {before} before the listings, {after} after")
    assert 0 <= after - before <= KEPT_SCRATCH
    a.agent_neighbours(0.3 * grid["cell_size"], min_count=1)  # a small call after a large one: the kept scratch serves
    assert 0 <= a.device_bytes - before <= KEPT_SCRATCH
    _steps((a,), 2)

    n = 600000  # 72 bytes of scratch per slot: 41 MiB, allocated for the call and freed in it
    pts = scenes.jittered_lattice(n, 1.0, (10.0, 10.0), 0.25, 3)
    side = float(np.ceil(pts.max() + 10.0))
    grid = dict(width=side, height=side, cell_size=2.0, offset=(0.0, 0.0))
    b = Simulation(LocationHash2D(**grid))
    b.add_agents(pts, StubHighLevelPlan((0.1, 0.0)), NoLocalPlan(), 2.0)
    b.step(0.05)
    b.select_agents(limit=1)
    before = b.device_bytes
    count, rows = agent_neighbours(b, 1.2, cap=n + 1, fill=0xAB)
    assert count == n and (rows[n:].view(np.uint8) == 0xAB).all()
    assert (np.diff(rows["id"][:n].astype(np.int64)) > 0).all()
    assert int(rows["count"][:n].sum()) == 2 * b.count_close_pairs(1.2) > 0
    print(f"cs_device_bytes: {before} before the listing of {n} rows, {b.device_bytes} after")
    assert 0 <= b.device_bytes - before <= KEPT_SCRATCH


def test_degenerate_cases_and_refusals():
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    a = Simulation(LocationHash2D(**grid))
    assert a.count_agents_with_neighbours(INF, min_count=0) == 0 and a.agent_neighbours(1.0).shape == (0,)  # an empty crowd
    a.add_agents([(3.0, 4.0)], StubHighLevelPlan((0.1, 0.0)), NoLocalPlan(), 2.0)
    one = a.agent_neighbours(INF)
    assert one.tolist() == [(0, 0, int(NONE), INF)] and a.count_agents_with_neighbours(INF) == 0  # one agent: isolated
    a.add_agents([(3.5, 4.0), (30.0, 30.0)], StubHighLevelPlan((0.1, 0.0)), NoLocalPlan(), 2.0)
    a.step(0.05)
    rec = a.read_agents()
    agree(a, rec, grid, 1.0, name="three agents")
    expected = [(0, 1, 1), (1, 1, 0), (2, 0, int(NONE))]
    assert [(int(r["id"]), int(r["count"]), int(r["nearest"])) for r in a.agent_neighbours(1.0)] == expected
    bad_terms = selection(1 << 9)
    bad_radius = selection(_abi.CS_SEL_CIRCLE, cx=1.0, cy=1.0, r=-1.0)
    nan_rect = selection(_abi.CS_SEL_RECT, x0=float("nan"), y0=0.0, x1=1.0, y1=1.0)
    for name, distance, ss, so in (("NaN distance", float("nan"), None, None), ("negative distance", -1.0, None, None),
                                   ("minus infinity", -INF, None, None), ("unknown terms in the subjects", 1.0, bad_terms, None),
                                   ("a negative radius in the others", 1.0, None, bad_radius),
                                   ("a NaN in the subjects", 1.0, nan_rect, None)):
        for cap in (None, 4):
            n, out = agent_neighbours(a, distance, ss, so, cap=cap, fill=0xAB)
            assert n == SIZE_MAX and "agent_neighbours" in last_error(a), name
            if cap:
                assert (out.view(np.uint8) == 0xAB).all(), name
        assert a.read_agents().tobytes() == rec.tobytes(), name
        a.step(0.05)  # (the engine is usable)
        rec = a.read_agents()
        assert [(int(r["id"]), int(r["count"]), int(r["nearest"])) for r in a.agent_neighbours(1.0)] == expected, name
    with pytest.raises(CrowdSimError, match="agent_neighbours"):
        a.agent_neighbours(-1.0)
    with pytest.raises(CrowdSimError, match="agent_neighbours"):
        a.count_agents_with_neighbours(1.0, dict(circle=(0.0, 0.0, -2.0)))
    with pytest.raises(CrowdSimError, match="min_count"):
        a.agent_neighbours(1.0, min_count=-1)
    assert a.read_agents().tobytes() == rec.tobytes()


def test_wide_ids_rows_by_external_id_across_renumberings(monkeypatch):
    """The recipe of tests/test_gpu_wide_ids.py: 10 x 600 ids through a 4096-id device space.  Rows of ids above 2^32 come
    back, ascending, with external nearest ids, equal to the restatement before and after a renumbering; the call never
    renumbers."""
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
        for name, distance, ss in (("everybody", 1.5, None), ("the late ones", 0.025, late), ("wide", 5.0, None)):
            want = agree(a, rec, grid, distance, ss, None, cols, f"{when}: {name}")
            assert len(want) > 0 and int(want["id"].min()) > 2 ** 32 and (np.diff(want["id"].astype(np.int64)) > 0).all()
            seen = want[want["count"] > 0]
            assert len(seen) > 0 and int(seen["nearest"].min()) > 2 ** 32

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
def test_twins_one_of_which_asks_every_step(flags):
    """One twin asks in all forms after every step for 10 steps, the other never does: the same bytes, events and report."""
    twins = [_scene(flags) for _ in range(2)]
    (a, led_a, _, grid), (b, led_b, _, _) = twins
    for s, led, _, _ in twins:
        _advance(s, led, 20)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    for _ in range(10):
        rows = a.agent_neighbours(2.0)
        assert len(rows) == len(a) and a.count_agents_with_neighbours(2.0) == int((rows["count"] > 0).sum()) > 0
        assert len(a.agent_neighbours(5.0, min_count=3, limit=100)) == 100
        a.count_agents_with_neighbours(0.6, dict(source_sink=0), None, min_count=0)
        _steps((a, b), 1)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert drain(a) == drain(b)
    assert a.last_report == b.last_report
