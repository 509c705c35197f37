"""The clusters of agents under a distance on one engine (include/crowdstep_state.h, Simulation.agent_clusters /
count_clusters): the engine against the restatement of the rules (tests/clusters_reference.py) applied to its OWN
read_agents().  Ids, labels, order, sizes and boxes are compared exactly, the sums under the bound the header states
("Clusters of agents between steps")."""
import ctypes as C

import numpy as np
import pytest

from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, LocationHash2D,
                              NoLocalPlan, Selection, Simulation, StubHighLevelPlan, Zanlungo, _abi, scenes)
from close_pairs_reference import last_error, takes_part
from clusters_reference import agent_clusters, agree, clusters
from select_reference import Ledger, drain, selection
from test_gpu_agent_write import _steps
from test_gpu_close_pairs import _advance, _scene

pytestmark = pytest.mark.gpu
FLAGS = [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER]
INF = float("inf")
KEPT_SCRATCH = 16 << 20  # the scratch an engine keeps (include/crowdstep_state.h); a larger one is freed in the call
STILL = (0.0, 0.0)


def _still_crowd(points, grid, flags=0):
    """agents at rest that no planner moves, added in the order given -> (simulation, their ids)"""
    s = Simulation(LocationHash2D(**grid), flags=flags)
    ids = s.add_agents(np.asarray(points, dtype=np.float64), StubHighLevelPlan(STILL), NoLocalPlan(), 2.0)
    return s, np.asarray(ids, dtype=np.uint64)


@pytest.mark.parametrize("flags", FLAGS)
def test_the_crossing_crowd_equals_the_restatement(flags):
    a, led, sinks, grid = _scene(flags)
    cell = grid["cell_size"]
    for steps, total in ((10, 10), (30, 40)):
        _advance(a, led, steps)
        rec = a.read_agents()
        cols = led.columns(rec)
        speed = np.hypot(rec["vx"].astype(np.float64), rec["vy"].astype(np.float64))
        slow = selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=float(np.median(speed)))
        crowd = selection(_abi.CS_SEL_LP, lp=int(cols[2][0]))
        cache = {}
        for distance in (0.0, 0.3 * cell, cell, 2.5 * cell):
            for who, sel in (("everyone", None), ("the slow half", slow), ("one local planner", crowd)):
                ids, labels, table = agree(a, rec, grid, distance, sel, 1, cols,
                                           f"flags {flags}, {total} steps, distance {distance}, {who}", cache)
                if distance == 0.0:
                    assert (table["size"] == 1).all() and len(table) == len(ids)
                if distance == 0.3 * cell and sel is None:  # (by the restatement alone)
                    assert int((table["size"] >= 2).sum()) > 1 and len(table) > 1
        # the Python surface
        want = clusters(rec, grid, cell, None, 2, cache)
        ids, labels, table = a.agent_clusters(cell, min_size=2)
        assert ids.dtype == labels.dtype == np.uint64 and ids.tolist() == want[0].tolist()
        assert labels.tolist() == want[1].tolist() and table["label"].tolist() == want[2]["label"].tolist()
        assert table["size"].tolist() == want[2]["size"].tolist() and table.dtype.names == want[2].dtype.names
        assert a.count_clusters(cell, min_size=2) == (len(want[2]), len(want[0]))
        few = a.agent_clusters(cell, min_size=2, limit=3)
        assert few[0].tolist() == want[0][:3].tolist() and few[2]["label"].tolist() == want[2]["label"][:3].tolist()
        assert a.read_agents().tobytes() == rec.tobytes()


def _serpentine(n, spacing=0.5, row=48.0, rows_apart=3.0, start=(2.25, 2.25)):
    """n points `spacing` apart (along the path) on a boustrophedon path: rows of `row` metres, `rows_apart` apart"""
    pts = []
    period = row + rows_apart
    for k in range(n):
        s = k * spacing
        r, t = int(s // period), s % period
        along = min(t, row)
        x = start[0] + (along if r % 2 == 0 else row - along)
        y = start[1] + r * rows_apart + max(t - row, 0.0)
        pts.append((x, y))
    return np.array(pts)


def test_a_serpentine_chain_is_one_cluster():
    """3,000 agents 0.5 m apart along a path that folds back every 48 m, rows 3 m apart, on 2 m cells, added in shuffled
    order: slot order, id order and path order are unrelated, the smallest id sits mid-chain, and the chain runs through
    a dozen workgroups and hundreds of cells.  One cluster at 0.6 m; two after one agent is removed."""
    n = 3000
    path = _serpentine(n)
    grid = dict(width=100.0, height=100.0, cell_size=2.0, offset=(0.0, 0.0))
    assert path.max() < 98.0
    rng = np.random.default_rng(31)
    at = rng.permutation(n)  # agent k (in order of ids) stands at path position at[k]
    at[np.nonzero(at == n // 2)[0][0]], at[0] = at[0], n // 2
    a, ids = _still_crowd(path[at], grid)
    assert len(ids) == n and ids[0] == ids.min() and at[0] == n // 2
    rec = a.read_agents()
    got_ids, labels, table = agree(a, rec, grid, 0.6, name="the chain")
    assert len(table) == 1 and int(table["size"][0]) == n and int(table["label"][0]) == int(ids.min())
    assert (labels == ids.min()).all() and got_ids.tolist() == sorted(ids.tolist())
    _, _, table = agree(a, rec, grid, 0.45, name="below the spacing")
    assert len(table) == n
    cut = 1000  # the path position of the agent that leaves
    a.remove_agents_by_id([int(ids[np.nonzero(at == cut)[0][0]])])
    rec = a.read_agents()
    assert len(rec) == n - 1
    _, labels, table = agree(a, rec, grid, 0.6, name="the chain cut")
    assert sorted(int(v) for v in table["size"]) == [cut, n - 1 - cut] == [1000, 1999]
    low = ids[np.isin(at, np.arange(cut))].min()  # the labels: the smallest id on either side of the cut
    high = ids[np.isin(at, np.arange(cut + 1, n))].min()
    assert sorted(int(v) for v in table["label"]) == sorted([int(low), int(high)])
    assert int(table["size"][table["label"] == high][0]) == n - 1 - cut
    a.step(0.05)


def test_a_bridge_to_the_bit():
    """Two 8 x 8 lattices of spacing 0.3 whose closest pair, one corner each, is about 1.0 apart, every other pair across
    at least 1.25: the lattices are one cluster iff that pair is linked, which the three distances around sqrt(d2) decide
    to the bit."""
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    k = np.arange(8) * 0.3
    left = np.stack(np.meshgrid(10.05 + k, 10.1 + k, indexing="ij"), axis=-1).reshape(-1, 2)
    right = np.stack(np.meshgrid(10.05 + 2.1 + 0.8 + k, 10.1 + 2.1 + 0.6 + k, indexing="ij"), axis=-1).reshape(-1, 2)
    a, ids = _still_crowd(np.full((128, 2), 20.0) + np.arange(128)[:, None] * 0.01, grid)
    w = a.read_agents()
    w = w[np.argsort(w["id"])]
    w["x"], w["y"] = np.concatenate([left[:, 0], right[:, 0]]), np.concatenate([left[:, 1], right[:, 1]])
    a.write_agents(w, fields=("position",))
    rec = a.read_agents()
    rec = rec[np.argsort(rec["id"])]
    p, q = rec[63], rec[64]  # the upper corner of the left lattice, the lower corner of the right one
    dx, dy = np.float64(p["x"]) - np.float64(q["x"]), np.float64(p["y"]) - np.float64(q["y"])
    d2 = dx * dx + dy * dy
    root = np.sqrt(d2)
    assert 0.99 < root < 1.01
    outcomes = []
    for distance in (np.nextafter(root, 0.0), root, np.nextafter(root, INF)):
        _, _, table = agree(a, rec, grid, float(distance), name=f"distance {float(distance).hex()}")
        outcomes.append(table["size"].tolist())
    print(f"d2 = {float(d2).hex()}: {outcomes}")
    assert [128] in outcomes and [64, 64] in outcomes and all(o in ([128], [64, 64]) for o in outcomes)


def test_agents_that_are_no_members_do_not_bridge():
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    a = Simulation(LocationHash2D(**grid))
    led = Ledger(a).watch()
    still, lp_ac, lp_b = StubHighLevelPlan(STILL), NoLocalPlan(), NoLocalPlan()
    # A - B - C in a row, 0.5 apart; B belongs to another local planner
    ac = a.add_agents([(7.0, 9.0), (8.0, 9.0)], still, lp_ac, 2.0)
    b = a.add_agents([(7.5, 9.0)], still, lp_b, 2.0)
    led.hear(drain(a))
    rec = a.read_agents()
    cols = led.columns(rec)
    handle = led._handles(lp_ac)[0]
    assert handle != led._handles(lp_b)[0]
    only_ac = selection(_abi.CS_SEL_LP, lp=handle)
    _, labels, table = agree(a, rec, grid, 0.6, None, 1, cols, "everyone")
    assert table["size"].tolist() == [3] and int(table["label"][0]) == min(int(i) for i in list(ac) + list(b))
    ids, labels, table = agree(a, rec, grid, 0.6, only_ac, 1, cols, "B of another planner")
    assert ids.tolist() == sorted(int(i) for i in ac) and table["size"].tolist() == [1, 1]
    assert labels.tolist() == ids.tolist()
    got = a.agent_clusters(0.6, Selection(local_planner=lp_ac))
    assert got[0].tolist() == ids.tolist() and got[1].tolist() == labels.tolist()
    # the same row along the low edge, B written just below it: it takes no part and bridges nobody
    w = rec[np.argsort(rec["id"])].copy()
    order = [int(ac[0]), int(b[0]), int(ac[1])]
    for agent, (x, y) in zip(order, ((0.1, 5.0), (-0.1, 5.45), (0.1, 5.9))):
        w["x"][w["id"] == agent], w["y"][w["id"] == agent] = x, y
    a.write_agents(w, fields=("position",))
    rec = a.read_agents()
    assert sorted(rec["id"][~takes_part(rec, grid)].tolist()) == [int(b[0])]
    ids, labels, table = agree(a, rec, grid, 0.6, name="B below the low edge")
    assert ids.tolist() == sorted(int(i) for i in ac) and table["size"].tolist() == [1, 1]
    w["x"][w["id"] == int(b[0])] = 0.0  # (on the edge it is a member again and bridges)
    a.write_agents(w, fields=("position",))
    rec = a.read_agents()
    _, _, table = agree(a, rec, grid, 0.6, name="B on the low edge")
    assert table["size"].tolist() == [3]


def test_min_size_caps_and_ids_without_labels():
    a, led, _, grid = _scene(n=1024, sinks=False)
    _advance(a, led, 20)
    rec = a.read_agents()
    cache = {}
    for distance in (0.5, 1.0, 1.5, 2.0):  # the first with a cluster of 8 and a cluster of 1, by the restatement alone
        sizes = clusters(rec, grid, distance, cache=cache)[2]["size"]
        if int(sizes.max()) >= 8 and int((sizes == 1).sum()) > 0:
            break
    every = agree(a, rec, grid, distance, None, 0, name="min_size 0", cache=cache)  # (agree also caps at half the counts)
    one = agree(a, rec, grid, distance, None, 1, name="min_size 1", cache=cache)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(every, one)) and len(one[0]) == len(rec)
    sizes = one[2]["size"]
    assert int(sizes.max()) >= 8 and int((sizes == 1).sum()) > 0
    for min_size in (2, 8):
        ids, labels, table = agree(a, rec, grid, distance, None, min_size, name=f"min_size {min_size}", cache=cache)
        assert len(table) == int((sizes >= min_size).sum()) > 0 and len(ids) == int(sizes[sizes >= min_size].sum())
    none = agree(a, rec, grid, distance, None, 10 ** 6, name="nothing that large", cache=cache)
    assert len(none[0]) == 0 and len(none[2]) == 0
    # out_ids without out_labels; counts that are NULL; every output NULL
    ids, labels, table = one
    rc, na, nc, g_ids, g_lab, _ = agent_clusters(a, distance, None, 1, agent_cap=len(ids), fill=0xAB, labels=False)
    assert rc == 0 and (na, nc) == (len(ids), len(table)) and np.array_equal(g_ids[:na], ids)
    assert (g_lab.view(np.uint8) == 0xAB).all() and (g_ids[na:].view(np.uint8) == 0xAB).all()
    rc, _, _, g_ids, g_lab, g_tab = agent_clusters(a, distance, None, 1, len(ids), len(table), counts=False)
    assert rc == 0 and np.array_equal(g_ids[:len(ids)], ids) and np.array_equal(g_lab[:len(ids)], labels)
    assert g_tab["label"][:len(table)].tolist() == table["label"].tolist()
    assert agent_clusters(a, distance, None, 1, counts=False)[0] == 0
    assert a.read_agents().tobytes() == rec.tobytes()


def test_refusals_write_nothing_and_leave_the_engine_usable():
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    a = Simulation(LocationHash2D(**grid))
    assert a.count_clusters(INF) == (0, 0) and a.agent_clusters(1.0)[2].shape == (0,)  # an empty crowd
    a.add_agents([(3.0, 4.0), (3.5, 4.0), (30.0, 30.0)], StubHighLevelPlan((0.1, 0.0)), NoLocalPlan(), 2.0)
    a.step(0.05)
    rec = a.read_agents()
    agree(a, rec, grid, 1.0, name="three agents")
    assert a.agent_clusters(1.0)[1].tolist() == [0, 0, 2]
    bad_terms = selection(1 << 9)
    bad_radius = selection(_abi.CS_SEL_CIRCLE, cx=1.0, cy=1.0, r=-1.0)
    nan_rect = selection(_abi.CS_SEL_RECT, x0=float("nan"), y0=0.0, x1=1.0, y1=1.0)
    for name, distance, sel in (("NaN distance", float("nan"), None), ("negative distance", -0.5, None),
                                ("minus infinity", -INF, None), ("unknown terms", 1.0, bad_terms),
                                ("a negative radius", 1.0, bad_radius), ("a NaN in the selection", 1.0, nan_rect)):
        for caps in ((None, None), (4, 4)):
            rc, na, nc, ids, lab, tab = agent_clusters(a, distance, sel, 1, *caps, fill=0xAB)
            assert rc == 3 and "agent_clusters" in last_error(a), name
            assert na == nc == 2 ** 62, name  # (the counts are not written either)
            if caps[0]:
                assert all((arr.view(np.uint8) == 0xAB).all() for arr in (ids, lab, tab)), name
        assert a.read_agents().tobytes() == rec.tobytes(), name
        assert a.agent_clusters(1.0)[1].tolist() == [0, 0, 2], name
    # out_labels without out_ids
    lab = np.full(4, 7, dtype=np.uint64)
    n = C.c_size_t(99)
    rc = a._lib.cs_agent_clusters(a._engine, 1.0, None, 1, None, lab.ctypes.data_as(C.POINTER(C.c_uint64)), 4, C.byref(n),
                                  None, 0, None)
    assert rc == 3 and "out_labels" in last_error(a) and (lab == 7).all() and n.value == 99
    with pytest.raises(CrowdSimError, match="agent_clusters"):
        a.agent_clusters(-1.0)
    with pytest.raises(CrowdSimError, match="agent_clusters"):
        a.count_clusters(1.0, dict(circle=(0.0, 0.0, -2.0)))
    assert a.read_agents().tobytes() == rec.tobytes()
    a.step(0.05)
    assert a.agent_clusters(1.0)[1].tolist() == [0, 0, 2]


def test_wide_ids_label_by_external_id_across_renumberings(monkeypatch):
    """The recipe of tests/test_gpu_wide_ids.py: 10 x 600 ids through a 4096-id device space.  Ids and labels above 2^32
    come back, equal to the restatement on read_agents() before and after a renumbering; the call never renumbers."""
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(2 ** 40 + 1))
    monkeypatch.setenv("CS_DEVICE_ID_LIMIT", "4096")
    pts, grid, extent, group = scenes.uniform_crowd(600, seed=9, cell_size=2.0, room=20.0)
    a = Simulation(LocationHash2D(**grid), flags=CS_CFG_WIDE_IDS)
    monkeypatch.delenv("CS_DEVICE_ID_LIMIT")
    monkeypatch.delenv("CS_FIRST_AGENT_ID")
    ids = scenes.add_counterflow(a, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    assert min(ids) > 2 ** 40
    spot = np.array([[extent + 15.0, extent + 15.0]])
    still, nolp = StubHighLevelPlan(STILL), NoLocalPlan()

    def check(when):
        rec = a.read_agents()
        for distance in (0.025, 1.5):
            got, labels, table = agree(a, rec, grid, distance, name=f"{when}: distance {distance}")
            assert int(got.min()) > 2 ** 32 and int(labels.min()) > 2 ** 32 and int(table["label"].min()) > 2 ** 32
            assert (distance < 1.0 or int(table["size"].max()) > 1) and np.isin(labels, rec["id"]).all()

    for r in range(10):
        more = a.add_agents(np.repeat(spot, 600, axis=0) + np.arange(600)[:, None] * 0.01, still, nolp, 1.0)
        a.step(0.05)
        if r in (0, 8):
            n_before = a.kernel_stat(_abi.CS_STAT_RENUMBERINGS)
            check(f"round {r}, {n_before} renumberings")
            assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) == n_before
        a.remove_agents_by_id(more[:-1])
    assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) >= 1
    check("at the end")


@pytest.mark.parametrize("flags", [0, CS_CFG_FORCE_TILED])
def test_twins_one_of_which_clusters_between_steps(flags):
    """One twin calls agent_clusters between steps 20 and 21 and again after every step to 30, the other never does: the
    same bytes at 21 and at 30, and the same events."""
    twins = [_scene(flags) for _ in range(2)]
    (a, led_a, _, grid), (b, led_b, _, _) = twins
    for s, led, _, _ in twins:
        _advance(s, led, 20)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert len(a.agent_clusters(2.0)[2]) > 1 and a.count_clusters(5.0, min_size=2)[0] > 0
    _steps((a, b), 1)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    for _ in range(9):
        a.agent_clusters(2.0, min_size=2)
        a.count_clusters(0.6, dict(source_sink=0))
        _steps((a, b), 1)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert drain(a) == drain(b)
    assert a.last_report == b.last_report


def test_the_scratch_the_call_leaves():
    a, led, _, grid = _scene(n=1024, sinks=False)
    _advance(a, led, 5)
    a.select_agents()  # (the selections' group table and the by-id scratch exist from here on: not the clusters' memory)
    before = a.device_bytes
    for distance in (0.0, 1.0, INF):
        ids, labels, table = a.agent_clusters(distance)
        assert len(ids) == 1024
    assert len(table) == 1
    after = a.device_bytes
    print(f"cs_device_bytes: {before} before the calls, {after} after")
    assert 0 <= after - before <= KEPT_SCRATCH
    a.close_pairs(1.0)  # the pairs share the kept scratch
    assert 0 <= a.device_bytes - before <= KEPT_SCRATCH
    _steps((a,), 2)
