"""Selecting, counting and removing agents by region, owner and state on one engine (include/crowdstep_state.h,
Simulation.select_agents / count_agents / remove_selected): the engine against the numpy restatement of the rules
(tests/select_reference.py) applied to its OWN read_agents().  Equality is exact, ids and order; no case is left out of a
comparison and there is no tolerance anywhere ("Selecting agents between steps")."""
import ctypes as C

import numpy as np
import pytest

from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, LocationHash2D,
                              NoLocalPlan, Selection, Simulation, StubHighLevelPlan, Zanlungo, _abi, scenes)
from select_reference import (NO_SINK, Ledger, add_three_sinks, count, drain, keep_events, pred, select, selection,
                              selections_for)
from test_gpu_agent_write import _add_crossing, _crossing, _steps
from test_gpu_agents_by_id import _Leader, _sink_scene

pytestmark = pytest.mark.gpu
FLAGS = [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER]
SIZE_MAX = C.c_size_t(-1).value


def _scene(flags, twins=1):
    """Twins of the 4096-agent crossing crowd plus three source-sinks, each with the ledger of who owns whom."""
    pts, pref, group, grid, extent = _crossing(4096)
    sims, ledgers, sinks = [], [], None
    for _ in range(twins):
        s = Simulation(LocationHash2D(**grid), flags=flags)
        ledgers.append(Ledger(s).watch())
        keep_events(s)
        _add_crossing(s, pts, group)
        sinks = add_three_sinks(s, extent)
        sims.append(s)
    return sims, ledgers, sinks, grid


def _advance(sims, ledgers, k):
    for s, led in zip(sims, ledgers):
        for _ in range(k):
            s.step(0.05)
        led.hear(drain(s))


def _agree(sim, led, sel, rec, name):
    """The engine's answer to `sel` equals the restatement on `rec` (its own read_agents()); returns the ids."""
    want = led.expected(sel, rec)
    n, got = select(sim, sel)
    print(f"  {name}: restatement {len(want)}, engine {n}")
    assert n == len(want), name
    assert got.tolist() == want.tolist(), name
    return want


@pytest.mark.parametrize("flags", FLAGS)
def test_every_term_every_pair_and_all_seven_equal_the_restatement(flags):
    (a,), (led,), sinks, _ = _scene(flags)
    for steps, total in ((10, 10), (30, 40)):
        _advance((a,), (led,), steps)
        rec = a.read_agents()
        owner, _, _ = led.columns(rec)
        print(f"flags {flags}, after {total} steps: {len(rec)} agents, {int((owner != NO_SINK).sum())} spawned, "
              f"waypoints {sorted(set(rec['next_waypoint'].tolist()))}")
        sels = selections_for(rec, led, sinks)
        lengths = []
        for name, sel in sels:
            want = _agree(a, led, sel, rec, name)
            lengths.append(len(want))
            assert a._lib.cs_select_agents(a._engine, C.byref(sel), None, 0) == len(want), name  # the count only
            if len(want) > 3:  # a cap below the count: the full count and the first `cap` ids
                cap = len(want) // 2
                n, few = select(a, sel, cap=cap)
                assert n == len(want) and few.tolist() == want[:cap].tolist(), name
        by_name = dict(zip([n for n, _ in sels], lengths))
        assert by_name["none"] == len(rec)
        for term in (1, 2, 4, 8, 16, 32, 64):  # (every term alone selects somebody, and not everybody)
            assert 0 < by_name[f"term {term}"] < len(rec), term
        for name in ("x1 <= x0", "wp_hi < wp_lo", "unknown sink", "unknown hlp", "unknown lp", "r == 0"):
            assert by_name[name] == 0, name
        if total == 40:
            assert int((owner != NO_SINK).sum()) >= 24 and by_name["all seven"] > 0
            assert all(by_name[f"sink {h}"] > 0 for h in sinks) and by_name["waypoint 1..2"] > 0
        only = [s for _, s in sels]
        rc, counts = count(a, only)
        assert rc == 0 and counts.tolist() == lengths
        padded = [only[k % len(only)] for k in range(1024)]  # the same again with the list padded to the limit
        rc, counts = count(a, padded)
        assert rc == 0 and counts.tolist() == [lengths[k % len(only)] for k in range(1024)]
        rc, _ = count(a, padded + only[:1])
        assert rc == 3 and "count_agents" in a._lib.cs_last_error(a._engine).decode()
        # the Python surface: keywords, a Selection, dicts
        x0, y0, x1, y1 = (getattr(only[1], f) for f in ("x0", "y0", "x1", "y1"))
        ids = a.select_agents(rect=(x0, y0, x1, y1))
        assert ids.dtype == np.uint64 and ids.tolist() == led.expected(only[1], rec).tolist()
        assert a.select_agents(Selection(rect=(x0, y0, x1, y1)), limit=5).tolist() == ids[:5].tolist()
        assert a.read_agents_by_id(ids)["id"].tolist() == ids.tolist()  # (ready for the by-id calls)
        got = a.count_agents([Selection(), dict(rect=(x0, y0, x1, y1)), Selection(source_sink=sinks[0])])
        assert got.tolist() == [len(rec), len(ids), by_name[f"sink {sinks[0]}"]]
        assert a.read_agents().tobytes() == rec.tobytes()


def test_edges_to_the_bit():
    """Bounds that ARE read-back coordinates, radii and speeds at an agent's own value and its two f64 neighbours, agents
    written onto cell corners and the grid's low edge: the engine and the restatement agree on every one, whichever way
    each case falls (a fused multiply-add or an f32 shortcut would not)."""
    (a,), (led,), sinks, grid = _scene(0)
    _advance((a,), (led,), 25)
    rec = a.read_agents()
    rng = np.random.default_rng(41)
    inf = float("inf")
    n_cases = 0
    # 1. rectangles whose edges are coordinates of chosen agents: in at the low edge, out at the high edge
    for _ in range(40):
        i, j = rng.choice(len(rec), 2, replace=False)
        lo, hi = (i, j) if rec["x"][i] <= rec["x"][j] else (j, i)
        sel = selection(_abi.CS_SEL_RECT, x0=float(rec["x"][lo]), x1=float(rec["x"][hi]), y0=-inf, y1=inf)
        got = _agree(a, led, sel, rec, f"x edges at agents {rec['id'][lo]}, {rec['id'][hi]}")
        if rec["x"][lo] < rec["x"][hi]:
            assert rec["id"][lo] in got and rec["id"][hi] not in got
        lo, hi = (i, j) if rec["y"][i] <= rec["y"][j] else (j, i)
        sel = selection(_abi.CS_SEL_RECT, y0=float(rec["y"][lo]), y1=float(rec["y"][hi]), x0=-inf, x1=inf)
        got = _agree(a, led, sel, rec, f"y edges at agents {rec['id'][lo]}, {rec['id'][hi]}")
        if rec["y"][lo] < rec["y"][hi]:
            assert rec["id"][lo] in got and rec["id"][hi] not in got
        n_cases += 2
    # 2. circles of radius sqrt(d2) and its two neighbours, d2 an agent's squared distance by the rule's own expression
    for _ in range(60):
        k = int(rng.integers(len(rec)))
        cx, cy = (float(v) for v in rng.uniform(40.0, 160.0, 2))
        dx, dy = rec["x"][k] - np.float64(cx), rec["y"][k] - np.float64(cy)
        r = float(np.sqrt(dx * dx + dy * dy))
        for radius in (np.nextafter(r, 0.0), r, np.nextafter(r, inf)):
            _agree(a, led, selection(_abi.CS_SEL_CIRCLE, cx=cx, cy=cy, r=float(radius)), rec,
                   f"circle through agent {rec['id'][k]}, r = {float(radius).hex()}")
            n_cases += 1
    # 3. speed bounds at an agent's own speed and its two neighbours, as the lower and as the upper bound
    for _ in range(40):
        k = int(rng.integers(len(rec)))
        s = float(np.sqrt(rec["vx"][k] * rec["vx"][k] + rec["vy"][k] * rec["vy"][k]))
        for bound in (np.nextafter(s, 0.0), s, np.nextafter(s, inf)):
            _agree(a, led, selection(_abi.CS_SEL_SPEED, speed_lo=float(bound), speed_hi=inf), rec,
                   f"speed from agent {rec['id'][k]}'s, {float(bound).hex()}")
            _agree(a, led, selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=float(bound)), rec,
                   f"speed up to agent {rec['id'][k]}'s, {float(bound).hex()}")
            n_cases += 2
    # 4. agents written onto cell corners, cell edges and the grid's low edge
    cell = grid["cell_size"]
    spots = [(0.0, 0.0), (0.0, 7.3), (9.1, 0.0), (cell * 30, cell * 41), (cell * 30, cell * 41 + 0.5), (cell * 17 + 1.0, cell * 9),
             (np.nextafter(cell * 50, 0.0), cell * 50), (cell * 50, np.nextafter(cell * 50, inf)), (cell, cell)]
    rows = rec[rng.choice(len(rec), len(spots), replace=False)].copy()
    rows["x"], rows["y"] = [p[0] for p in spots], [p[1] for p in spots]
    a.write_agents(rows, "position")
    rec = a.read_agents()
    placed = rec[np.isin(rec["id"], rows["id"])]
    for row in placed:
        x, y = float(row["x"]), float(row["y"])
        for sel, name in (
                (selection(_abi.CS_SEL_RECT, x0=x, y0=y, x1=x + cell, y1=y + cell), "the cell from the corner"),
                (selection(_abi.CS_SEL_RECT, x0=x - cell, y0=y - cell, x1=x, y1=y), "the cell up to the corner"),
                (selection(_abi.CS_SEL_RECT, x0=-inf, y0=-inf, x1=np.nextafter(x, inf), y1=np.nextafter(y, inf)), "just in"),
                (selection(_abi.CS_SEL_RECT, x0=np.nextafter(x, inf), y0=-inf, x1=inf, y1=inf), "just out"),
                (selection(_abi.CS_SEL_CIRCLE, cx=x, cy=y, r=0.0), "a zero circle on the agent"),
                (selection(_abi.CS_SEL_CIRCLE, cx=x, cy=y, r=5e-324), "the smallest circle on the agent"),
                (selection(_abi.CS_SEL_CIRCLE, cx=x, cy=y, r=1e-160), "a circle whose r*r is above zero")):
            got = _agree(a, led, sel, rec, f"agent {row['id']} at ({x.hex()}, {y.hex()}): {name}")
            if name in ("the cell from the corner", "just in", "a circle whose r*r is above zero"):
                assert row["id"] in got, name
            if name in ("the cell up to the corner", "just out", "a zero circle on the agent"):
                assert row["id"] not in got, name
            n_cases += 1
    assert len(placed) == len(spots)  # (read back through the f32 offset: a written 100 - 1 ulp is stored as 100 in cell 49)
    print(f"{n_cases} edge cases compared")


@pytest.mark.parametrize("flags", FLAGS)
def test_owners_are_those_of_the_spawned_events_also_after_the_sink_is_removed(flags):
    (a,), (led,), sinks, _ = _scene(flags)
    _advance((a,), (led,), 40)

    def check():
        rec = a.read_agents()
        owner, _, _ = led.columns(rec)
        found = {}
        for h in list(sinks) + [NO_SINK]:
            n, got = select(a, selection(_abi.CS_SEL_SOURCE_SINK, source_sink=int(h)))
            assert n == len(got) and got.tolist() == rec["id"][owner == h].tolist(), h
            found[h] = len(got)
        assert sum(found.values()) == len(rec)
        return found
    before = check()
    assert all(before[h] >= 5 for h in sinks) and before[NO_SINK] == 4096
    a.remove_source_sink(sinks[1])  # (the default: its crowd walks on, and is still found by its owner)
    assert check() == before
    _advance((a,), (led,), 15)
    after = check()
    assert after[sinks[1]] == before[sinks[1]] and after[sinks[0]] > before[sinks[0]]  # (the others keep spawning)


@pytest.mark.parametrize("flags", FLAGS)
def test_selections_and_counts_between_steps_disturb_nothing(flags):
    (a, b), ledgers, sinks, _ = _scene(flags, twins=2)
    led = ledgers[0]
    _advance((a, b), ledgers, 10)
    rec = a.read_agents()
    sels = [s for _, s in selections_for(rec, led, sinks)]
    for k in range(20):
        a.step(0.05)
        b.step(0.05)
        n, _ = select(a, sels[k % len(sels)])
        assert n != SIZE_MAX
        rc, _ = count(a, sels)
        assert rc == 0
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert drain(a) == drain(b)
    kept = [s.kernel_stat(_abi.CS_STAT_STEPS_ON_KEPT_WINDOWS) for s in (a, b)]
    print(f"flags {flags}: steps on kept windows {kept}")
    assert kept[0] == kept[1]


def test_selections_between_steps_keep_the_kept_windows(monkeypatch):
    """The set-up of tests/test_gpu_agents_by_id.py::test_reads_between_steps_keep_the_kept_windows: a small crowd steps on
    band windows cut one step earlier; a selection and a count between two steps leave them valid."""
    monkeypatch.setenv("CS_WINDOWS_KEEP", "1")
    pts, grid, extent, group = scenes.uniform_crowd(6000, seed=4, cell_size=2.0, margin=30.0)
    sims = [Simulation(LocationHash2D(**grid), flags=CS_CFG_FORCE_TILED) for _ in range(2)]
    for s in sims:
        scenes.add_counterflow(s, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    a, b = sims
    mid = float(np.median(pts[:, 0]))
    for k in range(12):
        a.step(0.05)
        b.step(0.05)
        ids = a.select_agents(rect=(mid - 10.0, -1e9, mid + 10.0 + k, 1e9), speed=(0.0, 5.0))
        assert 0 < len(ids) < 6000
        assert a.count_agents([Selection(), Selection(circle=(mid, mid, 15.0))])[0] == 6000
    kept = [s.kernel_stat(_abi.CS_STAT_STEPS_ON_KEPT_WINDOWS) for s in sims]
    print(f"steps on kept windows: selected {kept[0]}, untouched {kept[1]}")
    assert kept[0] == kept[1] and kept[1] > 0
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


@pytest.mark.parametrize("flags", FLAGS)
def test_remove_selected_equals_remove_by_id_of_the_selection(flags):
    """Events, callback planner calls and state: remove_selected(sel) on one twin, remove_agents_by_id(select_agents(sel))
    on the other; then remove_source_sink(h, with_agents=True) against the same spelled out."""
    grid = dict(width=60.0, height=60.0, cell_size=2.0, offset=(0.0, 0.0))
    sims, leaders = [], []
    for _ in range(2):
        s = Simulation(LocationHash2D(**grid), flags=flags)
        leader = _Leader()
        _sink_scene(s, leader)
        keep_events(s)
        sims.append(s)
        leaders.append(leader)
    a, b = sims
    _steps((a, b), 25)
    assert drain(a) == drain(b)  # (the spawns so far)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    box = dict(rect=(0.0, 0.0, 26.0, 60.0))  # half of the walkers, some of the leader's group, the spawned agents
    want = b.select_agents(**box)
    gone = a.remove_selected(**box)
    assert b.remove_agents_by_id(want) == len(want)
    assert gone.dtype == np.uint64 and gone.tolist() == want.tolist() and len(gone) > 100
    ra = a.read_agents()
    assert ra.tobytes() == b.read_agents().tobytes() and not np.isin(gone, ra["id"]).any()
    ev = drain(a)
    assert ev == drain(b) and [e[2] for e in ev] == gone.tolist() and {e[0] for e in ev} == {_abi.CS_EVENT_DESTROYED}
    assert {e[1] for e in ev} == {0, 0xFFFFFFFF}  # (spawned agents name their sink)
    assert leaders[0].removed == leaders[1].removed and len(leaders[0].removed) > 0
    assert len(a.select_agents(**box)) == 0
    _steps((a, b), 10)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert drain(a) == drain(b)
    # the sink with its crowd
    crowd = b.select_agents(source_sink=0)
    assert len(crowd) >= 1
    a.remove_source_sink(0, with_agents=True)
    b.remove_agents_by_id(crowd)
    b.remove_source_sink(0)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    ev = drain(a)
    assert ev == drain(b) and ev == [(_abi.CS_EVENT_DESTROYED, 0, int(i)) for i in crowd]
    _steps((a, b), 10)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert len(a.select_agents(source_sink=0)) == 0 and a.last_report["n_spawned"] == 0
    assert drain(a) == drain(b)
    assert leaders[0].removed == leaders[1].removed


def test_wide_ids_select_by_external_id_across_renumberings(monkeypatch):
    """The recipe of tests/test_gpu_wide_ids.py: 10 x 600 ids through a 4096-id device space.  Ids above 2^32 come back,
    ascending, equal to the restatement before and after a renumbering; a selection never renumbers."""
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
        mid = float(np.median(rec["x"]))
        for name, sel in (("everybody", selection(0)),
                          ("a rectangle", selection(_abi.CS_SEL_RECT, x0=-1e9, y0=-1e9, x1=mid, y1=1e9)),
                          ("the late ones", selection(_abi.CS_SEL_LP, lp=led._handles(nolp)[0])),
                          ("a circle", selection(_abi.CS_SEL_CIRCLE, cx=mid, cy=mid, r=extent / 3)),
                          ("the walkers that move", selection(_abi.CS_SEL_SPEED | _abi.CS_SEL_SOURCE_SINK,
                                                              source_sink=NO_SINK, speed_lo=1e-6, speed_hi=9.0))):
            got = _agree(a, led, sel, rec, f"{when}: {name}")
            assert len(got) > 0 and int(got.min()) > 2 ** 32 and (np.diff(got.astype(np.int64)) > 0).all()

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
    gone = a.remove_selected(local_planner=nolp)
    assert len(gone) == 10 and len(a) == 600
    check_rec = a.read_agents()
    assert check_rec["id"].tolist() == sorted(ids)


def test_an_agent_the_index_never_took_is_selected_by_its_record():
    pts, pref, group, grid, extent = _crossing(1024)
    a = Simulation(LocationHash2D(**grid))
    led = Ledger(a).watch()
    _add_crossing(a, pts, group)
    _steps((a,), 3)
    hlp, lp = StubHighLevelPlan((0.0, 0.0)), NoLocalPlan()
    where = (grid["width"] * 5.0, 1.0)
    with pytest.raises(CrowdSimError):  # created, then refused by the index (lib.rs:133-149)
        a.add_agents([where], hlp, lp, 1.5)
    rec = a.read_agents()
    assert len(rec) == 1025
    limbo = int(rec["id"][-1])
    assert (float(rec["x"][-1]), float(rec["y"][-1])) == where
    led.of[limbo] = (NO_SINK,) + led._handles(hlp, lp)
    h_hlp, h_lp = led._handles(hlp, lp)
    cases = [("no term", selection(0), True),
             ("no sink", selection(_abi.CS_SEL_SOURCE_SINK, source_sink=NO_SINK), True),
             ("its planner", selection(_abi.CS_SEL_HLP, hlp=h_hlp), True),
             ("its local planner", selection(_abi.CS_SEL_LP | _abi.CS_SEL_HLP, hlp=h_hlp, lp=h_lp), True),
             ("at rest, waypoint 0", selection(_abi.CS_SEL_SPEED | _abi.CS_SEL_WAYPOINT, speed_lo=0.0, speed_hi=1e-9), True),
             ("a rectangle round where it was created",
              selection(_abi.CS_SEL_RECT, x0=where[0], y0=0.0, x1=where[0] + 1.0, y1=2.0), True),
             ("a circle round where it was created", selection(_abi.CS_SEL_CIRCLE, cx=where[0], cy=0.0, r=1.5), True),
             ("the whole grid", selection(_abi.CS_SEL_RECT, x0=0.0, y0=0.0, x1=grid["width"], y1=grid["height"]), False),
             ("another planner", selection(_abi.CS_SEL_HLP, hlp=0), False),
             ("moving", selection(_abi.CS_SEL_SPEED, speed_lo=0.1, speed_hi=9.0), False)]
    lengths = []
    for name, sel, inside in cases:
        got = _agree(a, led, sel, rec, name)
        assert (limbo in got) == inside, name
        lengths.append(len(got))
    rc, counts = count(a, [s for _, s, _ in cases])
    assert rc == 0 and counts.tolist() == lengths
    n, few = select(a, cases[0][1], cap=1024)  # (the limbo agent has the largest id: beyond the cap)
    assert n == 1025 and few.tolist() == rec["id"][:1024].tolist()
    with pytest.raises(CrowdSimError, match="Index out of bounds"):  # every step still fails on it (lib.rs:299-302)
        a.step(0.05)


def test_refusals_leave_the_engine_usable():
    (a,), (led,), sinks, _ = _scene(0)
    _advance((a,), (led,), 12)
    rec = a.read_agents()
    nan = float("nan")
    good = selection(_abi.CS_SEL_RECT | _abi.CS_SEL_SPEED, x0=60.0, y0=50.0, x1=120.0, y1=140.0, speed_lo=0.5, speed_hi=3.0)
    bad = [("unknown term bits", selection(128)),
           ("unknown term bits beside known ones", selection(_abi.CS_SEL_RECT | 0x80000000, x1=1.0, y1=1.0)),
           ("NaN x0", selection(_abi.CS_SEL_RECT, x0=nan, y0=0.0, x1=1.0, y1=1.0)),
           ("NaN y1", selection(_abi.CS_SEL_RECT, x0=0.0, y0=0.0, x1=1.0, y1=nan)),
           ("NaN cx", selection(_abi.CS_SEL_CIRCLE, cx=nan, cy=0.0, r=1.0)),
           ("NaN r", selection(_abi.CS_SEL_CIRCLE, cx=0.0, cy=0.0, r=nan)),
           ("negative r", selection(_abi.CS_SEL_CIRCLE, cx=100.0, cy=100.0, r=-1.0)),
           ("NaN speed_lo", selection(_abi.CS_SEL_SPEED, speed_lo=nan, speed_hi=1.0)),
           ("NaN speed_hi", selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=nan))]
    lib, e = a._lib, a._engine
    out = np.full(len(rec), 0xABABABABABABABAB, dtype=np.uint64)
    ids_p = out.ctypes.data_as(C.POINTER(C.c_uint64))

    def refused(rc, call, name):
        assert rc == (3 if call == "count_agents" else SIZE_MAX), name
        assert call in lib.cs_last_error(e).decode(), (name, lib.cs_last_error(e).decode())
        assert (out == 0xABABABABABABABAB).all(), name
        _agree(a, led, good, rec, f"after the refusal of {name}")  # the next selection is right
    for name, sel in bad:
        refused(lib.cs_select_agents(e, C.byref(sel), ids_p, len(out)), "select_agents", name)
        refused(lib.cs_remove_selected(e, C.byref(sel), ids_p, len(out)), "remove_selected", name)
        arr = (_abi.Selection * 3)(good, sel, good)
        refused(lib.cs_count_agents(e, arr, 3, ids_p), "count_agents", name)
        with pytest.raises(CrowdSimError):
            a.count_agents([Selection(), sel])
    refused(lib.cs_select_agents(e, None, ids_p, len(out)), "select_agents", "a null selection")
    refused(lib.cs_remove_selected(e, None, ids_p, len(out)), "remove_selected", "a null selection")
    refused(lib.cs_count_agents(e, None, 2, ids_p), "count_agents", "null selections")
    arr = (_abi.Selection * 2)(good, good)
    refused(lib.cs_count_agents(e, arr, 2, None), "count_agents", "null counts")
    many = (_abi.Selection * 1025)(*([good] * 1025))
    big = np.full(1025, 0xABABABABABABABAB, dtype=np.uint64)
    assert lib.cs_count_agents(e, many, 1025, big.ctypes.data_as(C.POINTER(C.c_uint64))) == 3
    assert "count_agents" in lib.cs_last_error(e).decode() and (big == 0xABABABABABABABAB).all()
    assert lib.cs_count_agents(e, None, 0, None) == 0  # (nothing asked)
    # a NaN in a field no set term reads is nobody's business; +-inf are fine
    idle = selection(_abi.CS_SEL_RECT, x0=-float("inf"), y0=50.0, x1=float("inf"), y1=140.0, cx=nan, r=-1.0, speed_lo=nan)
    assert len(_agree(a, led, idle, rec, "a NaN in an unread field")) > 0
    assert len(a) == len(rec) and a.read_agents().tobytes() == rec.tobytes() and drain(a) == []
    a.step(0.05)  # (not poisoned)


def test_a_million_agents_one_per_cent_half_and_everybody():
    """The multi-workgroup append and every radix pass: 1,000,000 agents, 5 steps, three rectangles."""
    pts, grid, extent, group = scenes.uniform_crowd(1_000_000, seed=5, cell_size=2.0)
    a = Simulation(LocationHash2D(**grid))
    scenes.add_counterflow(a, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    _steps((a,), 5)
    rec = a.read_agents()
    assert len(rec) == 1_000_000
    x, y = rec["x"], rec["y"]
    none = np.zeros(len(rec), dtype=np.uint64)
    inf = float("inf")
    for name, sel, lo, hi in (
            ("one per cent", selection(_abi.CS_SEL_RECT, x0=float(np.quantile(x, 0.45)), x1=float(np.quantile(x, 0.55)),
                                       y0=float(np.quantile(y, 0.45)), y1=float(np.quantile(y, 0.55))), 5_000, 20_000),
            ("half", selection(_abi.CS_SEL_RECT, x0=-inf, x1=float(np.median(x)), y0=-inf, y1=inf), 400_000, 600_000),
            ("everybody", selection(_abi.CS_SEL_RECT, x0=-inf, x1=inf, y0=-inf, y1=inf), 1_000_000, 1_000_000)):
        want = rec["id"][pred(sel, rec, none, none, none)]
        n, got = select(a, sel)
        print(f"{name}: restatement {len(want)}, engine {n}")
        assert lo <= len(want) <= hi
        assert n == len(want) and (got == want).all(), name
