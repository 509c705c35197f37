"""Sending agents to goals by id in batches on one engine (include/crowdstep_state.h, Simulation.set_targets): the batch
has the effect of `planner.set_target(&agents[&id], goal, tol)` made in batch order (rmf/mod.rs:217-236).  The reference
of every parity test is the f64 oracle with a host-side follower (tests/host_follower.py, pinned on the CPU in
tests/test_set_targets_abi.py) on which set_target is called agent by agent; tolerance 1e-4 of the domain length with
ids and next_waypoint exact; tiled == gather bitwise ("Sending agents to goals between steps")."""
import subprocess

import numpy as np
import pytest

from oracle_sim import OracleSimulation
from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, HighLevelPlanner,
                              IdParityHighLevelPlan, LocationHash2D, MonotonicCrowd, NoHighLevelPlan, NoLocalPlan,
                              RouteFollower, Simulation, SourceSink, StubHighLevelPlan, Zanlungo, _abi)
from set_targets_scenes import EXITS, Host, lattice, run_dispatch, run_stream, run_swirl, same_calls
from test_oracle_reference_kats import DoglegRoutes

pytestmark = pytest.mark.gpu
FLAGS = [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER]
IGNORED, BOOKED, PLANNED, NO_PATH, FORWARDED = range(5)
GRID = (160.0, 160.0, 2.0, (0.0, 0.0))


def max_rel_err(a, b, scale):
    assert (a["id"] == b["id"]).all()
    return float(np.hypot(a["x"] - b["x"], a["y"] - b["y"]).max() / scale)


_reference = {}


def _ref(name, run):
    if name not in _reference:
        _reference[name] = run()
    return _reference[name]


# ---- parity with the reference host ------------------------------------------------------------------------------
def test_dispatch_matches_the_reference_host():
    """Dispatch, NoLocalPlan: 1600 agents sent to four exits three times (everybody, two thirds in id order, two thirds
    in a random order).  Statuses entry by entry and the plan_route log equal the reference host's; flags 0, FORCE_TILED
    and FORCE_GATHER agree bitwise."""
    ref = _ref("dispatch", lambda: run_dispatch(OracleSimulation, True))
    b = ref.sim.read_agents()
    assert len(b) == 1600 and all(np.isfinite(b[f]).all() for f in ("x", "y", "vx", "vy"))
    assert ref.statuses.count(PLANNED) > 1000 and ref.statuses.count(BOOKED) > 1000
    runs = [run_dispatch(Simulation, False, flags=f) for f in FLAGS]
    a = runs[0].sim.read_agents()
    err = max_rel_err(a, b, 160.0)
    print(f"dispatch: {len(ref.statuses)} entries, {ref.statuses.count(PLANNED)} planned, {ref.statuses.count(BOOKED)} "
          f"booked, {len(ref.routes.calls)} routes, max |dp|/L = {err:.3e}")
    assert err <= 1e-4 and (a["next_waypoint"] == b["next_waypoint"]).all()
    for h in runs:
        assert h.statuses == ref.statuses
        assert same_calls(h.calls(), ref.calls())
        assert h.sim.read_agents().tobytes() == a.tobytes()


@pytest.mark.parametrize("side", [32, 48])
def test_dispatch_under_zanlungo_matches_the_reference_host(side):
    """The swirl: private doglegs (scale 0.5) under Zanlungo, 25 steps (the reference's own NaN comes at step 39).  No
    agent is left out of the comparison.  On the tiled kernel, equal to gather bitwise."""
    ref = _ref(("swirl", side), lambda: run_swirl(OracleSimulation, True, side=side))
    b = ref.sim.read_agents()
    assert len(b) == side * side
    assert all(np.isfinite(b[f]).all() for f in ("x", "y", "vx", "vy"))
    pushed = int((np.abs(np.hypot(b["vx"], b["vy"]) - 1.2) > 1e-6).sum())
    assert pushed >= 20, pushed
    tiled = run_swirl(Simulation, False, side=side, flags=CS_CFG_FORCE_TILED)
    gather = run_swirl(Simulation, False, side=side, flags=CS_CFG_FORCE_GATHER)
    a = tiled.sim.read_agents()
    err = max_rel_err(a, b, 160.0)
    print(f"swirl {side} x {side}: {len(ref.routes.calls)} routes, {pushed} agents pushed, max |dp|/L = {err:.3e}")
    assert err <= 1e-4
    assert tiled.statuses == ref.statuses and same_calls(tiled.calls(), ref.calls())
    assert a.tobytes() == gather.sim.read_agents().tobytes() and gather.statuses == ref.statuses


@pytest.mark.parametrize("flags", [0, CS_CFG_FORCE_TILED])
def test_source_sink_agents_resent_mid_leg_match_the_reference_host(flags):
    """The 16-sink dogleg stream; at steps 50, 120 and 500 every third live agent is sent 30 m on and 5 m aside, then
    the sink's own set_target at its waypoint takes over again.  Counts, events and next_waypoint exact."""
    ref = _ref("stream", lambda: run_stream(OracleSimulation, True))
    b = ref.sim.read_agents()
    assert np.isfinite(b["x"]).all() and len(b) > 1000 and len(ref.routes.calls) > 200
    h = run_stream(Simulation, False, flags=flags)
    a = h.sim.read_agents()
    assert h.counts == ref.counts
    assert h.listener.added == ref.listener.added and h.listener.removed == ref.listener.removed
    err = max_rel_err(a, b, 160.0)
    print(f"stream re-sent: {len(a)} alive, {sum(c[2] for c in h.counts)} destroyed, {sum(c[3] for c in h.counts)} "
          f"waypoint hits, {len(h.routes.calls)} routes, max |dp|/L = {err:.3e}")
    assert err <= 1e-4 and (a["next_waypoint"] == b["next_waypoint"]).all()
    # the batches' own entries (the reference object also logs the sinks' calls, the engine's statuses do not)
    assert len(h.statuses) > 300 and set(h.statuses) <= {BOOKED, PLANNED}
    assert same_calls(h.calls(), ref.calls(), goals_exact=False)  # (goals from each side's own positions)


# ---- order inside a batch ----------------------------------------------------------------------------------------
def _pair(scale=4.0):
    h = Host(Simulation, False, scale=scale)
    ids = h.sim.add_agents([(41.0, 41.0), (41.5, 41.5)], h.hlp, NoLocalPlan(), 2.0)  # one hash cell at scale 4
    return h, ids


def test_the_first_entry_of_a_pair_plans_with_its_own_position():
    h, ids = _pair()
    assert h.send(ids, [EXITS[2], EXITS[2]]) == [PLANNED, BOOKED]
    assert h.routes.calls == [((41.0, 41.0), EXITS[2])]
    h, ids = _pair()
    assert h.send(ids[::-1], [EXITS[2], EXITS[2]]) == [PLANNED, BOOKED]
    assert h.routes.calls == [((41.5, 41.5), EXITS[2])]
    # both walk the first one's route: towards its dogleg point
    for _ in range(3):
        h.sim.step(0.1)
    a = h.sim.read_agents()
    assert (np.hypot(a["vx"], a["vy"]) > 1.19).all()


def test_an_id_given_twice_ends_on_the_last_goal_and_books_both_routes():
    h, ids = _pair()
    twin, _ = _pair()
    st = h.send([ids[0], ids[1], ids[0]], [EXITS[0], EXITS[0], EXITS[2]])
    assert st == [PLANNED, BOOKED, PLANNED] and len(h.routes.calls) == 2
    assert twin.send(ids, [EXITS[2], EXITS[0]]) == [PLANNED, PLANNED]
    # both routes are in the book: sending the other agent to either goal plans nothing more
    assert h.sim.set_targets([ids[1], ids[1]], [EXITS[2], EXITS[0]]).tolist() == [BOOKED, BOOKED]
    assert twin.sim.set_targets([ids[1], ids[1]], [EXITS[2], EXITS[0]]).tolist() == [BOOKED, BOOKED]
    assert len(h.routes.calls) == 2
    for _ in range(20):
        h.sim.step(0.1)
        twin.sim.step(0.1)
    a, b = h.sim.read_agents(), twin.sim.read_agents()
    assert a[0].tobytes() == b[0].tobytes() and a["x"][0] > 41.5  # on its way to (140, 140)


def test_a_goal_without_a_path_leaves_the_agent_on_its_old_route():
    h, ids = _pair()
    twin, _ = _pair()
    for s in (h, twin):
        assert s.send(ids, [EXITS[1], EXITS[1]]) == [PLANNED, BOOKED]
        for _ in range(5):
            s.sim.step(0.1)
    assert h.send([ids[0]], [(1000.0, 40.0)]) == [NO_PATH]
    assert h.routes.calls[-1][1] == (1000.0, 40.0)
    assert h.send([ids[0]], [(1000.0, 40.0)]) == [NO_PATH] and len(h.routes.calls) == 3  # (nothing was booked)
    for _ in range(20):
        h.sim.step(0.1)
        twin.sim.step(0.1)
    assert h.sim.read_agents().tobytes() == twin.sim.read_agents().tobytes()


def test_an_added_agent_sent_to_the_sinks_waypoint_moves_as_the_agent_the_sink_spawned():
    """An agent added at a sink's source and sent to the sink's first waypoint takes the very route the sink's agents
    take: bit for bit the same motion until the waypoint."""
    routes = DoglegRoutes()
    hlp = RouteFollower(routes, scale=4.0, arrive=0.1, speed=1.2)
    spawning = Simulation(LocationHash2D(*GRID))
    spawning.add_source_sink(SourceSink((20.0, 50.0), 1.0, MonotonicCrowd(10.0), hlp, NoLocalPlan(),
                                        [(60.0, 53.0), (100.0, 50.0)], False, 2.0))
    spawning.step(0.1)
    born = spawning.read_agents()
    assert len(born) == 1
    sent_routes = DoglegRoutes()
    sent = Simulation(LocationHash2D(*GRID))
    ids = sent.add_agents([(20.0, 50.0)], RouteFollower(sent_routes, scale=4.0, arrive=0.1, speed=1.2), NoLocalPlan(), 2.0)
    assert list(sent.set_targets(ids, [(60.0, 53.0)])) == [PLANNED]
    sent.step(0.1)
    assert sent_routes.calls == routes.calls[:1]
    for _ in range(250):
        a, b = sent.read_agents(), spawning.read_agents()
        b = b[b["id"] == born["id"][0]]
        assert [a[f][0] for f in ("x", "y", "vx", "vy")] == [b[f][0] for f in ("x", "y", "vx", "vy")]
        sent.step(0.1)
        spawning.step(0.1)
    assert a["x"][0] > 45.0


# ---- refused batches ---------------------------------------------------------------------------------------------
class Listening(HighLevelPlanner):
    def __init__(self):
        self.targets = []

    def get_desired_velocity(self, agent, time):
        return (0.25, 0.0)

    def set_target(self, agent, point, tolerance):
        self.targets.append((agent.agent_id, tuple(agent.position), tuple(point), tuple(tolerance)))


def _crowd(led=True):
    h = Host(Simulation, False, scale=4.0)
    h.heard = Listening()
    h.ids = h.sim.add_agents(lattice(12, 12, 1.6, (60.0, 60.0), 0.15, 3), h.hlp, NoLocalPlan(), 2.0)
    if led:  # (a group led by host code: the engine asks it every step)
        h.led = h.sim.add_agents(lattice(4, 4, 1.6, (100.0, 60.0), 0.0, 0), h.heard, NoLocalPlan(), 2.0)
    return h


def test_a_refused_batch_calls_no_planner_and_leaves_no_trace():
    h, twin = _crowd(), _crowd()
    for s in (h, twin):
        s.sim.step(0.1)
    gone = h.ids[5]
    for s in (h, twin):
        s.sim.remove_agents(gone)
    batch = h.ids[:5] + h.led[:2] + h.ids[6:40]
    goals = np.array([EXITS[k % 4] for k in range(len(batch))], dtype=np.float64)
    for bad_ids, bad_goals, why in (
            (batch + [10 ** 9], np.vstack([goals, goals[:1]]), "unknown agent id"),
            (batch + [gone], np.vstack([goals, goals[:1]]), "unknown agent id"),
            (batch, np.vstack([goals[:-1], [[np.nan, 1.0]]]), "not finite"),
            (batch, np.vstack([goals[:-1], [[np.inf, 1.0]]]), "not finite")):
        with pytest.raises(CrowdSimError, match=why):
            h.sim.set_targets(bad_ids, bad_goals)
    with pytest.raises(CrowdSimError, match="not finite"):
        h.sim.set_targets(batch, goals, tolerance=(np.nan, 0.0))
    keys = np.asarray(batch, dtype=np.uint64)
    import ctypes as C
    rc = h.sim._lib.cs_set_targets(h.sim._engine, keys.ctypes.data_as(C.POINTER(C.c_uint64)), None, len(keys), 0.0, 0.0,
                                   None)
    assert rc == 3 and "null array" in h.sim._lib.cs_last_error(h.sim._engine).decode()
    assert h.sim._lib.cs_set_targets(h.sim._engine, None, None, 0, 0.0, 0.0, None) == 0  # n == 0 is Ok
    assert len(h.sim.set_targets([], np.zeros((0, 2)))) == 0
    assert h.routes.calls == [] and h.heard.targets == []
    # the next valid batch behaves as on a twin that never saw the refused ones; the engine steps on
    sa, sb = h.send(batch, goals), twin.send(batch, goals)
    assert sa == sb and h.routes.calls == twin.routes.calls and h.heard.targets == twin.heard.targets
    assert PLANNED in sa and BOOKED in sa and sa.count(FORWARDED) == 2
    for _ in range(15):
        h.sim.step(0.1)
        twin.sim.step(0.1)
    assert h.sim.read_agents().tobytes() == twin.sim.read_agents().tobytes()


# ---- planner kinds -----------------------------------------------------------------------------------------------
def test_a_host_planner_hears_its_agents_targets_in_batch_order():
    h = _crowd()
    h.sim.step(0.1)
    a = h.sim.read_agents()
    order = [h.led[3], h.ids[0], h.led[0], h.led[3]]
    goals = [(10.0, 11.0), EXITS[0], (12.0, 13.0), (14.0, 15.0)]
    assert list(h.sim.set_targets(order, goals, tolerance=(0.5, 0.25))) == [FORWARDED, PLANNED, FORWARDED, FORWARDED]
    at = {int(r["id"]): (float(r["x"]), float(r["y"])) for r in a}
    assert h.heard.targets == [(h.led[3], at[h.led[3]], (10.0, 11.0), (0.5, 0.25)),
                               (h.led[0], at[h.led[0]], (12.0, 13.0), (0.5, 0.25)),
                               (h.led[3], at[h.led[3]], (14.0, 15.0), (0.5, 0.25))]


@pytest.mark.parametrize("flags", [0, CS_CFG_FORCE_TILED])
def test_planners_that_take_no_targets_ignore_them(flags):
    def build():
        sim = Simulation(LocationHash2D(*GRID), flags=flags)
        zan = Zanlungo(0.3, 1.0, 0.0, 0.4, 2.0, 0.2)
        ids = sim.add_agents(lattice(10, 10, 1.1, (60.0, 60.0), 0.1, 1), StubHighLevelPlan((0.4, 0.1)), zan, 2.0)
        ids += sim.add_agents(lattice(10, 10, 1.1, (72.0, 60.0), 0.1, 2), IdParityHighLevelPlan((0.0, 0.3)), zan, 2.0)
        ids += sim.add_agents(lattice(5, 5, 1.1, (60.0, 72.0), 0.1, 3), NoHighLevelPlan(), zan, 2.0)
        return sim, ids
    (a, ids), (b, _) = build(), build()
    for k in range(20):
        if k in (0, 7):
            assert (a.set_targets(ids[::-1], [EXITS[i % 4] for i in ids]) == IGNORED).all()
        a.step(0.05)
        b.step(0.05)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


# ---- the engine around the call ----------------------------------------------------------------------------------
def test_a_batch_behind_steps_queued_without_a_report():
    queued, waited = _crowd(led=False), _crowd(led=False)
    for s in (queued, waited):
        s.send(s.ids, [EXITS[i % 4] for i in s.ids])
    for _ in range(30):
        queued.sim.step(0.1, report=False)
        waited.sim.step(0.1)
    waited.sim.synchronize()
    goals = [EXITS[(i + 2) % 4] for i in queued.ids]
    assert queued.send(queued.ids, goals) == waited.send(waited.ids, goals)
    assert queued.routes.calls == waited.routes.calls
    for _ in range(10):
        queued.sim.step(0.1, report=False)
        waited.sim.step(0.1)
    assert queued.sim.read_agents().tobytes() == waited.sim.read_agents().tobytes()


def test_external_ids_before_and_after_a_renumbering(monkeypatch):
    """The set-up of test_gpu_wide_ids.py: ids from 2^40 on through a 4096-id device space.  The same batch by external
    id gives the same statuses and motion as on an engine with plain ids."""
    def run(wide):
        first = 2 ** 40 if wide else 0
        monkeypatch.setenv("CS_FIRST_AGENT_ID", str(first))
        if wide:
            monkeypatch.setenv("CS_DEVICE_ID_LIMIT", "4096")
        else:
            monkeypatch.delenv("CS_DEVICE_ID_LIMIT", raising=False)
        h = Host(Simulation, False, scale=4.0, flags=CS_CFG_WIDE_IDS if wide else 0)
        ids = h.sim.add_agents(lattice(20, 20, 1.6, (60.0, 60.0), 0.15, 3), h.hlp, NoLocalPlan(), 2.0)
        assert ids == list(range(first, first + 400))
        out = [h.send(ids[::-1], [EXITS[(i - first) % 4] for i in ids[::-1]])]
        spot = np.array([[20.0, 150.0]])
        for r in range(12):  # 12 x 500 ids: the device ids are renumbered several times
            more = h.sim.add_agents(np.repeat(spot, 500, axis=0) + np.arange(500)[:, None] * 0.01,
                                    StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.0)
            h.sim.step(0.1)
            h.sim.remove_agents_by_id(more)
        renumbered = h.sim.kernel_stat(_abi.CS_STAT_RENUMBERINGS)
        out.append(h.send(ids[::3], [EXITS[(i - first + 1) % 4] for i in ids[::3]]))
        with pytest.raises(CrowdSimError, match="unknown agent id"):
            h.sim.set_targets([first + 450], [EXITS[0]])  # (an id of an agent that was removed)
        for _ in range(10):
            h.sim.step(0.1)
        a = h.sim.read_agents()
        assert (a["id"] == np.arange(first, first + 400, dtype=np.uint64)).all()
        return out, h.calls(), a, renumbered
    (st_w, calls_w, a_w, n_w), (st_p, calls_p, a_p, n_p) = run(True), run(False)
    assert n_w >= 1 and n_p == 0
    assert st_w == st_p and calls_w == calls_p
    assert all(a_w[f].tobytes() == a_p[f].tobytes() for f in ("x", "y", "vx", "vy", "next_waypoint"))


def test_a_dispatch_on_kept_windows_equals_windows_cut_every_step(monkeypatch):
    runs = {}
    for keep in ("1", "0"):
        monkeypatch.setenv("CS_WINDOWS_KEEP", keep)
        h = Host(Simulation, False, scale=0.5, flags=CS_CFG_FORCE_TILED)
        pts = lattice(40, 40, 2.4, (30.0, 30.0), 0.1, 9)
        ids = h.sim.add_agents(pts, h.hlp, Zanlungo(0.3, 1.0, 0.0, 0.4, 2.0, 0.2), 2.0)
        for k in range(24):
            if k in (0, 9):
                h.send(ids[::(k + 1)], pts[::(k + 1)] + ((30.0, 10.0) if k == 0 else (-5.0, 25.0)))
            h.sim.step(0.1)
        runs[keep] = (h.sim.read_agents(), h.sim.kernel_stat(_abi.CS_STAT_STEPS_ON_KEPT_WINDOWS), h.statuses)
    print(f"steps on kept windows: {runs['1'][1]} / {runs['0'][1]}")
    assert runs["1"][1] > 0 and runs["0"][1] == 0
    assert runs["1"][0].tobytes() == runs["0"][0].tobytes() and runs["1"][2] == runs["0"][2]


def test_all_booked_at_size():
    """200,000 agents in few hash cells (scale 50): the first dispatch plans a few hundred routes; sent again from the
    same positions every entry is answered on the device: no route_plan call, every status BOOKED, no device memory."""
    h = Host(Simulation, False, scale=50.0, grid=(400.0, 400.0, 2.0, (0.0, 0.0)))
    rng = np.random.default_rng(12)
    pts = rng.uniform(20.0, 380.0, (200_000, 2))
    ids = np.asarray(h.sim.add_agents(pts, h.hlp, NoLocalPlan(), 1.0), dtype=np.uint64)
    exits = np.array([(10.0, 10.0), (390.0, 10.0), (390.0, 390.0), (10.0, 390.0), (200.0, 10.0)])
    order = rng.permutation(len(ids))
    goals = exits[order % 5]
    first = h.sim.set_targets(ids[order], goals)
    planned = int((first == PLANNED).sum())
    assert 50 < planned < 1000 and planned + int((first == BOOKED).sum()) == len(ids) and len(h.routes.calls) == planned
    # the first dispatch met an empty device book: what it booked through earlier entries, the host's map answered
    assert h.sim.targets_answered_on_device == 0
    a = h.sim.read_agents()
    held = h.sim.device_bytes
    again = h.sim.set_targets(ids[order], goals)
    assert (again == BOOKED).all() and len(h.routes.calls) == planned
    assert h.sim.targets_answered_on_device == len(ids)  # every entry by k_target_probe, none by a host lookup
    assert h.sim.device_bytes == held
    assert h.sim.read_agents().tobytes() == a.tobytes()
    h.sim.step(0.1)
    b = h.sim.read_agents()
    assert (np.abs(np.hypot(b["vx"], b["vy"]) - 1.2) < 1e-4).all()


# ---- Python's own spelling, C++ ----------------------------------------------------------------------------------
def test_route_follower_set_target_forwards_to_the_batched_call():
    h, ids = _pair()
    agents = h.sim.agents
    assert h.hlp.set_target(agents[ids[0]], EXITS[2], (0.0, 0.0)) == PLANNED
    assert h.hlp.set_target(agents[ids[1]], np.array(EXITS[2]), np.zeros(2)) == BOOKED
    assert h.routes.calls == [((41.0, 41.0), EXITS[2])]
    other = Simulation(LocationHash2D(*GRID))
    other.add_agents([(50.0, 50.0)], h.hlp, NoLocalPlan(), 2.0)
    with pytest.raises(CrowdSimError, match="Simulation.set_targets"):
        h.hlp.set_target(agents[ids[0]], EXITS[0], (0.0, 0.0))


def test_set_targets_in_cpp():
    """tests/cpp/test_set_targets.cpp sends, steps and prints; the same scene through the Python layer gives the same
    statuses and the same crowd, bit for bit."""
    from test_gpu_cpp_api import build_cpp_test
    out = subprocess.run([build_cpp_test("test_set_targets")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "set targets: passed" in out.stdout
    h = Host(Simulation, False, scale=4.0, grid=(80.0, 80.0, 2.0, (0.0, 0.0)))
    pts = [(30.0 + 1.5 * ix, 34.0 + 1.5 * iy) for ix in range(6) for iy in range(6)]
    ids = h.sim.add_agents(pts, h.hlp, NoLocalPlan(), 2.0)
    goals = [(60.0, 20.0)] * len(ids)
    goals[5] = (1000.0, 20.0)
    st = h.send(ids, goals)
    for _ in range(20):
        h.sim.step(0.1)
    st += [int(h.sim.set_targets([ids[5]], [(60.0, 20.0)], tolerance=(0.5, 0.5))[0])]
    for _ in range(5):
        h.sim.step(0.1)
    a = h.sim.read_agents()
    lines = out.stdout.splitlines()
    print("statuses", *st)
    assert [int(t) for t in [ln for ln in lines if ln.startswith("statuses")][0].split()[1:]] == st
    rows = [ln.split()[1:] for ln in lines if ln.startswith("agent ")]
    assert len(rows) == len(a)
    for row, r in zip(rows, a):
        print("agent", int(r["id"]), repr(float(r["x"])), repr(float(r["y"])), repr(float(r["vx"])), repr(float(r["vy"])))
        assert int(row[0]) == int(r["id"])
        assert [float(v) for v in row[1:]] == [float(r["x"]), float(r["y"]), float(r["vx"]), float(r["vy"])]
