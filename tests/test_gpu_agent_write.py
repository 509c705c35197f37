"""Writing agents between steps, by id, on one engine (include/crowdstep_state.h, Simulation.write_agents): a write
sets the start-of-step state of existing agents and the next step runs as if the previous one had left them there
("Writing agents between steps")."""
import os
import subprocess

import numpy as np
import pytest

from oracle_sim import OracleSimulation, fast_steps
from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, EventListener,
                              LocationHash2D, MonotonicCrowd, NoLocalPlan, Simulation, SourceSink, StubHighLevelPlan,
                              Zanlungo, _abi, scenes)
from rmf_crowdsim_amd.simulation import AGENT_DTYPE

pytestmark = pytest.mark.gpu
CROSSING = (0.3, 1.0, 0.0, 0.4, 2.0, 0.2)


def _crossing(n=4096, seed=5, steps=40):
    """Two interleaved flows crossing at 30 degrees at walking speed (tests/test_gpu_north_star.py::crossing_flows)."""
    from test_gpu_north_star import crossing_flows
    return crossing_flows(n, seed=seed, steps=steps)


def _add_crossing(sim, pts, group):
    th = np.radians(30.0)
    lp = Zanlungo(*CROSSING)
    sim.add_agents(pts[group == 0], StubHighLevelPlan((scenes.WALK_SPEED, 0.0)), lp, 2.0)
    sim.add_agents(pts[group == 1], StubHighLevelPlan((scenes.WALK_SPEED * np.cos(th), scenes.WALK_SPEED * np.sin(th))),
                   lp, 2.0)


def _twins(flags=0, n=4096):
    pts, pref, group, grid, extent = _crossing(n)
    sims = [Simulation(LocationHash2D(**grid), flags=flags) for _ in range(2)]
    for s in sims:
        _add_crossing(s, pts, group)
    return sims, grid


def _steps(sims, k, report=True):
    for s in sims:
        for _ in range(k):
            s.step(0.05, report=report)


@pytest.mark.parametrize("flags", [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER])
def test_writing_back_what_was_read_changes_nothing(flags):
    (a, b), _ = _twins(flags)
    _steps((a, b), 10)
    a.write_agents(a.read_agents())  # all three fields
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    _steps((a, b), 20)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


def test_a_written_position_lands_where_add_agents_puts_it():
    """Engine A adds at P; engine B adds elsewhere and writes P: the same state, bit for bit, and the same 20 steps.
    P includes points the saturating casts clamp into row / column 0 and points whose y aliases into the next row
    (location_hash_2d.rs:54-66)."""
    grid = dict(width=40.0, height=60.0, cell_size=2.0, offset=(-3.0, 1.5))  # row stride 20 cells, 30 rows
    rng = np.random.default_rng(3)
    P = np.concatenate([rng.uniform((0.0, 3.0), (50.0, 38.0), (300, 2)),
                        [[-3.5, 10.2], [-20.0, 7.7], [12.3, 0.2], [-4.0, -9.0],   # clamped: x, y, both
                         [9.1, 44.7], [21.6, 52.25], [30.3, 41.6]]])              # y beyond the stride: aliased
    elsewhere = rng.uniform((5.0, 5.0), (30.0, 30.0), (len(P), 2))
    a, b = Simulation(LocationHash2D(**grid)), Simulation(LocationHash2D(**grid))
    lp, hlp = Zanlungo(*scenes.METRIC_ZANLUNGO), StubHighLevelPlan((0.2, -0.1))
    a.add_agents(P, hlp, lp, 2.0)
    b.add_agents(elsewhere, hlp, lp, 2.0)
    rec = b.read_agents()
    rec["x"], rec["y"] = P[:, 0], P[:, 1]
    b.write_agents(rec, "position")
    ra, rb = a.read_agents(), b.read_agents()
    assert ra.tobytes() == rb.tobytes()
    assert (ra["x"] < grid["offset"][0]).sum() >= 3  # (the clamped ones keep their exact position)
    _steps((a, b), 20)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


def test_written_state_steps_like_the_oracle():
    """A 4096-agent crossing flow: after 10 steps half the crowd is teleported across the grid, 16 agents into a 3 x 3
    cell hotspot, every velocity is written at random; 30 more steps against the f64 CPU path from the state read back.
    Tiled == gather, bit for bit."""
    pts, pref, group, grid, extent = _crossing(4096)
    sims = {f: Simulation(LocationHash2D(**grid), flags=f) for f in (CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER)}
    for s in sims.values():
        _add_crossing(s, pts, group)
    _steps(sims.values(), 10)
    rec = sims[CS_CFG_FORCE_TILED].read_agents()
    rng = np.random.default_rng(11)
    upper = rec["y"] > np.median(rec["y"])
    rec["y"][upper] += grid["height"] - 8.0 - rec["y"][upper].max()  # across the grid, the formation kept
    lower = np.flatnonzero(~upper)
    hot = lower[:: len(lower) // 16][:16]
    k = np.arange(16)
    rec["x"][hot] = 10.3 + 0.7 * (k % 4)  # 16 agents 0.7 m apart inside cells [5, 8) x [5, 8)
    rec["y"][hot] = 10.2 + 0.7 * (k // 4)
    rec["vx"] = rng.uniform(-0.4, 0.4, len(rec))
    rec["vy"] = rng.uniform(-0.4, 0.4, len(rec))
    for s in sims.values():
        s.write_agents(rec)
    start = sims[CS_CFG_FORCE_TILED].read_agents()
    assert (start["y"][upper] > grid["height"] * 0.5).all()
    assert start.tobytes() == sims[CS_CFG_FORCE_GATHER].read_agents().tobytes()
    _steps(sims.values(), 30)
    got = sims[CS_CFG_FORCE_TILED].read_agents()
    assert got.tobytes() == sims[CS_CFG_FORCE_GATHER].read_agents().tobytes()
    th = np.radians(30.0)
    by_id_group = np.concatenate([np.zeros((group == 0).sum(), int), np.ones((group == 1).sum(), int)])
    pref_by_id = np.where(by_id_group[:, None] == 0, [scenes.WALK_SPEED, 0.0],
                          [scenes.WALK_SPEED * np.cos(th), scenes.WALK_SPEED * np.sin(th)])
    xy0 = np.stack([start["x"], start["y"]], axis=1)
    v0 = np.stack([start["vx"], start["vy"]], axis=1)
    struck = np.zeros(len(start), dtype=np.uint8)
    xy, vel, sec = fast_steps(xy0, pref_by_id, CROSSING, 2.0, grid, 0.05, 30, threads=min(16, os.cpu_count() or 1),
                              vel=v0, spurious=struck)
    assert sec >= 0
    d = np.hypot(got["x"] - xy[:, 0], got["y"] - xy[:, 1]) / extent
    d[struck != 0] = 0.0
    assert d.max() <= 1e-4, (d.max(), int((d > 1e-4).sum()))


def test_queries_and_the_spawn_probe_see_the_written_positions():
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    sim = Simulation(LocationHash2D(**grid))
    lp, hlp = NoLocalPlan(), StubHighLevelPlan((0.0, 0.0))
    ids = sim.add_agents([(5.0, 5.0), (30.0, 30.0)], hlp, lp, 1.0)
    sim.step(0.05)
    rec = sim.read_agents()
    rec["x"][0], rec["y"][0] = 20.5, 12.25
    sim.write_agents(rec[:1], "position")
    assert ids[0] in sim.get_neighbours_in_radius(0.5, (20.5, 12.25))
    assert ids[0] not in sim.get_neighbours_in_radius(1.0, (5.0, 5.0))
    # a source whose 0.4 m disk the write fills spawns nothing; emptied again, it spawns
    ss = SourceSink(source=np.array([10.0, 30.0]), radius_sink=0.5, crowd_generator=MonotonicCrowd(20.0),
                    high_level_planner=StubHighLevelPlan((0.0, 0.0)), local_planner=NoLocalPlan(),
                    waypoints=[np.array([10.0, 35.0])], loop_forever=False, agent_eyesight_range=1.0)
    sim.add_source_sink(ss)
    sim.step(0.05)
    assert sim.last_report["n_spawned"] == 1
    spawned = int(sim.read_agents()["id"].max())
    rec = sim.read_agents()
    rec = rec[rec["id"] == spawned]
    rec["x"], rec["y"] = 25.0, 25.0
    sim.write_agents(rec, "position")  # the disk is empty now
    sim.step(0.05)
    assert sim.last_report["n_spawned"] == 1
    rec = sim.read_agents()
    rec = rec[rec["id"] == ids[1]]
    rec["x"], rec["y"] = 10.1, 30.2  # into the disk (and the newest spawn moved out of it)
    newest = sim.read_agents()
    newest = newest[newest["id"] == newest["id"].max()]
    newest["x"], newest["y"] = 26.0, 26.0
    sim.write_agents(np.concatenate([rec, newest]), "position")
    sim.step(0.05)
    assert sim.last_report["n_spawned"] == 0
    rec["x"], rec["y"] = 12.0, 30.0
    sim.write_agents(rec, "position")
    sim.step(0.05)
    assert sim.last_report["n_spawned"] == 1


class _Events(EventListener):
    def __init__(self):
        self.events = []

    def agent_spawned(self, position, agent):
        self.events.append(("spawned", agent))

    def agent_destroyed(self, agent):
        self.events.append(("destroyed", agent))


def test_a_written_last_waypoint_at_the_sink_destroys_the_agent():
    grid = dict(width=60.0, height=60.0, cell_size=2.0, offset=(0.0, 0.0))
    sim = Simulation(LocationHash2D(**grid))
    ev = _Events()
    sim.add_event_listener(ev)
    wps = [np.array([10.0, 40.0]), np.array([40.0, 40.0]), np.array([40.0, 10.0])]
    ss = SourceSink(source=np.array([10.0, 10.0]), radius_sink=0.5, crowd_generator=MonotonicCrowd(20.0),
                    high_level_planner=StubHighLevelPlan((0.0, 1.0)), local_planner=NoLocalPlan(),
                    waypoints=wps, loop_forever=False, agent_eyesight_range=1.0)
    sim.add_source_sink(ss)
    for _ in range(60):
        sim.step(0.05)
    rec = sim.read_agents()
    assert len(rec) >= 4 and (rec["next_waypoint"] == 0).all()
    w = rec[:3].copy()
    w["next_waypoint"] = 2
    w["x"], w["y"] = 40.1, 9.8 + 0.1 * np.arange(3)  # within radius_sink of the sink after this step's 5 cm too
    sim.write_agents(w, ("position", "next_waypoint"))
    assert (sim.read_agents()[:3]["next_waypoint"] == 2).all()
    ev.events.clear()
    sim.step(0.05)
    assert sim.last_report["n_destroyed"] == 3
    assert sorted(i for k, i in ev.events if k == "destroyed") == sorted(int(i) for i in w["id"])
    left = set(int(i) for i in sim.read_agents()["id"])
    assert not left & set(int(i) for i in w["id"])
    bad = sim.read_agents()[:1].copy()
    bad["next_waypoint"] = 3  # the sink has three waypoints
    with pytest.raises(CrowdSimError, match="next_waypoint out of range"):
        sim.write_agents(bad, "next_waypoint")


def test_refused_batches_change_nothing():
    (a, b), grid = _twins(0, n=1024)
    _steps((a, b), 5)
    base = a.read_agents()
    gone = int(base["id"][7])
    a.remove_agents(gone)
    b.remove_agents(gone)
    base = a.read_agents()

    def one(**kw):
        r = base[:4].copy()
        for k, v in kw.items():
            r[k][1] = v
        return r
    cases = [
        (np.concatenate([base[:2], np.array([(gone, 1.0, 1.0, 0, 0, 0, 2.0)], dtype=AGENT_DTYPE)]), 7, "unknown agent id"),
        (np.concatenate([base[:3], base[1:2]]), 7, "twice"),
        (one(x=np.nan), 7, "not finite"),
        (one(vy=np.inf), 7, "not finite"),
        (one(vx=1e300), 7, "not finite"),
        (one(x=grid["width"] * 3.0), 7, "Index out of bounds"),
        (one(next_waypoint=1), 7, "next_waypoint out of range"),
        (base[:4], 0, "empty field mask"),
        (base[:4], 8, "unknown field mask"),
    ]
    for rec, fields, msg in cases:
        with pytest.raises(CrowdSimError, match=msg):
            a.write_agents(rec, fields)
        assert a.read_agents().tobytes() == base.tobytes(), msg
    _steps((a, b), 10)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    # an agent the index refused ("limbo", lib.rs:133-149) is not a live indexed agent
    with pytest.raises(CrowdSimError):
        a.add_agents([(grid["width"] * 5, 1.0)], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.0)
    limbo = [r for r in a.read_agents() if int(r["id"]) not in set(int(i) for i in b.read_agents()["id"])]
    assert len(limbo) == 1
    with pytest.raises(CrowdSimError, match="unknown agent id"):
        a.write_agents(np.array(limbo, dtype=AGENT_DTYPE), "velocity")


def test_a_tile_driven_by_hand_refuses_cells_it_does_not_own():
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    t = Simulation(LocationHash2D(**grid), tile=(0, 10, 0, 20), halo_cells=1)
    t.add_agents([(3.0, 3.0), (30.0, 3.0)], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.0)
    rec = t.read_agents()
    assert len(rec) == 1
    before = rec.tobytes()
    rec["x"] = 25.0  # row 12: another tile's
    with pytest.raises(CrowdSimError, match="does not own"):
        t.write_agents(rec, "position")
    assert t.read_agents().tobytes() == before
    rec["x"] = 7.0
    t.write_agents(rec, "position")
    assert t.read_agents()["x"][0] == 7.0


def test_steps_queued_without_a_report_finish_first():
    (a, b), _ = _twins(0, n=2048)
    _steps((a, b), 3)
    rec = a.read_agents()
    rec["vx"] *= 0.5
    _steps((a, b), 7, report=False)  # fire-and-forget
    b.synchronize()
    a.write_agents(rec, "velocity")
    b.write_agents(rec, "velocity")
    _steps((a, b), 5)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


def test_wide_ids_write_by_external_id_across_renumberings(monkeypatch):
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(2 ** 40 + 1))
    monkeypatch.setenv("CS_DEVICE_ID_LIMIT", "4096")
    pts, grid, extent, group = scenes.uniform_crowd(600, seed=9, cell_size=2.0, room=20.0)
    sim = Simulation(LocationHash2D(**grid), flags=CS_CFG_WIDE_IDS)
    monkeypatch.delenv("CS_DEVICE_ID_LIMIT")
    monkeypatch.delenv("CS_FIRST_AGENT_ID")
    ids = scenes.add_counterflow(sim, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    spot = np.array([[extent + 15.0, extent + 15.0]])
    late = []
    for r in range(10):  # 10 x 600 ids through a 4096-id device space
        more = sim.add_agents(np.repeat(spot, 600, axis=0) + np.arange(600)[:, None] * 0.01, StubHighLevelPlan((0.0, 0.0)),
                              NoLocalPlan(), 1.0)
        sim.step(0.05)
        for i in more[:-1]:
            sim.remove_agents(i)
        late.append(more[-1])
        if r in (6, 8):  # between two renumberings: ids below and above the last one
            rec = sim.read_agents()
            pick = rec[np.isin(rec["id"], np.array([ids[0], ids[5], late[0], late[-1]], dtype=np.uint64))]
            pick["vx"], pick["vy"] = 0.25, -0.5
            sim.write_agents(pick, "velocity")
            got = sim.read_agents()
            hit = np.isin(got["id"], pick["id"])
            assert hit.sum() == 4 and (got["vx"][hit] == 0.25).all() and (got["vy"][hit] == -0.5).all()
            assert (got["vx"][~hit] != 0.25).all()
    assert sim.kernel_stat(_abi.CS_STAT_RENUMBERINGS) >= 1
    rec = sim.read_agents()
    pick = rec[np.isin(rec["id"], np.array([ids[1], late[0], late[-1]], dtype=np.uint64))]
    assert len(pick) == 3
    pick["x"] = np.round(pick["x"] * 4.0) / 4.0 + 0.5  # (quarter metres: the f32 offset holds them exactly)
    sim.write_agents(pick, "position")
    got = sim.read_agents()
    hit = np.isin(got["id"], pick["id"])
    assert (got["x"][hit] == pick["x"]).all()
    rest = rec[~np.isin(rec["id"], pick["id"])]
    assert got[~hit].tobytes() == rest.tobytes()


def test_teleports_on_kept_windows_equal_fresh_windows(monkeypatch):
    """A small crowd steps on band windows cut one step earlier (CS_WINDOWS_KEEP); teleports into empty rows and columns
    void them, the next step cuts its own: no window errors (CS_CHECK_WINDOWS=1) and the CS_WINDOWS_KEEP=0 result."""
    monkeypatch.setenv("CS_CHECK_WINDOWS", "1")
    pts, grid, extent, group = scenes.uniform_crowd(6000, seed=4, cell_size=2.0, margin=30.0)
    runs = {}
    for keep in ("1", "0"):
        monkeypatch.setenv("CS_WINDOWS_KEEP", keep)
        sim = Simulation(LocationHash2D(**grid), flags=CS_CFG_FORCE_TILED)
        scenes.add_counterflow(sim, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
        runs[keep] = sim
    for k in range(12):
        rec = runs["1"].read_agents()
        if k in (3, 7):
            sel = rec[k:: 97][:40]
            j = np.arange(len(sel))
            if k == 3:  # into the empty rows of low x
                sel["x"], sel["y"] = 3.0 + 0.7 * (j // 20), 31.0 + 0.9 * (j % 20)
            else:  # into the empty columns of high y
                sel["x"], sel["y"] = 31.0 + 0.9 * (j % 20), grid["width"] - 5.0 - 0.7 * (j // 20)
            for s in runs.values():
                s.write_agents(sel, "position")
        for s in runs.values():
            s.step(0.05)
    assert runs["1"].kernel_stat(_abi.CS_STAT_STEPS_ON_KEPT_WINDOWS) > 0
    assert runs["0"].kernel_stat(_abi.CS_STAT_STEPS_ON_KEPT_WINDOWS) == 0
    assert runs["1"].read_agents().tobytes() == runs["0"].read_agents().tobytes()


def test_commit_agents_equals_write_agents():
    (a, b), _ = _twins(0, n=1024)
    _steps((a, b), 4)
    rec = b.read_agents()
    agents = a.agents
    for k, aid in enumerate(list(agents)[::50]):
        agents[aid].position = agents[aid].position + np.array([0.25, -0.125])
        agents[aid].velocity = np.array([0.1 * k, 0.0])
    agents[int(rec["id"][3])].next_waypoint = 0  # unchanged: not written
    edited = rec[::50].copy()
    edited["x"] += 0.25
    edited["y"] -= 0.125
    edited["vx"] = 0.1 * np.arange(len(edited))
    edited["vy"] = 0.0
    assert a.commit_agents() == len(edited)
    b.write_agents(edited, ("position", "velocity"))
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert a.commit_agents() == 0
    a.agents[int(rec["id"][0])].eyesight_range = 5.0
    with pytest.raises(CrowdSimError, match="only position, velocity and next_waypoint"):
        a.commit_agents()
    _steps((a, b), 5)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


def test_cpp_write_round_trip_and_mesh_mover():
    from test_gpu_cpp_api import build_cpp_test
    out = subprocess.run([build_cpp_test("test_agent_write")], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "agent write: passed" in out.stdout


def test_the_oracle_has_no_write():
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="needs the HIP engine"):
        sim.write_agents(np.zeros(1, dtype=AGENT_DTYPE))
