"""Reading and removing agents by id in batches on one engine (include/crowdstep_state.h,
Simulation.read_agents_by_id / remove_agents_by_id): a batched read returns the rows of read_agents() and disturbs
nothing; a batched remove leaves the engine where the loop of single removes leaves it, events and planner callbacks
included ("Reading and removing agents by id").  Twins are compared bit for bit."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from oracle_sim import OracleSimulation
from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, EventListener,
                              HighLevelPlanner, LocationHash2D, MonotonicCrowd, NoLocalPlan, Simulation, SourceSink,
                              StubHighLevelPlan, Zanlungo, _abi, scenes)
from rmf_crowdsim_amd.simulation import AGENT_DTYPE
from test_gpu_agent_write import _add_crossing, _crossing, _steps, _twins

pytestmark = pytest.mark.gpu
FLAGS = [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER]
STAGED_KEYS_MAX = 40960  # the match stages up to this many keys in LDS (csrc/cs_agent_write.hip.inc)


def _rows(full, ids):
    """The rows of a full read (ascending id) with these ids, in the order of `ids`."""
    ids = np.asarray(ids, dtype=np.uint64)
    at = np.searchsorted(full["id"], ids)
    assert (full["id"][at] == ids).all()
    return full[at]


def _keep_events(sim):
    """Record events and leave them in the engine's queue (the Python layer would hand them to listeners)."""
    sim._lib.cs_event_recording(sim._engine, 1)
    sim._dispatch_events = lambda: None


def _events(sim):
    """Drain the engine's queue: (kind, source_sink, id) in order."""
    buf, out = (_abi.Event * 4096)(), []
    while True:
        n = sim._lib.cs_drain_events(sim._engine, buf, len(buf))
        out += [(int(buf[i].kind), int(buf[i].source_sink), int(buf[i].id)) for i in range(n)]
        if n < len(buf):
            return out


class _Events(EventListener):
    def __init__(self):
        self.events = []

    def agent_spawned(self, position, agent):
        self.events.append(("spawned", agent))

    def agent_destroyed(self, agent):
        self.events.append(("destroyed", agent))


@pytest.mark.parametrize("flags", FLAGS)
def test_a_batched_read_equals_the_rows_of_a_full_read_and_disturbs_nothing(flags):
    (a, b), _ = _twins(flags)
    _steps((a, b), 10)
    full = a.read_agents()
    rng = np.random.default_rng(17)
    for size in (1, 7, 1000, len(full)):
        ids = rng.choice(full["id"], size, replace=False)  # (a random order)
        got = a.read_agents_by_id(ids)
        assert got.dtype == AGENT_DTYPE and got.tobytes() == _rows(full, ids).tobytes(), size
    ids = rng.choice(full["id"], 300, replace=True)
    ids = np.concatenate([ids, ids[:50], ids[:1], ids[:1]])  # repeats: every occurrence is answered
    assert len(np.unique(ids)) < len(ids)
    assert a.read_agents_by_id(ids).tobytes() == _rows(full, ids).tobytes()
    got, found = a.read_agents_by_id(ids, missing_ok=True)
    assert found.all() and got.tobytes() == _rows(full, ids).tobytes()
    assert len(a.read_agents_by_id([])) == 0
    assert a.read_agents().tobytes() == full.tobytes()
    for k in range(20):  # a read between any two steps
        a.step(0.05)
        b.step(0.05)
        a.read_agents_by_id(rng.choice(full["id"], 64, replace=False))
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    kept = [s.kernel_stat(_abi.CS_STAT_STEPS_ON_KEPT_WINDOWS) for s in (a, b)]
    print(f"flags {flags}: steps on kept windows {kept}")
    assert kept[0] == kept[1]


def test_reads_between_steps_keep_the_kept_windows(monkeypatch):
    """The set-up of tests/test_gpu_kept_windows.py: a small crowd steps on band windows cut one step earlier.  A read
    between two steps leaves them valid: the counter advances as on an untouched twin."""
    monkeypatch.setenv("CS_WINDOWS_KEEP", "1")
    pts, grid, extent, group = scenes.uniform_crowd(6000, seed=4, cell_size=2.0, margin=30.0)
    sims = [Simulation(LocationHash2D(**grid), flags=CS_CFG_FORCE_TILED) for _ in range(2)]
    for s in sims:
        ids = scenes.add_counterflow(s, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    a, b = sims
    for k in range(12):
        a.step(0.05)
        b.step(0.05)
        full = a.read_agents_by_id(ids[k::13])
        assert len(full) == len(ids[k::13])
    kept = [s.kernel_stat(_abi.CS_STAT_STEPS_ON_KEPT_WINDOWS) for s in sims]
    print(f"steps on kept windows: read {kept[0]}, untouched {kept[1]}")
    assert kept[0] == kept[1] and kept[1] > 0
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


def _sink_scene(sim, hlp=None):
    """Walkers, a source-sink whose agents reach their sink within four seconds, and (with `hlp`) a group led by a
    callback planner."""
    lp = Zanlungo(*scenes.METRIC_ZANLUNGO)
    ix, iy = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    pts = np.stack([18.0 + 1.05 * ix.ravel() + 0.01 * iy.ravel(), 17.5 + 1.1 * iy.ravel() + 0.02 * ix.ravel()], axis=1)
    ids = {"plain": sim.add_agents(pts, StubHighLevelPlan((0.3, 0.25)), lp, 2.0)}
    if hlp is not None:
        ids["callback"] = sim.add_agents(pts[:40] + np.array([0.0, 22.0]), hlp, lp, 2.0)
    sim.add_source_sink(SourceSink(source=np.array([8.0, 50.0]), radius_sink=0.5, crowd_generator=MonotonicCrowd(20.0),
                                   high_level_planner=StubHighLevelPlan((1.0, 0.0)), local_planner=lp,
                                   waypoints=[np.array([12.0, 50.0])], loop_forever=False, agent_eyesight_range=2.0))
    return ids


def test_missing_ids_are_flagged_or_refuse_the_read():
    grid = dict(width=60.0, height=60.0, cell_size=2.0, offset=(0.0, 0.0))
    sim = Simulation(LocationHash2D(**grid))
    heard = _Events()
    sim.add_event_listener(heard)
    ids = _sink_scene(sim)["plain"]
    for _ in range(120):
        sim.step(0.05)
    despawned = [i for k, i in heard.events if k == "destroyed"]
    assert len(despawned) >= 2  # (at the sink)
    removed = [ids[3], ids[77]]
    for i in removed:
        sim.remove_agents(i)
    full = sim.read_agents()
    spawned_alive = [int(i) for i in full["id"] if int(i) > max(ids)]
    assert spawned_alive  # (source-sink agents on their way are found like any other)
    never = [10 ** 9, 2 ** 31 + 5, 2 ** 40 + 1]
    alive = [ids[0], spawned_alive[0], ids[200], ids[5]]
    ask = np.array(alive[:2] + never[:1] + removed + alive[2:] + despawned[:2] + never[1:], dtype=np.uint64)
    got, found = sim.read_agents_by_id(ask, missing_ok=True)
    assert found.tolist() == [i in alive for i in ask.tolist()]
    assert got[found].tobytes() == _rows(full, ask[found]).tobytes()
    zero = np.zeros(int((~found).sum()), dtype=AGENT_DTYPE)
    zero["id"] = ask[~found]
    assert got[~found].tobytes() == zero.tobytes()
    # without `found` the same batch is refused and the output buffer is not written
    with pytest.raises(CrowdSimError, match="unknown agent id"):
        sim.read_agents_by_id(ask)
    out = np.full(len(ask) * AGENT_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    rc = sim._lib.cs_read_agents_by_id(sim._engine, ask.ctypes.data_as(C.POINTER(C.c_uint64)), len(ask),
                                       out.ctypes.data_as(C.POINTER(_abi.AgentView)), None)
    assert rc == 2 and (out == 0xAB).all()
    assert sim.read_agents().tobytes() == full.tobytes()
    sim.step(0.05)  # (not poisoned)


@pytest.mark.parametrize("flags", FLAGS)
def test_one_batched_remove_equals_the_loop_of_single_removes(flags):
    (a, b), _ = _twins(flags)
    for s in (a, b):
        _keep_events(s)
    _steps((a, b), 10)
    batch = np.random.default_rng(23).choice(a.read_agents()["id"], 500, replace=False)
    assert a.remove_agents_by_id(batch) == 500
    for i in batch:
        b.remove_agents(int(i))
    assert len(a) == len(b) == 4096 - 500
    ra = a.read_agents()
    assert ra.tobytes() == b.read_agents().tobytes() and not np.isin(batch, ra["id"]).any()
    ev = _events(a)
    assert ev == _events(b)
    assert ev == [(_abi.CS_EVENT_DESTROYED, 0xFFFFFFFF, int(i)) for i in batch]
    for k in range(20):
        a.step(0.05)
        b.step(0.05)
        assert a.last_report == b.last_report, k
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert _events(a) == _events(b)


class _Leader(HighLevelPlanner):
    """A callback planner that records what the engine tells it."""

    def __init__(self):
        self.removed = []

    def get_desired_velocity(self, agent, time):
        return (0.25, -0.125)

    def remove_agent_id(self, agent_id):
        self.removed.append(int(agent_id))


@pytest.mark.parametrize("flags", FLAGS)
def test_batched_remove_of_sink_agents_and_callback_planner_agents(flags):
    """Spawned agents carry their source-sink in the DESTROYED event; a callback planner hears remove_agent_id in the
    order of the batch."""
    grid = dict(width=60.0, height=60.0, cell_size=2.0, offset=(0.0, 0.0))
    sims, leaders, ids = [], [], None
    for _ in range(2):
        s = Simulation(LocationHash2D(**grid), flags=flags)
        leader = _Leader()
        ids = _sink_scene(s, leader)
        _keep_events(s)
        sims.append(s)
        leaders.append(leader)
    a, b = sims
    _steps((a, b), 25)
    _events(a), _events(b)  # (the spawns so far)
    full = a.read_agents()
    assert full.tobytes() == b.read_agents().tobytes()
    spawned = [int(i) for i in full["id"] if int(i) > max(ids["callback"])]
    assert len(spawned) >= 2
    rng = np.random.default_rng(29)
    batch = np.concatenate([rng.choice(ids["plain"], 60, replace=False), rng.choice(ids["callback"], 15, replace=False),
                            spawned]).astype(np.uint64)
    rng.shuffle(batch)
    a.remove_agents_by_id(batch)
    for i in batch:
        b.remove_agents(int(i))
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    ev = _events(a)
    assert ev == _events(b) and [e[2] for e in ev] == [int(i) for i in batch]
    assert {e[1] for e in ev if e[2] in spawned} == {0} and {e[1] for e in ev if e[2] not in spawned} == {0xFFFFFFFF}
    want = [int(i) for i in batch if int(i) in set(ids["callback"])]
    assert leaders[0].removed == want and leaders[1].removed == want
    _steps((a, b), 20)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert _events(a) == _events(b)


def test_listeners_hear_a_batched_remove():
    (a, b), _ = _twins(0, n=1024)
    heard = [_Events(), _Events()]
    a.add_event_listener(heard[0])
    b.add_event_listener(heard[1])
    _steps((a, b), 3)
    batch = a.read_agents()["id"][::-9]
    a.remove_agents_by_id(batch)
    for i in batch:
        b.remove_agents(int(i))
    assert heard[0].events == heard[1].events == [("destroyed", int(i)) for i in batch]
    assert int(batch[0]) not in a.agents and len(a.agents) == 1024 - len(batch)  # (the cached dict was dropped)


def test_removed_agents_step_like_the_oracle():
    """The same batch removed at once on the engine and one by one on the f64 CPU oracle after 10 steps, then 20 steps:
    ids and counts exact, positions within the project's parity clause (max |p_gpu - p_oracle| / L <= 1e-4, DESIGN.md
    section 6)."""
    pts, pref, group, grid, extent = _crossing(4096)
    gpu, cpu = Simulation(LocationHash2D(**grid)), OracleSimulation(LocationHash2D(**grid))
    for s in (gpu, cpu):
        _add_crossing(s, pts, group)
    _steps((gpu, cpu), 10)
    batch = np.random.default_rng(31).choice(gpu.read_agents()["id"], 500, replace=False)
    gpu.remove_agents_by_id(batch)
    for i in batch:
        cpu.remove_agents(int(i))
    _steps((gpu, cpu), 20)
    g, c = gpu.read_agents(), cpu.read_agents()
    assert len(g) == len(c) == 4096 - 500 and (g["id"] == c["id"]).all()
    err = float(np.hypot(g["x"] - c["x"], g["y"] - c["y"]).max() / extent)
    print(f"batched remove, 20 steps after: max |dp| / L against the oracle = {err:.3e}")
    assert err <= 1e-4


def test_refused_batches_remove_nothing():
    (a, b), _ = _twins(0, n=1024)
    _keep_events(a)
    _steps((a, b), 5)
    base = a.read_agents()
    ids = base["id"]
    gone = int(ids[7])
    a.remove_agents(gone)
    b.remove_agents(gone)
    base = a.read_agents()
    assert _events(a) == [(_abi.CS_EVENT_DESTROYED, 0xFFFFFFFF, gone)]
    cases = [
        (np.concatenate([ids[20:60], [10 ** 9], ids[60:70]]), "unknown agent id"),  # never existed
        (np.concatenate([ids[20:60], [gone]]), "unknown agent id"),                 # already removed
        (np.concatenate([[2 ** 45], ids[20:25]]), "unknown agent id"),
        (np.concatenate([ids[20:60], ids[33:34]]), "twice"),
        (np.array([ids[2], ids[2]]), "twice"),
    ]
    for batch, msg in cases:
        with pytest.raises(CrowdSimError, match=msg):
            a.remove_agents_by_id(batch.astype(np.uint64))
        assert len(a) == len(base) and a.read_agents().tobytes() == base.tobytes(), msg
        assert _events(a) == [], msg
    assert a.remove_agents_by_id([]) == 0
    _steps((a, b), 10)  # not poisoned, and nothing about the next steps changed
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


def test_agents_the_index_refused_are_read_and_removed_by_id():
    (a, b), grid = _twins(0, n=1024)
    for s in (a, b):
        _keep_events(s)
    _steps((a, b), 3)
    for s in (a, b):
        for x in (5.0, 9.0):  # two agents outside the grid: created, then refused by the index (lib.rs:133-149)
            with pytest.raises(CrowdSimError):
                s.add_agents([(grid["width"] * x, 1.0)], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.5)
    full = a.read_agents()
    assert len(full) == 1026 and full.tobytes() == b.read_agents().tobytes()
    limbo = [int(i) for i in full["id"][-2:]]
    ask = np.array([limbo[1], full["id"][10], limbo[0], limbo[1]], dtype=np.uint64)
    assert a.read_agents_by_id(ask).tobytes() == _rows(full, ask).tobytes()
    with pytest.raises(CrowdSimError, match="twice"):
        a.remove_agents_by_id([limbo[0], 3, limbo[0]])
    assert a.read_agents().tobytes() == full.tobytes() and _events(a) == []
    batch = [int(full["id"][10]), limbo[1], int(full["id"][500])]
    a.remove_agents_by_id(batch)
    for i in batch:
        b.remove_agents(i)
    assert len(a) == len(b) == 1023
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    ev = _events(a)
    assert ev == _events(b) and [e[2] for e in ev] == batch
    a.remove_agents_by_id([limbo[0]])  # (the other one would fail every step until it is removed, lib.rs:299-302)
    b.remove_agents(limbo[0])
    _steps((a, b), 5)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


def test_steps_queued_without_a_report_finish_before_a_read_or_a_remove():
    (a, b), _ = _twins(0, n=2048)
    _steps((a, b), 3)
    ids = a.read_agents()["id"][::17]
    _steps((a, b), 7, report=False)  # fire-and-forget
    got = a.read_agents_by_id(ids)
    assert got.tobytes() == _rows(b.read_agents(), ids).tobytes()
    _steps((a, b), 4, report=False)
    a.remove_agents_by_id(ids)
    b.synchronize()
    for i in ids:
        b.remove_agents(int(i))
    _steps((a, b), 5)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


def test_wide_ids_read_and_remove_by_external_id_across_renumberings(monkeypatch):
    """The recipe of tests/test_gpu_wide_ids.py: 10 x 600 ids through a 4096-id device space, so the device ids are
    renumbered between the adds and the batch calls; the external ids (above 2^40) keep naming the same agents."""
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(2 ** 40 + 1))
    monkeypatch.setenv("CS_DEVICE_ID_LIMIT", "4096")
    pts, grid, extent, group = scenes.uniform_crowd(600, seed=9, cell_size=2.0, room=20.0)
    sims = [Simulation(LocationHash2D(**grid), flags=CS_CFG_WIDE_IDS) for _ in range(2)]
    monkeypatch.delenv("CS_DEVICE_ID_LIMIT")
    monkeypatch.delenv("CS_FIRST_AGENT_ID")
    a, b = sims
    for s in sims:
        ids = scenes.add_counterflow(s, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    assert min(ids) > 2 ** 40
    spot = np.array([[extent + 15.0, extent + 15.0]])
    late = []
    for r in range(10):
        for s in sims:
            more = s.add_agents(np.repeat(spot, 600, axis=0) + np.arange(600)[:, None] * 0.01,
                                StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.0)
            s.step(0.05)
        a.remove_agents_by_id(more[:-1])  # (most of the round's agents leave in one batch)
        for i in more[:-1]:
            b.remove_agents(i)
        late.append(more[-1])
        if r in (6, 8):  # ids from before and after the last renumbering, in one batch
            full = a.read_agents()
            ask = np.array([late[-1], ids[0], late[0], ids[5], more[3]], dtype=np.uint64)
            got, found = a.read_agents_by_id(ask, missing_ok=True)
            assert found.tolist() == [True, True, True, True, False]
            assert got[:4].tobytes() == _rows(full, ask[:4]).tobytes()
            assert full.tobytes() == b.read_agents().tobytes()
    assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) >= 1
    n_before = a.kernel_stat(_abi.CS_STAT_RENUMBERINGS)
    batch = np.array([late[0], ids[1], late[-1], ids[300]], dtype=np.uint64)
    a.remove_agents_by_id(batch)
    for i in batch:
        b.remove_agents(int(i))
    assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) == n_before  # (neither call renumbers)
    got = a.read_agents()
    assert got.tobytes() == b.read_agents().tobytes() and not np.isin(batch, got["id"]).any()
    assert len(got) == 600 + 10 - 4
    _steps((a, b), 5)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


def test_batches_beyond_the_lds_staging_limit():
    """100,000 agents: a batch of more than 40,960 ids takes the match that searches the keys in global memory; it
    answers as the staged match answers a 40,000-id prefix, and removes what two staged batches remove."""
    pts, grid, extent, group = scenes.uniform_crowd(100_000, seed=3, cell_size=2.0)
    sims = [Simulation(LocationHash2D(**grid)) for _ in range(2)]
    for s in sims:
        scenes.add_counterflow(s, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    a, b = sims
    _steps((a, b), 3)
    full = a.read_agents()
    ids = np.random.default_rng(37).permutation(full["id"])
    assert len(ids) > 2 * STAGED_KEYS_MAX
    big = a.read_agents_by_id(ids)  # unstaged
    assert big.tobytes() == _rows(full, ids).tobytes()
    assert a.read_agents_by_id(ids[:40_000]).tobytes() == big[:40_000].tobytes()  # staged
    batch = ids[:60_000]
    a.remove_agents_by_id(batch)  # unstaged
    b.remove_agents_by_id(batch[:30_000])  # staged, twice
    b.remove_agents_by_id(batch[30_000:])
    assert len(a) == len(b) == 40_000
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert a.read_agents().tobytes() == _rows(full, np.sort(ids[60_000:])).tobytes()
    got, found = a.read_agents_by_id(ids, missing_ok=True)
    assert (~found[:60_000]).all() and found[60_000:].all()
    _steps((a, b), 5)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()


def test_query_then_remove_clears_the_region_and_the_spawn_probe_sees_it():
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    sim = Simulation(LocationHash2D(**grid))
    lp, hlp = NoLocalPlan(), StubHighLevelPlan((0.0, 0.0))
    p = (10.0, 30.0)
    near = [(10.1, 30.2), (9.8, 29.9), (10.9, 30.4), (11.5, 31.0)]
    far = [(5.0, 5.0), (30.0, 30.0), (20.0, 12.0)]
    ids = sim.add_agents(near + far, hlp, lp, 1.0)
    sim.add_source_sink(SourceSink(source=np.array(p), radius_sink=0.5, crowd_generator=MonotonicCrowd(20.0),
                                   high_level_planner=hlp, local_planner=lp, waypoints=[np.array([10.0, 35.0])],
                                   loop_forever=False, agent_eyesight_range=1.0))
    sim.step(0.05)
    assert sim.last_report["n_spawned"] == 0  # (the spot is taken)
    found = sim.get_neighbours_in_radius(2.5, p)
    assert sorted(found) == sorted(ids[:4])
    rows = sim.read_agents_by_id(found)
    assert (np.hypot(rows["x"] - p[0], rows["y"] - p[1]) <= 2.5).all()
    sim.remove_agents_by_id(found)
    assert sim.get_neighbours_in_radius(2.5, p) == []
    assert sorted(int(i) for i in sim.read_agents()["id"]) == sorted(ids[4:])
    sim.step(0.05)
    assert sim.last_report["n_spawned"] == 1  # the probe (lib.rs:214) sees the spot free


def test_device_bytes_count_the_batch_buffers():
    (a, _), _ = _twins(0, n=1024)
    _steps((a,), 2)
    before = a.device_bytes
    ids = a.read_agents()["id"]
    a.read_agents_by_id(ids)
    grown = a.device_bytes
    assert grown >= before + len(ids) * (4 + 4 + 4 + 32)  # keys, slots, count and meta words, records
    a.read_agents_by_id(ids[:10])
    a.remove_agents_by_id(ids[:10])
    assert a.device_bytes == grown  # (kept and shared, not grown per call)


def test_cpp_read_and_remove_by_id():
    from test_gpu_cpp_api import build_cpp_test
    out = subprocess.run([build_cpp_test("test_agents_by_id")], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "agents by id: passed" in out.stdout


def test_the_oracle_has_no_read_or_remove_by_id():
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="needs the HIP engine"):
        sim.read_agents_by_id([0])
    with pytest.raises(CrowdSimError, match="needs the HIP engine"):
        sim.remove_agents_by_id([0])
