"""Sending agents to goals by id in batches (include/crowdstep_state.h, cs_set_targets) without a GPU: the header, the
binding table and the constants agree, the HIP library exports both entry points with the bound signatures, the C++
mirror compiles, a library without the state header (the test oracle) says so, and the host-side follower that the GPU
parity tests use as their reference (tests/host_follower.py) is pinned against the oracle's own route follower."""
import ctypes
import os
import re

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_TARGETS = ("cs_set_targets", "cs_mesh_set_targets")
STATUSES = ("IGNORED", "BOOKED", "PLANNED", "NO_PATH", "FORWARDED")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_set_targets():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    for name in SET_TARGETS:
        assert name in declared and name in _abi.STATE_SYMBOLS and name not in _abi.SYMBOLS, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    C = ctypes
    want = (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.c_size_t, C.c_double, C.c_double,
                      C.POINTER(C.c_uint8)])
    for name in SET_TARGETS:
        assert _abi.STATE_SYMBOLS[name] == want
    crowdstep = open(os.path.join(ROOT, "include", "crowdstep.h")).read()
    assert "set_targets" not in crowdstep and "CS_TARGET_" not in crowdstep


def test_the_status_constants_agree_with_the_header():
    defined = dict(re.findall(r"#define\s+CS_TARGET_([A-Z_]+)\s+(\d+)u", _header()))
    assert sorted(defined) == sorted(STATUSES)
    for name in STATUSES:
        assert getattr(_abi, "CS_TARGET_" + name) == int(defined[name]), name
    assert [getattr(_abi, "CS_TARGET_" + n) for n in STATUSES] == [0, 1, 2, 3, 4]
    import host_follower
    assert (host_follower.BOOKED, host_follower.PLANNED, host_follower.NO_PATH) == \
        (_abi.CS_TARGET_BOOKED, _abi.CS_TARGET_PLANNED, _abi.CS_TARGET_NO_PATH)


def test_hip_library_exports_set_targets():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    assert _abi.STATE_SYMBOLS["cs_set_targets_device_hits"] == (ctypes.c_uint64, [ctypes.c_void_p])
    for name in SET_TARGETS + ("cs_set_targets_device_hits",):
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_cpp_mirror_with_set_targets_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_set_targets"))


def test_oracle_does_not_pretend_to_set_targets(oracle_lib):
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import CrowdSimError, LocationHash2D
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="set_targets needs the HIP engine"):
        sim.set_targets([0], [(1.0, 1.0)])


def test_route_follower_set_target_names_the_batched_call_when_it_cannot_forward(oracle_lib):
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import CrowdSimError, LocationHash2D, NoLocalPlan, RouteFollower
    from rmf_crowdsim_amd.simulation import Agent
    hlp = RouteFollower(lambda s, g: [s, g])
    agent = Agent(0, np.zeros(2), np.zeros(2), 0, 2.0)
    with pytest.raises(CrowdSimError, match="Simulation.set_targets"):  # registered with nobody
        hlp.set_target(agent, (1.0, 1.0), (0.0, 0.0))
    sims = [OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0))) for _ in range(2)]
    sims[0].add_agents([(1.0, 1.0)], hlp, NoLocalPlan(), 2.0)
    with pytest.raises(CrowdSimError, match="set_targets needs the HIP engine"):  # forwarded: one simulation
        hlp.set_target(agent, (1.0, 1.0), (0.0, 0.0))
    sims[1].add_agents([(1.0, 1.0)], hlp, NoLocalPlan(), 2.0)
    with pytest.raises(CrowdSimError, match="registered with 2 simulations.*Simulation.set_targets"):
        hlp.set_target(agent, (1.0, 1.0), (0.0, 0.0))


def test_goal_batches_must_match_their_ids():
    from rmf_crowdsim_amd import CrowdSimError
    from rmf_crowdsim_amd.simulation import set_targets_by_id
    with pytest.raises(CrowdSimError, match="2 ids but 1 goals"):
        set_targets_by_id(None, None, [1, 2], [(0.0, 0.0)], (0.0, 0.0))


def test_spatial_hash_rounds_ties_away_from_zero():
    from host_follower import spatial_hash
    assert [spatial_hash(v, 4.0) for v in (0.0, 1.9, 2.0, 5.9, 6.0, -2.0, -1.9, -6.0)] == [0, 0, 1, 1, 2, -1, 0, -2]
    assert spatial_hash(0.49999999999999994, 1.0) == 0 and spatial_hash(0.5, 1.0) == 1


# ---- the pin of tests/host_follower.py: as a host planner behind the oracle's callback path it moves every agent
# exactly as the oracle's own CS_HLP_ROUTE does (positions, counts, events, and the plan_route calls) ----
def test_host_follower_equals_the_oracles_route_follower_on_the_kat_scene(oracle_lib):
    import rmf_crowdsim_amd
    from host_follower import HostFollower
    from oracle_sim import OracleSimulation
    from test_oracle_reference_kats import run_route_follower_kat
    ref = run_route_follower_kat(OracleSimulation).read_agents()
    keep = rmf_crowdsim_amd.RouteFollower
    rmf_crowdsim_amd.RouteFollower = HostFollower  # (the scene takes its follower from the package)
    try:
        got = run_route_follower_kat(OracleSimulation).read_agents()
    finally:
        rmf_crowdsim_amd.RouteFollower = keep
    assert len(ref) > 1 and got.tobytes() == ref.tobytes()


def test_host_follower_equals_the_oracles_route_follower_step_by_step_on_the_kat_scene(oracle_lib):
    """run_route_follower_kat's scene again, with what that function does not return: the crowd after every step, the
    per-step counts and the plan_route log."""
    from host_follower import HostFollower
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import LocationHash2D, MonotonicCrowd, NoLocalPlan, RouteFollower, SourceSink
    from test_oracle_reference_kats import DoglegRoutes

    def run(follower):
        routes = DoglegRoutes()
        sim = OracleSimulation(LocationHash2D(100.0, 100.0, 2.0, (-50.0, -50.0)))
        sim.add_source_sink(SourceSink((0.0, 0.0), 1.0, MonotonicCrowd(10.0), follower(routes, scale=1.0), NoLocalPlan(),
                                       [(10.0, 0.0)], False, 2.0))
        sim.add_agents([(-20.0, -20.0)], follower(routes, scale=1.0), NoLocalPlan(), 2.0)
        frames, counts = [], []
        for _ in range(151):
            sim.step(0.1)
            r = sim.last_report
            frames.append(sim.read_agents().tobytes())
            counts.append((len(sim), r["n_spawned"], r["n_destroyed"], r["n_waypoint_hits"]))
        return frames, counts, routes.calls
    got, want = run(HostFollower), run(RouteFollower)
    assert got[1] == want[1] and sum(c[2] for c in want[1]) >= 10 and sum(c[3] for c in want[1]) >= 10
    assert got[2] == want[2] == [((0.0, 0.0), (10.0, 0.0))]
    assert got[0] == want[0]


def test_host_follower_equals_the_oracles_route_follower_on_the_dogleg_stream(oracle_lib):
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import RouteFollower
    from set_targets_scenes import run_stream
    a = run_stream(OracleSimulation, True, resend=())
    b = run_stream(OracleSimulation, True, resend=(), follower=RouteFollower)
    ra, rb = a.sim.read_agents(), b.sim.read_agents()
    print(f"{len(ra)} alive, {sum(c[2] for c in a.counts)} destroyed, {sum(c[3] for c in a.counts)} waypoint hits, "
          f"{len(a.routes.calls)} routes")
    assert len(ra) > 1000 and sum(c[2] for c in a.counts) > 200 and len(a.routes.calls) > 16
    assert ra.tobytes() == rb.tobytes()
    assert a.counts == b.counts and a.routes.calls == b.routes.calls
    assert a.listener.added == b.listener.added and a.listener.removed == b.listener.removed
    assert set(a.hlp.statuses) == {1, 2}  # the spawns and waypoints of the stream: planned once, then booked
