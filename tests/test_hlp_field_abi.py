"""The flow-field high-level planner (include/crowdstep_state.h, cs_register_hlp_field) without a GPU: the header declares
the four entry points and the binding table binds them, the cross-compiled library exports them, the C++ mirror compiles,
FieldPlanner.get_desired_velocity gives hand-computed values of the rule, the f64 oracle steps a crowd with a FieldPlanner
through the callback fallback, and flow_field_to_goals leads every free bin downhill to the goal."""
import ctypes
import math
import os
import re

import numpy as np

from rmf_crowdsim_amd import (Agent, FieldPlanner, LocationHash2D, NoLocalPlan, _abi, _native, flow_field_to_goals)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cs_register_hlp_field", "cs_hlp_field_update", "cs_mesh_register_hlp_field", "cs_mesh_hlp_field_update")
NAN = float("nan")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_field_planner_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    for name in CALLS:
        assert name in declared and name in _abi.STATE_SYMBOLS and name not in _abi.SYMBOLS, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    reg = (C.c_uint32, [C.c_void_p, C.POINTER(_abi.FieldDesc), C.c_uint32, C.POINTER(C.c_float)])
    upd = (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)])
    assert [_abi.STATE_SYMBOLS[n] for n in CALLS] == [reg, upd, reg, upd]
    for name, value in (("CS_HLP_FIELD", 5), ("CS_HLP_FIELD_NEAREST", 0), ("CS_HLP_FIELD_BILINEAR", 1),
                        ("CS_STAT_HLP_FIELD_LAUNCHES", 8)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"u\b", _header()), name
        assert getattr(_abi, name) == value
    assert "Flow-field high-level planner" in _header()
    # crowdstep.h, which the oracle and the Rust shim mirror, knows nothing of it
    assert "hlp_field" not in open(os.path.join(ROOT, "include", "crowdstep.h")).read().lower()


def test_hip_library_exports_the_field_planner_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in CALLS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_cpp_mirror_with_the_field_planner_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_hlp_field"))


def _at(planner, x, y):
    return planner.get_desired_velocity(Agent(0, np.array([x, y], dtype=np.float64), np.zeros(2), 0, 0.0), None)


def _raster():
    """4 x 3 bins of 2.0 x 0.5 from (10, -1): vx = 1 + ix + 10 * iy, vy = -(that); values exact in f32"""
    v = np.zeros((3, 4, 2), dtype=np.float32)
    for iy in range(3):
        for ix in range(4):
            v[iy, ix] = (1.0 + ix + 10.0 * iy, -(1.0 + ix + 10.0 * iy))
    return (10.0, -1.0), (2.0, 0.5), v


def test_the_rule_on_hand_cases():
    origin, cell, v = _raster()
    near, lin = FieldPlanner(origin, cell, v, "nearest"), FieldPlanner(origin, cell, v, "bilinear")
    # a bin-centre sample is returned exactly, by both samplings (tx = ty = 0 at a centre)
    for ix in range(4):
        for iy in range(3):
            c = (10.0 + 2.0 * (ix + 0.5), -1.0 + 0.5 * (iy + 0.5))
            want = (float(v[iy, ix, 0]), float(v[iy, ix, 1]))
            assert _at(near, *c) == want and _at(lin, *c) == want, (ix, iy)
    # a point on an inner bin edge takes the upper bin; the low edge of the raster is inside, the high edge outside
    assert _at(near, 12.0, -0.75) == (2.0, -2.0) and _at(near, math.nextafter(12.0, 0.0), -0.75) == (1.0, -1.0)
    assert _at(near, 11.0, -0.5) == (11.0, -11.0)
    assert _at(near, 10.0, -1.0) == (1.0, -1.0)
    for p in (near, lin):
        assert _at(p, 10.0 + 4 * 2.0, 0.0) is None and _at(p, 11.0, -1.0 + 3 * 0.5) is None
        assert _at(p, math.nextafter(18.0, 0.0), 0.49) is not None  # (18 - 2^-48 - 10 is exact: fx < 4)
        assert _at(p, math.nextafter(10.0, 0.0), 0.0) is None and _at(p, 11.0, -1.5) is None
        assert _at(p, NAN, 0.0) is None and _at(p, 11.0, float("inf")) is None and _at(p, float("-inf"), 0.0) is None
    # bilinear between four centres: fx = 1.75, fy = 1.25 -> i0 = 1, tx = 0.25, j0 = 0, ty = 0.75
    x, y = 10.0 + 2.0 * 1.75, -1.0 + 0.5 * 1.25
    a, b = 2.0 + (3.0 - 2.0) * 0.25, 12.0 + (13.0 - 12.0) * 0.25
    r = a + (b - a) * 0.75
    assert _at(lin, x, y) == (float(np.float32(r)), float(np.float32(-r))) == (9.75, -9.75)
    # bilinear clamps at an edge: left of the first centre along x (ax < 0: tx = 0), beyond the last along y (j1 = j0)
    assert _at(lin, 10.5, -1.0 + 0.5 * 1.25) == (1.0 + (11.0 - 1.0) * 0.75, -(1.0 + (11.0 - 1.0) * 0.75))
    assert _at(lin, 10.0 + 2.0 * 1.75, 0.45) == (22.25, -22.25)
    assert _at(lin, 17.9, 0.49) == (24.0, -24.0) and _at(lin, 10.0, -1.0) == (1.0, -1.0)
    # the result is rounded to f32 once
    w = v.copy()
    w[0, 0, 0], w[0, 1, 0] = 1.0, 1.0 + 2.0 ** -23
    got = _at(FieldPlanner(origin, cell, w, "bilinear"), 10.0 + 2.0 * 0.75, -0.75)  # tx = 0.25, ty = 0
    assert got[0] == float(np.float32(1.0 + 2.0 ** -23 * 0.25)) == 1.0
    # a NaN corner falls back to the agent's own bin; a NaN own bin is None under both samplings
    w = v.copy()
    w[1, 2] = (NAN, 5.0)
    holed_near, holed_lin = FieldPlanner(origin, cell, w, "nearest"), FieldPlanner(origin, cell, w, "bilinear")
    assert _at(holed_lin, x, y) == (12.0, -12.0)         # own bin (1, 1), corner (2, 1) is NaN
    assert _at(holed_lin, 13.5, -0.8) == (2.25, -2.25)   # own bin (1, 0): fy = 0.4, j0 = j1 = 0, no NaN among the four ...
    assert _at(holed_lin, 13.5, -0.7) == (2.0, -2.0)     # ... own bin (1, 0): fy = 0.6, j1 = 1, corner (2, 1) is NaN
    assert _at(holed_lin, 15.0, -0.25) is None and _at(holed_near, 15.0, -0.25) is None  # the centre of (2, 1)
    assert _at(holed_lin, 14.1, -0.45) is None
    w[1, 2] = (5.0, NAN)
    assert _at(FieldPlanner(origin, cell, w, "nearest"), 15.0, -0.25) is None
    assert _at(holed_lin, 11.0, -0.75) == (1.0, -1.0)    # far from the hole: untouched
    # update keeps the raster and replaces the values; another shape is refused
    near.update(-v)
    assert _at(near, 11.0, -0.75) == (-1.0, 1.0)
    try:
        near.update(v[:2])
    except Exception as err:  # noqa: BLE001
        assert "vectors has shape" in str(err)
    else:
        raise AssertionError("an update of another shape was taken")
    # the host form follows the planner
    host = near.as_host_planner()
    assert _at(host, 11.0, -0.75) == (-1.0, 1.0) and not hasattr(host, "_bound")


def test_the_oracle_steps_a_crowd_that_follows_a_rotating_field(oracle_lib):
    """The reference path without a GPU: on a library without cs_register_hlp_field the planner registers as a host
    callback planner.  The crowd walks round the centre of a rotating field, step for step what the rule says."""
    from oracle_sim import OracleSimulation
    n, cell, omega, dt, steps = 64, 0.25, 0.5, 0.05, 40
    centres = (np.arange(n) + 0.5) * cell
    v = np.zeros((n, n, 2), dtype=np.float32)
    v[..., 0] = -omega * (centres[:, None] - 8.0)  # (-omega * (y - cy), omega * (x - cx))
    v[..., 1] = omega * (centres[None, :] - 8.0)
    planner = FieldPlanner((0.0, 0.0), cell, v, "bilinear")
    calls = []
    rule = planner.get_desired_velocity
    planner.get_desired_velocity = lambda agent, time: (calls.append(1), rule(agent, time))[1]
    sim = OracleSimulation(LocationHash2D(16.0, 16.0, 1.0, (0.0, 0.0)))
    angles = np.linspace(0.0, 2.0 * np.pi, 24, endpoint=False)
    pts = np.column_stack([8.0 + 3.0 * np.cos(angles), 8.0 + 3.0 * np.sin(angles)])
    ids = sim.add_agents(pts, planner, NoLocalPlan(), 1.0)
    assert not planner._bound  # (no device registration: the callback descriptor)
    want = pts.copy()
    for _ in range(steps):
        vel = np.array([_at(planner, *p) for p in want])
        want = want + vel * dt
        sim.step(dt)
    assert len(calls) >= steps * len(pts)
    rec = sim.read_agents()
    assert rec["id"].tolist() == ids
    got = np.column_stack([rec["x"], rec["y"]])
    assert np.abs(got - want).max() <= 1e-12
    # ... which is a rotation by omega * t: the radius kept to the order of the Euler step, the angle advanced
    radius = np.hypot(got[:, 0] - 8.0, got[:, 1] - 8.0)
    turned = np.mod(np.arctan2(got[:, 1] - 8.0, got[:, 0] - 8.0) - angles, 2.0 * np.pi)
    assert np.abs(radius - 3.0).max() < 0.05 and np.abs(turned - omega * dt * steps).max() < 0.02


def test_flow_field_to_goals_leads_downhill_round_a_wall():
    ny, nx, speed = 7, 9, 1.25
    blocked = np.zeros((ny, nx), dtype=bool)
    blocked[:, 4] = True
    blocked[5, 4] = False      # the gap
    blocked[0:2, 0:2] = True
    blocked[0, 0] = False      # a free bin nobody can reach (its three neighbours are blocked)
    goals = np.zeros((ny, nx), dtype=bool)
    goals[1, 8] = True
    cell = (1.5, 1.0)
    field, dist = flow_field_to_goals(blocked, goals, (3.0, -2.0), cell, speed, return_distance=True)
    assert field.shape == (ny, nx, 2) and field.dtype == np.float32
    unreachable = ~blocked & ~np.isfinite(dist)
    assert unreachable.tolist() == (np.arange(ny)[:, None] == 0).__and__(np.arange(nx)[None, :] == 0).tolist()
    assert np.array_equal(np.isnan(field).any(axis=2), blocked | unreachable)
    assert np.array_equal(np.isnan(field).all(axis=2), blocked | unreachable)
    assert field[1, 8].tolist() == [0.0, 0.0] and dist[1, 8] == 0.0
    free = ~blocked & ~unreachable & ~goals
    assert free.sum() > 40
    for iy, ix in zip(*np.nonzero(free)):
        vx, vy = (float(c) for c in field[iy, ix])
        assert abs(math.hypot(vx, vy) - speed) < 1e-6, (ix, iy)
        dx, dy = int(np.sign(round(vx / cell[0], 6))), int(np.sign(round(vy / cell[1], 6)))
        unit = np.array([dx * cell[0], dy * cell[1]]) / math.hypot(dx * cell[0], dy * cell[1])
        assert np.abs(np.array([vx, vy]) - speed * unit).max() < 1e-6, (ix, iy)  # it points AT a neighbour's centre
        jx, jy = ix + dx, iy + dy
        assert 0 <= jx < nx and 0 <= jy < ny and not blocked[jy, jx], (ix, iy)
        assert dist[jy, jx] < dist[iy, ix], (ix, iy)  # ... which is strictly closer to the goal
    # everybody left of the wall goes through the gap: the bin in front of it points into it
    assert field[5, 3].tolist() == [speed, 0.0] and field[5, 4].tolist() == [speed, 0.0]
    # the planner takes the vectors as they come
    planner = FieldPlanner((3.0, -2.0), cell, field, "nearest")
    assert _at(planner, 3.0 + 1.5 * 4.5, -2.0 + 0.5) is None and _at(planner, 3.0 + 1.5 * 3.5, -2.0 + 5.5) == (speed, 0.0)
