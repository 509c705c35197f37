"""Solving a flow field on the device (include/crowdstep_state.h, cs_flow_field_solve) without a GPU: the header declares the
two calls and the binding table binds them with the header's argument lists, the cross-compiled library exports them, the
structs have the C layout, the C++ mirror compiles; and the rule itself: the tests' restatement (sweeps to the fixed point,
tests/flow_solve_reference.py) gives closed forms typed in by hand, equals the package's heap Dijkstra
(flow_field_solve_host) bit for bit, and its distances equal flow_field_to_goals bit for bit on the cells where numpy's
hypot equals sqrt(w * w + h * h)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import flow_solve_reference as ref
from rmf_crowdsim_amd import _abi, _native, flow_field_solve_host, flow_field_to_goals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cs_flow_field_solve", "cs_mesh_flow_field_solve")
INF, NAN = float("inf"), float("nan")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_flow_solve_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    for name in CALLS:
        assert name in declared and name in _abi.STATE_SYMBOLS and name not in _abi.SYMBOLS, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    want = (C.c_int, [C.c_void_p, C.POINTER(_abi.FlowDesc), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_double),
                      C.POINTER(_abi.FlowStats)])
    assert [_abi.STATE_SYMBOLS[n] for n in CALLS] == [want, want]
    for name, handle in zip(CALLS, ("cs_engine", "cs_mesh")):
        args = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text).group(1)
        assert [re.sub(r"\s+", " ", a.strip()) for a in args.split(",")] == [
            handle + "*", "const cs_flow_desc*", "uint32_t hlp", "float* out_vxy", "double* out_dist", "cs_flow_stats*"]
    assert "Solving a flow field on the device" in _header()
    assert re.search(r"#define\s+CS_ABI_VERSION\s+1u?\b", open(os.path.join(ROOT, "include", "crowdstep.h")).read())
    # crowdstep.h, which the oracle and the Rust shim mirror, knows nothing of it
    assert "flow_field" not in open(os.path.join(ROOT, "include", "crowdstep.h")).read().lower()


def test_hip_library_exports_the_flow_solve_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in CALLS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_structs_have_the_layout_of_the_c_structs(tmp_path):
    desc = [f for f, _ in _abi.FlowDesc._fields_]
    stats = [f for f, _ in _abi.FlowStats._fields_]
    assert desc == ["raster", "goals", "blocked", "slowness", "speed", "density_weight", "density_filter"]
    assert stats == ["reached", "rounds", "reserved"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n%zu\\n", sizeof(cs_flow_desc), sizeof(cs_flow_stats));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_flow_desc, {f}));\n' for f in desc)
                   + "".join(f'  printf("%zu\\n", offsetof(cs_flow_stats, {f}));\n' for f in stats)
                   + '  printf("%zu\\n%zu\\n", sizeof(cs_field_desc), sizeof(cs_selection));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.FlowDesc) == 88 and got[1] == ctypes.sizeof(_abi.FlowStats) == 16
    assert got[2:9] == [getattr(_abi.FlowDesc, f).offset for f in desc] == [0, 40, 48, 56, 64, 72, 80]
    assert got[9:12] == [getattr(_abi.FlowStats, f).offset for f in stats] == [0, 8, 12]
    assert got[12:] == [ctypes.sizeof(_abi.FieldDesc), ctypes.sizeof(_abi.Selection)] == [40, 104]  # (untouched)


def test_cpp_mirror_with_the_flow_solve_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_flow_solve"))


# ---- the rule, on hand cases --------------------------------------------------------------------------------------------

def _both(blocked, goals, cell, speed, **how):
    """the restatement's answer, after checking that the package's host solver gives the same bytes"""
    vec, dist, reached, _ = ref.solve(blocked, goals, cell, speed, **how)
    hvec, hdist = flow_field_solve_host(blocked, goals, cell, speed, **how)
    assert dist.tobytes() == hdist.tobytes() and vec.tobytes() == hvec.tobytes()
    assert reached == int(np.isfinite(hdist).sum())
    return vec, dist, reached


def _f32(v):
    return float(np.float32(v))


def test_an_open_3_by_3_raster_gives_the_three_lengths():
    cw, ch, speed = 0.3, 0.7, 1.25
    goals = np.zeros((3, 3), dtype=bool)
    goals[1, 1] = True
    vec, dist, reached = _both(None, goals, (cw, ch), speed)
    diag = math.sqrt(cw * cw + ch * ch)
    assert dist.tolist() == [[diag, ch, diag], [cw, 0.0, cw], [diag, ch, diag]] and reached == 9
    assert vec[1, 1].tolist() == [0.0, 0.0]
    assert vec[1, 0].tolist() == [_f32(speed * cw / cw), 0.0] and vec[1, 2].tolist() == [_f32(speed * -cw / cw), 0.0]
    assert vec[0, 1].tolist() == [0.0, _f32(speed * ch / ch)] and vec[2, 1].tolist() == [0.0, _f32(speed * -ch / ch)]
    assert vec[0, 0].tolist() == [_f32(speed * cw / diag), _f32(speed * ch / diag)]
    assert vec[2, 2].tolist() == [_f32(speed * -cw / diag), _f32(speed * -ch / diag)]
    assert vec[0, 2].tolist() == [_f32(speed * -cw / diag), _f32(speed * ch / diag)]


def test_a_wall_corner_forces_the_two_step_detour():
    cw, ch = 0.5, 0.25
    goals = np.zeros((2, 2), dtype=bool)
    goals[0, 0] = True
    blocked = np.zeros((2, 2), dtype=bool)
    blocked[0, 1] = True  # beside the diagonal from (1, 1) to (0, 0): nobody cuts its corner
    vec, dist, reached = _both(blocked, goals, (cw, ch), 1.0)
    assert dist.tolist() == [[0.0, INF], [ch, ch + cw]] and reached == 3
    assert vec[1, 1].tolist() == [-1.0, 0.0] and vec[1, 0].tolist() == [0.0, -1.0]
    assert np.isnan(vec[0, 1]).all()
    # without the wall the diagonal is taken
    _, open_dist, _ = _both(None, goals, (cw, ch), 1.0)
    assert open_dist[1, 1] == math.sqrt(cw * cw + ch * ch) < ch + cw


def test_a_sealed_pocket_a_blocked_goal_no_goal_and_all_goals():
    cell = (0.5, 0.5)
    blocked = np.zeros((5, 5), dtype=bool)
    blocked[1:4, 1:4] = True
    blocked[2, 2] = False  # the pocket
    goals = np.zeros((5, 5), dtype=bool)
    goals[0, 0] = True
    goals[1, 1] = True  # blocked: ignored
    vec, dist, reached = _both(blocked, goals, cell, 1.0)
    assert dist[2, 2] == INF and np.isnan(vec[2, 2]).all() and dist[1, 1] == INF and np.isnan(vec[1, 1]).all()
    assert reached == 16 and np.isfinite(dist[~blocked]).sum() == 16
    assert dist[4, 4] == 0.5 * 8  # round the block: no diagonal at its corners
    # a goal inside the pocket reaches nobody else
    only = np.zeros((5, 5), dtype=bool)
    only[2, 2] = True
    vec, dist, reached = _both(blocked, only, cell, 1.0)
    assert reached == 1 and dist[2, 2] == 0.0 and vec[2, 2].tolist() == [0.0, 0.0] and np.isnan(vec[0, 0]).all()
    # no goal at all
    vec, dist, reached = _both(blocked, np.zeros((5, 5), dtype=bool), cell, 1.0)
    assert reached == 0 and np.isinf(dist).all() and np.isnan(vec).all()
    # every bin a goal
    vec, dist, reached = _both(None, np.ones((4, 6), dtype=bool), cell, 1.0)
    assert reached == 24 and not dist.any() and not vec.any() and not np.signbit(vec).any()


def test_the_first_step_in_order_breaks_a_tie():
    # goals left and right of the middle column at equal distance: step (-1, 0) comes before (1, 0)
    goals = np.zeros((1, 3), dtype=bool)
    goals[0, 0] = goals[0, 2] = True
    vec, dist, _ = _both(None, goals, (0.5, 0.5), 2.0)
    assert dist.tolist() == [[0.0, 0.5, 0.0]] and vec[0, 1].tolist() == [-2.0, 0.0]
    # goals in all four corners of a 3 x 3 raster: the middle takes the first diagonal, (-1, -1)
    goals = np.zeros((3, 3), dtype=bool)
    goals[0, 0] = goals[0, 2] = goals[2, 0] = goals[2, 2] = True
    vec, dist, _ = _both(None, goals, (0.5, 0.5), 1.0)
    assert vec[1, 1].tolist() == [_f32(-0.5 / math.sqrt(0.5)), _f32(-0.5 / math.sqrt(0.5))]
    # ... and the top edge's middle, between two goals at cell_w, goes left; above and below at cell_h, down (dy = -1)
    assert vec[0, 1].tolist() == [-1.0, 0.0] and vec[1, 0].tolist() == [0.0, -1.0]


def test_slowness_in_one_column_doubles_that_columns_step_costs():
    cw, ch = 0.5, 0.25
    goals = np.zeros((1, 5), dtype=bool)
    goals[0, 0] = True
    slow = np.ones((1, 5), dtype=np.float32)
    slow[0, 2] = 2.0
    _, dist, _ = _both(None, goals, (cw, ch), 1.0, slowness=slow)
    # a step costs the slowness of the bin the walker LEAVES: only the step out of column 2 is doubled
    assert dist.tolist() == [[0.0, cw, cw + 2 * cw, cw + 2 * cw + cw, cw + 2 * cw + cw + cw]]
    # the same through the density term: 4 agents at weight 0.25 double the bin
    counts = np.zeros((1, 5), dtype=np.uint32)
    counts[0, 2] = 4
    _, dense, _ = _both(None, goals, (cw, ch), 1.0, counts=counts, density_weight=0.25)
    assert dense.tobytes() == dist.tobytes()
    # slowness zero: free steps (the distances are promised, not progress)
    slow[0, 1:] = 0.0
    _, free, _ = _both(None, goals, (cw, ch), 1.0, slowness=slow)
    assert free.tolist() == [[0.0] * 5]


CASES = {"issue": ref.issue_case, "serpentine": lambda: ref.serpentine(12, 30, 3), "spiral": lambda: ref.spiral(19)}


@pytest.mark.parametrize("cell", [(0.5, 0.5), (0.5, 0.25), (0.3, 0.7)], ids=str)
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_restatement_equals_the_host_solver_and_flow_field_to_goals(case, cell):
    assert float(np.hypot(cell[0], cell[1])) == float(np.sqrt(np.float64(cell[0]) * cell[0] + np.float64(cell[1]) * cell[1]))
    blocked, goals = CASES[case]()
    _, dist, reached = _both(blocked, goals, cell, 1.3)
    _, old = flow_field_to_goals(blocked, goals, (0.0, 0.0), cell, 1.3, return_distance=True)
    assert dist.tobytes() == old.tobytes()
    free = int((~blocked).sum())
    assert (reached, free) == (2088, 2192) if case == "issue" else reached == free
    # with a random slowness and a density the two solvers still agree (flow_field_to_goals knows neither)
    rng = np.random.default_rng(7)
    slow = rng.uniform(0.5, 4.0, blocked.shape).astype(np.float32)
    counts = rng.integers(0, 5, blocked.shape).astype(np.uint32)
    _, heavy, _ = _both(blocked, goals, cell, 1.3, slowness=slow, counts=counts, density_weight=0.25)
    assert (heavy[np.isfinite(heavy)] >= 0.5 * dist[np.isfinite(dist)]).all() and heavy.tobytes() != dist.tobytes()


def test_the_host_solver_refuses_what_the_device_refuses():
    from rmf_crowdsim_amd import CrowdSimError
    goals = np.ones((2, 2), dtype=bool)
    bad = np.ones((2, 2), dtype=np.float32)
    for how in (dict(speed=NAN), dict(speed=-1.0), dict(density_weight=-0.5, counts=np.zeros((2, 2))),
                dict(density_weight=2.0 ** 33, counts=np.zeros((2, 2))), dict(density_weight=1.0),
                dict(slowness=bad * NAN), dict(slowness=bad * INF), dict(slowness=-bad), dict(slowness=bad[:1])):
        how = dict(how)
        speed = how.pop("speed", 1.0)
        with pytest.raises(CrowdSimError):
            flow_field_solve_host(None, goals, 0.5, speed, **how)
