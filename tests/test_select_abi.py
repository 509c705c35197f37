"""Selecting agents (include/crowdstep_state.h) without a GPU: the header declares the six entry points and the binding
table binds them with these signatures, the cross-compiled library exports them, the ctypes Selection has the layout of
the C struct, the C++ mirror compiles, a library without the state header says so, and the numpy restatement of the
rules (tests/select_reference.py), which the GPU tests compare the engine with, holds on hand cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import Selection, _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE
from select_reference import NO_SINK, pred, selection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT = ("cs_select_agents", "cs_count_agents", "cs_remove_selected", "cs_mesh_select_agents", "cs_mesh_count_agents",
          "cs_mesh_remove_selected")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_selection_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    for name in SELECT:
        assert name in declared and name in _abi.STATE_SYMBOLS, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    C = ctypes
    sel, ids = C.POINTER(_abi.Selection), C.POINTER(C.c_uint64)
    for name in ("cs_select_agents", "cs_remove_selected", "cs_mesh_select_agents", "cs_mesh_remove_selected"):
        assert _abi.STATE_SYMBOLS[name] == (C.c_size_t, [C.c_void_p, sel, ids, C.c_size_t]), name
    for name in ("cs_count_agents", "cs_mesh_count_agents"):
        assert _abi.STATE_SYMBOLS[name] == (C.c_int, [C.c_void_p, sel, C.c_size_t, ids]), name
    # the constants of the header and of the bindings agree
    for name, value in re.findall(r"#define (CS_SEL_[A-Z_]+|CS_SELECT_MAX)\s+(\d+)u", _header()):
        assert getattr(_abi, name) == int(value), name
    assert {n for n, _ in re.findall(r"#define (CS_SEL_[A-Z_]+)\s+(\d+)u", _header())} == {
        "CS_SEL_RECT", "CS_SEL_CIRCLE", "CS_SEL_SOURCE_SINK", "CS_SEL_HLP", "CS_SEL_LP", "CS_SEL_WAYPOINT", "CS_SEL_SPEED"}
    assert _abi.CS_SELECT_MAX == 1024


def test_hip_library_exports_the_selection_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in SELECT:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_selection_has_the_layout_of_the_c_struct(tmp_path):
    names = [f for f, _ in _abi.Selection._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cs_selection));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_selection, {f}));\n' for f in names)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.Selection) == 104
    assert got[1:] == [getattr(_abi.Selection, f).offset for f in names]
    fields = re.search(r"typedef struct cs_selection \{(.*?)\} cs_selection;", _header(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", fields) == names  # (every field of the struct, in order)


def test_cpp_mirror_with_the_selection_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_select"))


def test_oracle_does_not_pretend_to_select(oracle_lib):
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import CrowdSimError, LocationHash2D
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="select_agents needs the HIP engine"):
        sim.select_agents(rect=(0.0, 0.0, 1.0, 1.0))
    with pytest.raises(CrowdSimError, match="count_agents needs the HIP engine"):
        sim.count_agents([Selection()])
    with pytest.raises(CrowdSimError, match="remove_selected needs the HIP engine"):
        sim.remove_selected(rect=(0.0, 0.0, 1.0, 1.0))
    with pytest.raises(CrowdSimError, match="remove_selected needs the HIP engine"):
        sim.remove_source_sink(0, with_agents=True)
    sim.remove_source_sink(0)  # (the default is the reference's call, which every library has)


def test_the_selection_value_type_builds_the_struct():
    hlp, lp = object(), object()
    handles = {id(hlp): 3, id(lp): 0}
    sel = Selection(rect=(1, 2.5, 3, 4), circle=(5, 6, 7), source_sink=2, high_level_planner=hlp, local_planner=lp,
                    waypoint=(1, 4), speed=(0.5, 2)).struct(lambda p: handles.get(id(p)))
    assert sel.terms == 127
    assert (sel.x0, sel.y0, sel.x1, sel.y1, sel.cx, sel.cy, sel.r) == (1.0, 2.5, 3.0, 4.0, 5.0, 6.0, 7.0)
    assert (sel.source_sink, sel.hlp, sel.lp, sel.wp_lo, sel.wp_hi, sel.speed_lo, sel.speed_hi) == (2, 3, 0, 1, 4, 0.5, 2.0)
    assert Selection().struct().terms == 0
    one = Selection(waypoint=2, high_level_planner=object(), local_planner=7).struct(lambda p: None)
    assert (one.terms, one.wp_lo, one.wp_hi, one.lp) == (_abi.CS_SEL_WAYPOINT | _abi.CS_SEL_HLP | _abi.CS_SEL_LP, 2, 2, 7)
    assert one.hlp not in (0, 1, 0xFFFFFFFF)  # (a planner the engine never saw: a handle nobody has)


def _records(rows):
    out = np.zeros(len(rows), dtype=AGENT_DTYPE)
    for k, (x, y, vx, vy, wp) in enumerate(rows):
        out[k] = (k, x, y, vx, vy, wp, 2.0)
    return out


def test_the_restatement_on_hand_cases():
    nan = float("nan")
    rec = _records([(1.0, 1.0, 0.0, 0.0, 0),     # 0: on the low corner of the rectangle
                    (3.0, 1.5, 3.0, 4.0, 1),     # 1: x == x1
                    (2.0, 4.0, 0.0, -2.0, 2),    # 2: y == y1
                    (3.0, 4.0, 1.0, 0.0, 0),     # 3: at distance exactly 5 from the origin
                    (nan, 1.5, 1.0, 1.0, 0),     # 4: a NaN coordinate
                    (2.0, 2.0, nan, 0.0, 7)])    # 5: a NaN velocity
    owner = np.array([NO_SINK, 0, 0, 1, NO_SINK, 2])
    hlp = np.array([0, 1, 1, 2, 0, 3])
    lp = np.array([0, 0, 1, 1, 0, 0])

    def picked(sel):
        return np.flatnonzero(pred(sel, rec, owner, hlp, lp)).tolist()
    assert picked(selection(0)) == [0, 1, 2, 3, 4, 5]  # no term: everybody, NaN or not
    rect = selection(_abi.CS_SEL_RECT, x0=1.0, y0=1.0, x1=3.0, y1=4.0)
    assert picked(rect) == [0, 5]  # x == x0 in, x == x1 out, y == y1 out, NaN out
    assert picked(selection(_abi.CS_SEL_CIRCLE, cx=0.0, cy=0.0, r=5.0)) == [0, 1, 2, 5]  # distance exactly r: out
    assert picked(selection(_abi.CS_SEL_CIRCLE, cx=0.0, cy=0.0, r=np.nextafter(5.0, 6.0))) == [0, 1, 2, 3, 5]
    assert picked(selection(_abi.CS_SEL_CIRCLE, cx=2.0, cy=2.0, r=0.0)) == []  # (0 < 0 is false at the centre too)
    assert picked(selection(_abi.CS_SEL_SOURCE_SINK, source_sink=NO_SINK)) == [0, 4]
    assert picked(selection(_abi.CS_SEL_SOURCE_SINK, source_sink=0)) == [1, 2]
    assert picked(selection(_abi.CS_SEL_SOURCE_SINK, source_sink=9)) == []
    assert picked(selection(_abi.CS_SEL_HLP, hlp=1)) == [1, 2]
    assert picked(selection(_abi.CS_SEL_LP, lp=1)) == [2, 3]
    assert picked(selection(_abi.CS_SEL_HLP | _abi.CS_SEL_LP, hlp=1, lp=1)) == [2]
    assert picked(selection(_abi.CS_SEL_WAYPOINT, wp_lo=1, wp_hi=2)) == [1, 2]
    assert picked(selection(_abi.CS_SEL_WAYPOINT, wp_lo=2, wp_hi=1)) == []  # an empty range
    assert picked(selection(_abi.CS_SEL_WAYPOINT, wp_lo=0, wp_hi=2 ** 64 - 1)) == [0, 1, 2, 3, 4, 5]
    # speeds: 0, 5, 2, 1, sqrt(2), NaN; the lower bound is inclusive, the upper one exclusive, both squared
    assert picked(selection(_abi.CS_SEL_SPEED, speed_lo=1.0, speed_hi=5.0)) == [2, 3, 4]
    assert picked(selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=float("inf"))) == [0, 1, 2, 3, 4]  # NaN out
    assert picked(selection(_abi.CS_SEL_SPEED, speed_lo=2.0, speed_hi=2.0)) == []
    assert picked(selection(_abi.CS_SEL_RECT, x0=2.0, y0=0.0, x1=2.0, y1=9.0)) == []  # x1 <= x0
    assert picked(selection(_abi.CS_SEL_RECT, x0=-np.inf, y0=-np.inf, x1=2.5, y1=np.inf)) == [0, 2, 5]  # a half plane
    both = selection(_abi.CS_SEL_RECT | _abi.CS_SEL_SPEED, x0=1.0, y0=1.0, x1=3.0, y1=4.0, speed_lo=0.0, speed_hi=1.0)
    assert picked(both) == [0]  # terms are ANDed; agent 5 fails the speed term through its NaN


def test_the_restatement_rounds_each_product_and_sum_once():
    """A point whose squared distance differs between a fused and an unfused evaluation: the restatement is the unfused
    one (dx*dx and dy*dy rounded, then their sum rounded)."""
    dx, dy = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -29
    unfused = np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy)
    rec = _records([(dx, dy, 0.0, 0.0, 0)])
    none = np.zeros(1)
    r_in, r_out = np.sqrt(np.nextafter(unfused, 9.0)), np.sqrt(unfused)
    for r in (r_in, r_out, np.nextafter(r_out, 0.0), np.nextafter(r_in, 9.0)):
        want = bool(unfused < np.float64(r) * np.float64(r))
        assert bool(pred(selection(_abi.CS_SEL_CIRCLE, cx=0.0, cy=0.0, r=float(r)), rec, none, none, none)[0]) == want
