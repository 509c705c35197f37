"""Who crosses a line (include/crowdstep_state.h, cs_gate_crossings) without a GPU: the header declares the entry points
and the binding table binds them with these signatures, the cross-compiled library exports them, the ctypes structs and
the numpy dtypes have the layout of the C structs, the C++ mirror compiles, gates_array and path_gates lay out what they
should, and the restatement of the rule (tests/gates_reference.py), which the GPU tests compare the engine with, holds on
hand cases typed in as closed forms."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE, GATE_CROSSING_DTYPE, GATE_DTYPE, gates_array, path_gates
from gates_reference import crossings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cs_gate_crossings", "cs_mesh_gate_crossings")
GRID = dict(width=40.0, height=40.0, cell_size=2.0, offset=(-20.0, -20.0))  # x and y in [-20, 20)
INF = float("inf")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_gate_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    want = (C.c_size_t, [C.c_void_p, C.POINTER(_abi.Gate), C.c_size_t, C.c_double, C.POINTER(_abi.Selection),
                         C.POINTER(C.c_uint64), C.POINTER(_abi.GateCrossing), C.c_size_t])
    for name in CALLS:
        assert name in declared and _abi.STATE_SYMBOLS[name] == want, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    for call in CALLS:  # the argument list of the header, type by type
        args = re.search(r"\bsize_t " + call + r"\((.*?)\);", text, flags=re.S).group(1)
        kinds = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
        assert [re.sub(r" [a-z_0-9]+$", "", k) for k in kinds] == [
            "cs_mesh*" if "mesh" in call else "cs_engine*", "const cs_gate*", "size_t", "double", "const cs_selection*",
            "uint64_t*", "cs_gate_crossing*", "size_t"], kinds
        assert [k.split(" ")[-1] for k in kinds[1:]] == ["gates", "n", "speed_max", "filter", "out_counts", "out", "cap"]
    assert "Who crosses a line" in _header()
    assert re.search(r"#define\s+CS_GATES_MAX\s+\(1u << 20\)", text) and _abi.CS_GATES_MAX == 1 << 20
    assert re.search(r"#define\s+CS_ABI_VERSION\s+1\b", open(os.path.join(ROOT, "include", "crowdstep.h")).read())
    assert len(re.findall(r"#define\s+CS_NO_HIT\b", text)) == 1 and len(re.findall(r"#define\s+CS_PAIRS_MAX\b", text)) == 1


def test_hip_library_exports_the_gate_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in CALLS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_structs_and_the_dtypes_have_the_layout_of_the_c_structs(tmp_path):
    gate = [f for f, _ in _abi.Gate._fields_]
    row = [f for f, _ in _abi.GateCrossing._fields_]
    assert gate == ["ax", "ay", "bx", "by", "t0", "t1"] == list(GATE_DTYPE.names) == [f for f, _ in _abi.GATE_DTYPE]
    assert row == ["gate", "dir", "id", "s", "u"] == list(GATE_CROSSING_DTYPE.names) == [f for f, _ in _abi.GATE_CROSSING_DTYPE]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n%zu\\n", sizeof(cs_gate), sizeof(cs_gate_crossing));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_gate, {f}));\n' for f in gate)
                   + "".join(f'  printf("%zu\\n", offsetof(cs_gate_crossing, {f}));\n' for f in row)
                   + '  printf("%zu\\n%zu\\n", sizeof(cs_selection), sizeof(cs_leg));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.Gate) == GATE_DTYPE.itemsize == 48
    assert got[1] == ctypes.sizeof(_abi.GateCrossing) == GATE_CROSSING_DTYPE.itemsize == 32
    assert got[2:8] == [getattr(_abi.Gate, f).offset for f in gate] == [0, 8, 16, 24, 32, 40]
    assert got[8:13] == [getattr(_abi.GateCrossing, f).offset for f in row] == [0, 4, 8, 16, 24]
    assert [GATE_DTYPE.fields[f][1] for f in gate] == got[2:8] and [GATE_CROSSING_DTYPE.fields[f][1] for f in row] == got[8:13]
    assert [GATE_DTYPE.fields[f][0] for f in gate] == [np.dtype("f8")] * 6
    assert [GATE_CROSSING_DTYPE.fields[f][0] for f in row] == [np.dtype("u4"), np.dtype("i4"), np.dtype("u8"),
                                                                np.dtype("f8"), np.dtype("f8")]
    assert got[13:] == [ctypes.sizeof(_abi.Selection), ctypes.sizeof(_abi.Leg)] == [104, 56]


def test_cpp_mirror_with_the_gate_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_gate_crossings"))


def test_gates_array_and_path_gates_lay_out_what_they_should():
    g = gates_array([(0.0, 1.0, 2.0, 3.0), (4.0, 5.0, 6.0, 7.0)], t1=1.5)
    assert g.dtype == GATE_DTYPE and g.tolist() == [(0.0, 1.0, 2.0, 3.0, 0.0, 1.5), (4.0, 5.0, 6.0, 7.0, 0.0, 1.5)]
    g = gates_array([[(0.0, 1.0), (2.0, 3.0)], [(4.0, 5.0), (6.0, 7.0)]], t0=[0.25, 0.5], t1=[1.0, 2.0])
    assert g.tolist() == [(0.0, 1.0, 2.0, 3.0, 0.25, 1.0), (4.0, 5.0, 6.0, 7.0, 0.5, 2.0)]
    assert len(gates_array(np.zeros((0, 4)), 0.0, 1.0)) == 0
    with pytest.raises(ValueError):
        gates_array([(0.0, 1.0, 2.0, 3.0)] * 2, t0=[0.0, 0.0, 0.0], t1=1.0)
    chain = path_gates([(0.0, 0.0), (1.0, 0.0), (1.0, 2.0), (-3.0, 2.0)], 0.5, 2.0)
    assert chain.tolist() == [(0.0, 0.0, 1.0, 0.0, 0.5, 2.0), (1.0, 0.0, 1.0, 2.0, 0.5, 2.0), (1.0, 2.0, -3.0, 2.0, 0.5, 2.0)]
    with pytest.raises(ValueError):
        path_gates([(0.0, 0.0)], 0.0, 1.0)


def _records(rows, first_id=10):
    out = np.zeros(len(rows), dtype=AGENT_DTYPE)
    for k, (x, y, vx, vy) in enumerate(rows):
        out[k] = (first_id + k, x, y, vx, vy, 0, 2.0)
    return out


def _all(rec, seg, t0, t1, speed_max=INF, mask=None):
    rows, counts = crossings(rec, GRID, gates_array([seg], t0, t1), speed_max, mask)
    assert (rows["gate"] == 0).all()
    assert counts.tolist() == [[int((rows["dir"] == 1).sum()), int((rows["dir"] == -1).sum())]]
    return [(int(r["id"]), int(r["dir"]), float(r["s"]), float(r["u"])) for r in rows]


GATE = (0.0, 0.0, 4.0, 0.0)  # along +x: left is y > 0


def test_the_restatement_on_hand_cases():
    # from 2 m below at 1 m/s: crosses after 2 s a quarter along, ending on the left; from above: on the right
    up, down = _records([(1.0, -2.0, 0.0, 1.0)]), _records([(3.0, 1.0, 0.0, -0.5)])
    assert _all(up, GATE, 0.0, 5.0) == [(10, 1, 2.0, 0.25)]
    assert _all(down, GATE, 0.0, 5.0) == [(10, -1, 2.0, 0.75)]
    # the other winding swaps the sides and measures u from the other end
    assert _all(up, (4.0, 0.0, 0.0, 0.0), 0.0, 5.0) == [(10, -1, 2.0, 0.75)]
    # s == T is no crossing; T == 0 gives nothing
    assert _all(up, GATE, 0.0, 2.0) == [] and _all(up, GATE, 0.0, 2.0 + 2.0 ** -50) == [(10, 1, 2.0, 0.25)]
    assert _all(up, GATE, 1.0, 1.0) == [] and _all(_records([(1.0, 0.0, 0.0, 1.0)]), GATE, 0.0, 0.0) == []
    # t0 > 0 moves the start: 1.5 s later the walker is 0.5 m below; after 2.5 s it has crossed and walks away
    assert _all(up, GATE, 1.5, 5.0) == [(10, 1, 0.5, 0.25)]
    assert _all(up, GATE, 2.5, 5.0) == []
    # on the line and moving off it, either way: s == +0.0 bitwise, never -0.0
    for vy, d in ((1.0, 1), (-1.0, -1)):
        rows, _ = crossings(_records([(1.0, 0.0, 0.0, vy)]), GRID, gates_array([GATE], 0.0, 5.0), INF)
        assert len(rows) == 1 and rows["dir"][0] == d and rows["s"].view(np.uint64)[0] == 0 and rows["u"][0] == 0.25
    # moving parallel to the gate, on it or beside it, and standing still: miss
    assert _all(_records([(1.0, 0.0, 1.0, 0.0), (1.0, -1.0, -1.0, 0.0), (1.0, -1.0, 0.0, 0.0)]), GATE, 0.0, 100.0) == []
    # moving away: miss
    assert _all(_records([(1.0, -2.0, 0.0, -1.0), (1.0, 2.0, 0.5, 1.0)]), GATE, 0.0, 100.0) == []
    # a gate with A == B: nobody, not even somebody who walks through the point
    assert _all(_records([(1.0, -2.0, 0.0, 1.0), (1.0, 0.0, 0.0, 1.0)]), (1.0, 0.0, 1.0, 0.0), 0.0, 100.0) == []
    # u == 0 is in and u == 1 is out; beyond either end: out
    ends = _records([(0.0, -1.0, 0.0, 1.0), (4.0, -1.0, 0.0, 1.0), (-0.125, -1.0, 0.0, 1.0), (4.125, -1.0, 0.0, 1.0)])
    assert _all(ends, GATE, 0.0, 5.0) == [(10, 1, 1.0, 0.0)]
    assert _all(ends, (4.0, 0.0, 8.0, 0.0), 0.0, 5.0) == [(11, 1, 1.0, 0.0), (13, 1, 1.0, 0.03125)]
    # an oblique walker: from (-1, -1) with velocity (1, 0.5) it is on the line after 2 s at x == 1
    assert _all(_records([(-1.0, -1.0, 1.0, 0.5)]), GATE, 0.0, 5.0) == [(10, 1, 2.0, 0.25)]
    # ss == S2 is excluded, a hair more includes; a NaN velocity is excluded; speed_max == 0 excludes everybody
    pace = _records([(1.0, -2.0, 0.0, 1.0), (2.0, -2.0, float("nan"), 1.0), (3.0, -2.0, 0.0, float("nan"))])
    assert _all(pace, GATE, 0.0, 5.0, speed_max=1.0) == [] and _all(pace, GATE, 0.0, 5.0, speed_max=0.0) == []
    assert _all(pace, GATE, 0.0, 5.0, speed_max=1.0 + 2.0 ** -52) == [(10, 1, 2.0, 0.25)]
    assert _all(pace, GATE, 0.0, 5.0) == [(10, 1, 2.0, 0.25)]
    # the filter; an outsider (beyond the grid's rectangle now, or at NaN) is never a row, wherever it would walk to
    three = _records([(1.0, -2.0, 0.0, 1.0), (2.0, 1.0, 0.0, -1.0), (3.0, -1.0, 0.0, 1.0)])
    assert [r[:2] for r in _all(three, GATE, 0.0, 5.0)] == [(10, 1), (11, -1), (12, 1)]
    assert [r[:2] for r in _all(three[::-1], GATE, 0.0, 5.0)] == [(10, 1), (11, -1), (12, 1)]
    assert [r[0] for r in _all(three, GATE, 0.0, 5.0, mask=np.array([False, True, True]))] == [11, 12]
    out = _records([(1.0, -20.5, 0.0, 1.0), (float("nan"), -1.0, 0.0, 1.0), (20.0, -1.0, -1.0, 1.0), (1.0, -19.0, 0.0, 1.0)])
    assert _all(out, (0.0, 0.0, 40.0, 0.0), 0.0, 50.0) == [(13, 1, 19.0, 0.025)]


def test_a_dyadic_chain_counts_a_walker_once():
    # agents on a 1/8 lattice, a five-gate chain on y == 0 against the single gate -4 .. 4, four velocities: the same
    # (id, dir, s) rows, the chain's u mapped back onto the whole gate, and no agent twice
    vertices = [-4.0, -2.5, -2.0, 0.25, 1.0, 4.0]
    chain = path_gates([(v, 0.0) for v in vertices], 0.0, 8.0)
    whole = gates_array([(-4.0, 0.0, 4.0, 0.0)], 0.0, 8.0)
    xs, ys = np.meshgrid(np.arange(-5.0, 5.0 + 0.125, 0.125), np.arange(-1.0, 1.0 + 0.125, 0.125))
    total = 0
    for vx, vy in ((0.0, 1.0), (0.0, -0.5), (0.25, 0.5), (-0.5, -0.25)):
        rec = _records([(float(x), float(y), vx, vy) for x, y in zip(xs.ravel(), ys.ravel())])
        a, ca = crossings(rec, GRID, chain, INF)
        b, cb = crossings(rec, GRID, whole, INF)
        assert len(np.unique(a["id"])) == len(a) == len(b) > 500
        order = np.argsort(a["id"], kind="stable")
        a = a[order]
        assert (a["id"] == b["id"]).all() and (a["dir"] == b["dir"]).all() and a["s"].tobytes() == b["s"].tobytes()
        lo = np.array(vertices)[a["gate"].astype(np.int64)]
        hi = np.array(vertices)[a["gate"].astype(np.int64) + 1]
        # (u is one division by a length that is no power of two: where along the line, to a few ulps of 8 m)
        assert (np.abs((lo + a["u"] * (hi - lo)) - (-4.0 + b["u"] * 8.0)) < 1e-13).all()
        assert ca.sum(axis=0).tolist() == cb.sum(axis=0).tolist()
        assert (ca.sum(axis=1) > 0).all()  # (every gate of the chain has somebody)
        total += len(a)
    print(f"  the dyadic chain: {total} rows, each once")
