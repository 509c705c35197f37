"""The pairs of agents within a distance (include/crowdstep_state.h, cs_close_pairs) without a GPU: the header declares the
entry points and the binding table binds them with these signatures, the cross-compiled library exports them, the ctypes
IdPair has the layout of the C struct, CS_PAIRS_MAX matches, the C++ mirror compiles, a library without the state header
says so, and the numpy restatement of the rules (tests/close_pairs_reference.py), which the GPU tests compare the engine
with, holds on hand cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE
from close_pairs_reference import pairs, rectangle, roles, takes_part
from select_reference import selection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ("cs_close_pairs", "cs_mesh_close_pairs")
GRID = dict(width=10.0, height=8.0, cell_size=2.0, offset=(1.0, -3.0))  # x in [1, 9): 4 rows; y in [-3, 7): 5 columns


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_pair_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    want = (C.c_size_t, [C.c_void_p, C.c_double, C.POINTER(_abi.Selection), C.POINTER(_abi.Selection),
                         C.POINTER(_abi.IdPair), C.POINTER(C.c_double), C.c_size_t])
    for name in PAIRS:
        assert name in declared and _abi.STATE_SYMBOLS[name] == want, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    for call in PAIRS:  # the argument list of the header, type by type
        args = re.search(r"\bsize_t " + call + r"\((.*?)\);", text, flags=re.S).group(1)
        kinds = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
        assert [re.sub(r" [a-z_0-9]+$", "", k) for k in kinds] == [
            "cs_mesh*" if "mesh" in call else "cs_engine*", "double", "const cs_selection*", "const cs_selection*",
            "cs_id_pair*", "double*", "size_t"], kinds
    assert re.search(r"#define CS_PAIRS_MAX\s+\(1u << 26\)", _header()) and _abi.CS_PAIRS_MAX == 1 << 26 == 67108864


def test_hip_library_exports_the_pair_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in PAIRS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_id_pair_has_the_layout_of_the_c_struct(tmp_path):
    names = [f for f, _ in _abi.IdPair._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cs_id_pair));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_id_pair, {f}));\n' for f in names)
                   + '  printf("%zu\\n", sizeof(cs_selection));\n  printf("%u\\n", CS_PAIRS_MAX);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.IdPair) == 16
    assert names == ["a", "b"] and got[1:3] == [_abi.IdPair.a.offset, _abi.IdPair.b.offset] == [0, 8]
    assert got[3] == ctypes.sizeof(_abi.Selection) == 104  # (untouched)
    assert got[4] == _abi.CS_PAIRS_MAX
    # a uint64[n, 2] array is an array of cs_id_pair
    arr = np.array([[1, 2], [3, 2 ** 40]], dtype=np.uint64)
    as_pairs = ctypes.cast(arr.ctypes.data, ctypes.POINTER(_abi.IdPair))
    assert (as_pairs[0].a, as_pairs[0].b, as_pairs[1].a, as_pairs[1].b) == (1, 2, 3, 2 ** 40)


def test_cpp_mirror_with_the_pair_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_close_pairs"))


def test_oracle_does_not_pretend_to_list_pairs(oracle_lib):
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import CrowdSimError, LocationHash2D
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="close_pairs needs the HIP engine"):
        sim.close_pairs(1.0)
    with pytest.raises(CrowdSimError, match="close_pairs needs the HIP engine"):
        sim.count_close_pairs(0.5, dict(rect=(0.0, 0.0, 1.0, 1.0)))


def _records(rows, first_id=10):
    out = np.zeros(len(rows), dtype=AGENT_DTYPE)
    for k, (x, y) in enumerate(rows):
        out[k] = (first_id + k, x, y, 0.0, 0.0, 0, 2.0)
    return out


def test_the_rectangle_of_the_grid():
    assert rectangle(GRID) == (1.0, 9.0, -3.0, 7.0)  # x over height / cell rows, y over width / cell columns
    assert rectangle(dict(width=7.9, height=5.0, cell_size=2.0, offset=(0.0, 0.0))) == (0.0, 4.0, 0.0, 6.0)
    nan, inf = float("nan"), float("inf")
    rec = _records([(1.0, -3.0),                    # on gx0 and gy0: in
                    (9.0, 0.0),                     # on gx1: out
                    (np.nextafter(9.0, 0.0), np.nextafter(7.0, 0.0)),  # just inside both high edges: in
                    (np.nextafter(1.0, 0.0), 0.0),  # just below gx0: out
                    (2.0, 7.0),                     # on gy1: out
                    (nan, 0.0), (2.0, nan), (inf, 0.0), (2.0, -inf)])
    assert takes_part(rec, GRID).tolist() == [True, False, True, False, False, False, False, False, False]


def test_the_restatement_on_hand_cases():
    nan, inf = float("nan"), float("inf")
    # two agents on one point: a pair at any distance above 0 (d2 == 0), none at distance 0
    rec = _records([(2.0, 1.0), (2.0, 1.0)])
    for distance, n in ((0.0, 0), (5e-324, 0), (1e-160, 1), (0.5, 1), (inf, 1)):  # (5e-324 squared is 0: 0 < 0 is false)
        got, d2 = pairs(rec, GRID, distance)
        assert len(got) == n, distance
        if n:
            assert got.tolist() == [[10, 11]] and d2.tolist() == [0.0]
    # a pair at exactly `distance` is out, at the next f64 below it is in: 3-4-5, all products and sums exact
    rec = _records([(2.0, 1.0), (5.0, 5.0)])
    assert len(pairs(rec, GRID, 5.0)[0]) == 0
    assert len(pairs(rec, GRID, np.nextafter(5.0, 0.0))[0]) == 0
    got, d2 = pairs(rec, GRID, np.nextafter(5.0, inf))
    assert got.tolist() == [[10, 11]] and d2.tolist() == [25.0]
    near = _records([(2.0, 1.0), (np.nextafter(5.0, 0.0), 5.0)])  # the second agent a hair closer: in at distance 5
    got, d2 = pairs(near, GRID, 5.0)
    assert got.tolist() == [[10, 11]] and d2[0] < 25.0
    # who takes part: on gx0 in, on gx1 out, just below gx0 out, NaN and inf out; all within reach of agent 10
    rec = _records([(1.5, 0.0), (1.0, 0.0), (9.0, 0.0), (np.nextafter(1.0, 0.0), 0.0), (nan, 0.0), (inf, 0.0), (2.0, nan),
                    (2.0, -inf), (8.5, 0.0)])
    got, d2 = pairs(rec, GRID, inf)
    assert got.tolist() == [[10, 11], [10, 18], [11, 18]] and d2.tolist() == [0.25, 49.0, 56.25]
    assert pairs(rec, GRID, inf, count_only=True) == 3
    assert pairs(rec, GRID, 1.0)[0].tolist() == [[10, 11]]
    # the order is by (a, b) as ids, whatever the order of the records, and d2 follows
    shuffled = rec[[8, 1, 4, 0, 2, 3, 5, 6, 7]]
    again, d2_again = pairs(shuffled, GRID, inf)
    assert again.tolist() == got.tolist() and d2_again.tolist() == [0.25, 49.0, 56.25]
    # roles: a pair counts iff one is in A and the other in B; an agent may be both
    rec = _records([(2.0, 0.0), (2.5, 0.0), (3.0, 0.0), (3.5, 0.0)])  # ids 10..13 in a row, 0.5 apart
    a = np.array([True, False, False, False])
    everyone = np.ones(4, dtype=bool)
    assert pairs(rec, GRID, 1.1, a, None)[0].tolist() == [[10, 11], [10, 12]]
    assert pairs(rec, GRID, 1.1, None, a)[0].tolist() == [[10, 11], [10, 12]]  # (symmetric in the roles)
    assert pairs(rec, GRID, 1.1, a, a)[0].tolist() == []                        # A == B == one agent: no pair with itself
    ab = np.array([True, True, False, False])
    assert pairs(rec, GRID, 1.1, ab, ab)[0].tolist() == [[10, 11]]               # A == B: the pairs inside the group
    b = np.array([False, False, True, True])
    assert pairs(rec, GRID, 1.1, ab, b)[0].tolist() == [[10, 12], [11, 12], [11, 13]]   # disjoint: only across
    both = np.array([False, True, True, False])  # agent 11 is in A and in B
    assert pairs(rec, GRID, 1.1, ab, both)[0].tolist() == [[10, 11], [10, 12], [11, 12]]
    assert pairs(rec, GRID, 1.1, np.zeros(4, dtype=bool), everyone)[0].tolist() == []   # A selects nobody
    assert pairs(rec, GRID, 1.1, everyone, everyone)[0].tolist() == pairs(rec, GRID, 1.1)[0].tolist()
    # the roles come from select_reference.pred
    ra, rb = roles(selection(_abi.CS_SEL_RECT, x0=0.0, y0=-1.0, x1=2.25, y1=1.0), None, rec)
    assert ra.tolist() == [True, False, False, False] and rb.all()
