"""The neighbours of each agent (include/crowdstep_state.h, cs_agent_neighbours) without a GPU: the header declares the
entry points and the binding table binds them with these signatures, the cross-compiled library exports them, the ctypes
NeighbourStat and the numpy dtype have the layout of the C struct, cs_selection is untouched, the C++ mirror compiles, a
library without the state header says so, and the restatement of the rules (tests/neighbours_reference.py), which the GPU
tests compare the engine with, holds on hand cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE, NEIGHBOUR_DTYPE
from neighbours_reference import neighbours

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cs_agent_neighbours", "cs_mesh_agent_neighbours")
GRID = dict(width=10.0, height=8.0, cell_size=2.0, offset=(1.0, -3.0))  # x in [1, 9): 4 rows; y in [-3, 7): 5 columns
INF = float("inf")
NONE = _abi.CS_NO_NEIGHBOUR


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_neighbour_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    want = (C.c_size_t, [C.c_void_p, C.c_double, C.POINTER(_abi.Selection), C.POINTER(_abi.Selection), C.c_uint64,
                         C.POINTER(_abi.NeighbourStat), C.c_size_t])
    for name in CALLS:
        assert name in declared and _abi.STATE_SYMBOLS[name] == want, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    for call in CALLS:  # the argument list of the header, type by type
        args = re.search(r"\bsize_t " + call + r"\((.*?)\);", text, flags=re.S).group(1)
        kinds = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
        assert [re.sub(r" [a-z_0-9]+$", "", k) for k in kinds] == [
            "cs_mesh*" if "mesh" in call else "cs_engine*", "double", "const cs_selection*", "const cs_selection*",
            "uint64_t", "cs_neighbour_stat*", "size_t"], kinds
    assert "Neighbours of each agent between steps" in _header()
    assert re.search(r"#define\s+CS_NO_NEIGHBOUR\s+UINT64_MAX", _header()) and NONE == 2 ** 64 - 1


def test_hip_library_exports_the_neighbour_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in CALLS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_row_and_the_dtype_have_the_layout_of_the_c_struct(tmp_path):
    names = [f for f, _ in _abi.NeighbourStat._fields_]
    assert names == ["id", "count", "nearest", "nearest_d2"] == list(NEIGHBOUR_DTYPE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cs_neighbour_stat));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_neighbour_stat, {f}));\n' for f in names)
                   + '  printf("%zu\\n", sizeof(cs_selection));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.NeighbourStat) == NEIGHBOUR_DTYPE.itemsize == 32
    assert got[1:5] == [getattr(_abi.NeighbourStat, f).offset for f in names] == [0, 8, 16, 24]
    assert [NEIGHBOUR_DTYPE.fields[f][1] for f in names] == got[1:5]
    assert [NEIGHBOUR_DTYPE.fields[f][0] for f in names] == [np.dtype("u8")] * 3 + [np.dtype("f8")]
    assert got[5] == ctypes.sizeof(_abi.Selection) == 104  # (untouched)


def test_cpp_mirror_with_the_neighbour_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_neighbours"))


def test_oracle_does_not_pretend_to_count_neighbours(oracle_lib):
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import CrowdSimError, LocationHash2D
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="agent_neighbours needs the HIP engine"):
        sim.agent_neighbours(1.0)
    with pytest.raises(CrowdSimError, match="agent_neighbours needs the HIP engine"):
        sim.count_agents_with_neighbours(0.5, dict(rect=(0.0, 0.0, 1.0, 1.0)), min_count=2)


def _records(rows, first_id=10):
    out = np.zeros(len(rows), dtype=AGENT_DTYPE)
    for k, (x, y) in enumerate(rows):
        out[k] = (first_id + k, x, y, 0.0, 0.0, 0, 2.0)
    return out


def _rows(table):
    return [(int(r["id"]), int(r["count"]), int(r["nearest"]), float(r["nearest_d2"])) for r in table]


def test_the_restatement_on_hand_cases():
    # three agents in a row at spacing 0.55: at 0.6 the ends see the middle, the middle sees both (the smaller id wins the
    # tie if the two squares are equal, else the smaller square); at 0.5 nobody sees anybody
    rec = _records([(2.0, 0.0), (2.55, 0.0), (3.1, 0.0)])
    d01 = (np.float64(2.0) - np.float64(2.55)) * (np.float64(2.0) - np.float64(2.55))
    d12 = (np.float64(2.55) - np.float64(3.1)) * (np.float64(2.55) - np.float64(3.1))
    mid = (10, float(d01)) if d01 <= d12 else (12, float(d12))
    assert _rows(neighbours(rec, GRID, 0.6)) == [(10, 1, 11, float(d01)), (11, 2, mid[0], mid[1]), (12, 1, 11, float(d12))]
    assert _rows(neighbours(rec, GRID, 0.5)) == [(10, 0, NONE, INF), (11, 0, NONE, INF), (12, 0, NONE, INF)]
    # ... a subject that is no other is still a subject; an other that is no subject has no row
    ends = np.array([True, False, True])
    assert _rows(neighbours(rec, GRID, 0.6, subjects=ends)) == [(10, 1, 11, float(d01)), (12, 1, 11, float(d12))]
    assert _rows(neighbours(rec, GRID, 0.6, others=ends)) == [(10, 0, NONE, INF), (11, 2, mid[0], mid[1]), (12, 0, NONE, INF)]
    # two agents on one point: neighbours for any distance > 0, d2 == +0.0; not at distance 0
    rec = _records([(2.0, 1.0), (2.0, 1.0)])
    got = neighbours(rec, GRID, 1e-9)
    assert _rows(got) == [(10, 1, 11, 0.0), (11, 1, 10, 0.0)] and not np.signbit(got["nearest_d2"]).any()
    assert _rows(neighbours(rec, GRID, 0.0)) == [(10, 0, NONE, INF), (11, 0, NONE, INF)]
    # a subject with four others at exactly d2 == 2.0: the smallest id wins, wherever it stands among the records
    rec = _records([(5.0, 1.0), (4.0, 0.0), (6.0, 0.0), (4.0, 2.0), (6.0, 2.0)])
    rec["id"] = [20, 17, 15, 16, 18]
    got = neighbours(rec, GRID, 1.5)
    assert _rows(got[got["id"] == 20]) == [(20, 4, 15, 2.0)]
    assert _rows(neighbours(rec, GRID, float(np.sqrt(2.0)), subjects=rec["id"] == 20)) in ([(20, 0, NONE, INF)], [(20, 4, 15, 2.0)])
    assert _rows(neighbours(rec, GRID, float(np.nextafter(np.sqrt(2.0), INF)), subjects=rec["id"] == 20))[0][1] in (0, 4)
    assert _rows(neighbours(rec, GRID, 1.5, subjects=rec["id"] == 20, others=rec["id"] != 15)) == [(20, 3, 16, 2.0)]
    # an outsider 0.1 m from an insider: neither counted nor reported (just below gx0; a NaN; beyond gy1)
    below = float(np.nextafter(1.0, 0.0))
    rec = _records([(1.0, 0.1), (below, 0.0), (float("nan"), 0.1), (1.05, 7.0), (1.05, 6.95)])
    assert _rows(neighbours(rec, GRID, 0.5)) == [(10, 0, NONE, INF), (14, 0, NONE, INF)]
    assert _rows(neighbours(rec, GRID, INF)) == [(10, 1, 14, float(np.float64(-0.05) * np.float64(-0.05)
                                                                   + np.float64(0.1 - 6.95) * np.float64(0.1 - 6.95))),
                                                 (14, 1, 10, float(np.float64(0.05) * np.float64(0.05)
                                                                   + np.float64(6.95 - 0.1) * np.float64(6.95 - 0.1)))]
    # distance 0 and +inf
    rec = _records([(2.0, 1.0), (2.0, 1.0), (8.5, 6.5), (9.0, 0.0), (float("nan"), 0.0)])
    assert [r[1] for r in _rows(neighbours(rec, GRID, 0.0))] == [0, 0, 0]
    far = neighbours(rec, GRID, INF)
    assert far["id"].tolist() == [10, 11, 12] and far["count"].tolist() == [2, 2, 2] and far["nearest"].tolist() == [11, 10, 10]
    # min_count: 0 reports every subject, larger values filter
    rec = _records([(2.0, 0.0), (2.5, 0.0), (3.0, 0.0), (5.0, 0.0), (5.5, 0.0), (8.0, 5.0)])
    for min_count, want in ((0, [10, 11, 12, 13, 14, 15]), (1, [10, 11, 12, 13, 14]), (2, [11]), (3, [])):
        assert neighbours(rec, GRID, 0.6, min_count=min_count)["id"].tolist() == want, min_count
    # the rows do not depend on the order of the records
    rec = _records([(2.0, 0.0), (2.5, 0.0), (3.0, 0.0), (3.5, 0.0), (6.0, 0.0)])
    rec["id"] = [14, 12, 10, 13, 11]
    base = neighbours(rec, GRID, 0.6)
    assert base["id"].tolist() == [10, 11, 12, 13, 14] and base["count"].tolist() == [2, 0, 2, 1, 1]
    assert base["nearest"].tolist() == [12, NONE, 10, 10, 12]
    for order in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
        assert neighbours(rec[order], GRID, 0.6).tobytes() == base.tobytes()
