"""The clusters of agents under a distance (include/crowdstep_state.h, cs_agent_clusters) without a GPU: the header declares
the entry points and the binding table binds them with these signatures, the cross-compiled library exports them, the
ctypes Cluster has the layout of the C struct, cs_selection is untouched, the C++ mirror compiles, a library without the
state header says so, and the restatement of the rules (tests/clusters_reference.py), which the GPU tests compare the
engine with, holds on hand cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE, CLUSTER_DTYPE
from clusters_reference import clusters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cs_agent_clusters", "cs_mesh_agent_clusters")
GRID = dict(width=10.0, height=8.0, cell_size=2.0, offset=(1.0, -3.0))  # x in [1, 9): 4 rows; y in [-3, 7): 5 columns
INF = float("inf")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_cluster_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    want = (C.c_int, [C.c_void_p, C.c_double, C.POINTER(_abi.Selection), C.c_uint64, C.POINTER(C.c_uint64),
                      C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_abi.Cluster), C.c_size_t,
                      C.POINTER(C.c_size_t)])
    for name in CALLS:
        assert name in declared and _abi.STATE_SYMBOLS[name] == want, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    for call in CALLS:  # the argument list of the header, type by type
        args = re.search(r"\bint " + call + r"\((.*?)\);", text, flags=re.S).group(1)
        kinds = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
        assert [re.sub(r" [a-z_0-9]+$", "", k) for k in kinds] == [
            "cs_mesh*" if "mesh" in call else "cs_engine*", "double", "const cs_selection*", "uint64_t", "uint64_t*",
            "uint64_t*", "size_t", "size_t*", "cs_cluster*", "size_t", "size_t*"], kinds
    assert "Clusters of agents between steps" in _header()


def test_hip_library_exports_the_cluster_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in CALLS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_cluster_has_the_layout_of_the_c_struct(tmp_path):
    names = [f for f, _ in _abi.Cluster._fields_]
    assert names == ["label", "size", "min_x", "min_y", "max_x", "max_y", "sum_x", "sum_y"] == list(CLUSTER_DTYPE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cs_cluster));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_cluster, {f}));\n' for f in names)
                   + '  printf("%zu\\n", sizeof(cs_selection));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.Cluster) == CLUSTER_DTYPE.itemsize == 64
    assert got[1:9] == [getattr(_abi.Cluster, f).offset for f in names] == [8 * k for k in range(8)]
    assert [CLUSTER_DTYPE.fields[f][1] for f in names] == got[1:9]
    assert got[9] == ctypes.sizeof(_abi.Selection) == 104  # (untouched)


def test_cpp_mirror_with_the_cluster_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_clusters"))


def test_oracle_does_not_pretend_to_cluster(oracle_lib):
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import CrowdSimError, LocationHash2D
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="agent_clusters needs the HIP engine"):
        sim.agent_clusters(1.0)
    with pytest.raises(CrowdSimError, match="agent_clusters needs the HIP engine"):
        sim.count_clusters(0.5, dict(rect=(0.0, 0.0, 1.0, 1.0)), min_size=2)


def _records(rows, first_id=10):
    out = np.zeros(len(rows), dtype=AGENT_DTYPE)
    for k, (x, y) in enumerate(rows):
        out[k] = (first_id + k, x, y, 0.0, 0.0, 0, 2.0)
    return out


def _rows(table):
    return [(int(r["label"]), int(r["size"])) for r in table]


def test_the_restatement_on_hand_cases():
    # three agents in a row 0.5 apart at distance 0.6: one cluster, labelled with the smallest id
    rec = _records([(2.0, 0.0), (2.5, 0.0), (3.0, 0.0)])
    ids, labels, table, _ = clusters(rec, GRID, 0.6)
    assert ids.tolist() == [10, 11, 12] and labels.tolist() == [10, 10, 10] and _rows(table) == [(10, 3)]
    row = table[0]
    assert (row["min_x"], row["max_x"], row["min_y"], row["max_y"], row["sum_x"], row["sum_y"]) == (2.0, 3.0, 0.0, 0.0, 7.5, 0.0)
    # ... at exactly the spacing nobody is linked (strict)
    assert _rows(clusters(rec, GRID, 0.5)[2]) == [(10, 1), (11, 1), (12, 1)]
    # the middle one deselected: it bridges nobody, the other two are two singletons
    ids, labels, table, _ = clusters(rec, GRID, 0.6, np.array([True, False, True]))
    assert ids.tolist() == [10, 12] and labels.tolist() == [10, 12] and _rows(table) == [(10, 1), (12, 1)]
    assert (table[1]["min_x"], table[1]["max_x"], table[1]["sum_x"]) == (3.0, 3.0, 3.0)
    # the middle one just below gx0 (and the outer two within 0.6 of it, not of one another): the same
    below = float(np.nextafter(1.0, 0.0))
    rec = _records([(1.0, 0.55), (below, 0.0), (1.0, -0.55)])
    ids, labels, table, _ = clusters(rec, GRID, 0.6)
    assert ids.tolist() == [10, 12] and labels.tolist() == [10, 12] and _rows(table) == [(10, 1), (12, 1)]
    inside = _records([(1.0, 0.55), (1.0, 0.0), (1.0, -0.55)])  # (on gx0 it is a member and bridges)
    assert _rows(clusters(inside, GRID, 0.6)[2]) == [(10, 3)]
    # distance 0: every member its own cluster, even two on one point; +inf: all members one cluster, outsiders none
    rec = _records([(2.0, 1.0), (2.0, 1.0), (8.5, 6.5), (9.0, 0.0), (float("nan"), 0.0)])
    assert _rows(clusters(rec, GRID, 0.0)[2]) == [(10, 1), (11, 1), (12, 1)]
    ids, labels, table, _ = clusters(rec, GRID, INF)
    assert ids.tolist() == [10, 11, 12] and labels.tolist() == [10, 10, 10] and _rows(table) == [(10, 3)]
    assert _rows(clusters(rec, GRID, 1e-9)[2]) == [(10, 2), (12, 1)]
    # min_size: 0 and 1 report every cluster, larger values filter both outputs
    rec = _records([(2.0, 0.0), (2.5, 0.0), (3.0, 0.0), (5.0, 0.0), (5.5, 0.0), (8.0, 5.0)])
    for min_size, want in ((0, [(10, 3), (13, 2), (15, 1)]), (1, [(10, 3), (13, 2), (15, 1)]), (2, [(10, 3), (13, 2)]),
                           (3, [(10, 3)]), (4, [])):
        ids, labels, table, _ = clusters(rec, GRID, 0.6, None, min_size)
        assert _rows(table) == want, min_size
        assert len(ids) == sum(n for _, n in want) and sorted(set(labels.tolist())) == [l for l, _ in want]
    # labels do not depend on the order of the records; the smallest id may sit mid-chain
    rec = _records([(2.0, 0.0), (2.5, 0.0), (3.0, 0.0), (3.5, 0.0), (6.0, 0.0)])
    rec["id"] = [14, 12, 10, 13, 11]
    base = clusters(rec, GRID, 0.6)
    assert base[0].tolist() == [10, 11, 12, 13, 14] and base[1].tolist() == [10, 11, 10, 10, 10]
    assert _rows(base[2]) == [(10, 4), (11, 1)]
    for order in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
        again = clusters(rec[order], GRID, 0.6)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], base[:3]))
