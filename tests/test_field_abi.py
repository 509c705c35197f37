"""Rasterising the crowd (include/crowdstep_state.h, cs_agent_field) without a GPU: the header declares the entry points
and the binding table binds them with these signatures, the cross-compiled library exports them, the ctypes FieldDesc has
the layout of the C struct, the C++ mirror compiles, a library without the state header says so, and the numpy
restatement of the rules (tests/field_reference.py), which the GPU tests compare the engine with, holds on hand cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE, field_desc
from field_reference import bins_of, desc, raster, tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD = ("cs_agent_field", "cs_mesh_agent_field")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_field_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    want = (C.c_int, [C.c_void_p, C.POINTER(_abi.FieldDesc), C.POINTER(_abi.Selection), C.POINTER(C.c_uint32),
                      C.POINTER(C.c_double), C.POINTER(C.c_double)])
    for name in FIELD:
        assert name in declared and _abi.STATE_SYMBOLS[name] == want, name
    assert _abi.STATE_SYMBOLS["cs_mesh_field_gather_bytes"] == (C.c_uint64, [C.c_void_p])
    assert sorted(_abi.STATE_SYMBOLS) == declared
    for call in FIELD:  # the argument list of the header, type by type
        args = re.search(r"\bint " + call + r"\((.*?)\);", text, flags=re.S).group(1)
        kinds = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
        assert [re.sub(r" [a-z_]+$", "", k) for k in kinds] == [
            "cs_mesh*" if "mesh" in call else "cs_engine*", "const cs_field_desc*", "const cs_selection*", "uint32_t*",
            "double*", "double*"], kinds
    assert int(re.search(r"#define CS_FIELD_MAX_CELLS\s+(\d+)u", _header()).group(1)) == _abi.CS_FIELD_MAX_CELLS == 4194304
    assert not re.findall(r"#define (CS_SEL_\w*FIELD\w*)", _header())  # (the CS_SEL_* set is the selections' own)


def test_hip_library_exports_the_field_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in FIELD + ("cs_mesh_field_gather_bytes",):
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_field_desc_has_the_layout_of_the_c_struct(tmp_path):
    names = [f for f, _ in _abi.FieldDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cs_field_desc));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_field_desc, {f}));\n' for f in names)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.FieldDesc) == 40
    assert got[1:] == [getattr(_abi.FieldDesc, f).offset for f in names]
    fields = re.search(r"typedef struct cs_field_desc \{(.*?)\} cs_field_desc;", _header(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", fields) == names  # (every field of the struct, in order)
    assert ctypes.sizeof(_abi.Selection) == 104  # (untouched)


def test_cpp_mirror_with_the_field_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_field"))


def test_oracle_does_not_pretend_to_rasterise(oracle_lib):
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import CrowdSimError, LocationHash2D
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="agent_field needs the HIP engine"):
        sim.agent_field((0.0, 0.0), 1.0, (10, 10))
    with pytest.raises(CrowdSimError, match="agent_field needs the HIP engine"):
        sim.agent_field((0.0, 0.0), (1.0, 2.0), (5, 10), velocity=True)


def test_the_python_arguments_build_the_struct():
    d = field_desc((1.5, -2.0), 0.25, (3, 7))
    assert (d.x0, d.y0, d.cell_w, d.cell_h, d.nx, d.ny) == (1.5, -2.0, 0.25, 0.25, 7, 3)  # shape is (ny, nx)
    d = field_desc(np.array([0.0, 4.0]), (2.0, 0.5), (1, 1))
    assert (d.cell_w, d.cell_h, d.nx, d.ny) == (2.0, 0.5, 1, 1)


def _records(rows):
    out = np.zeros(len(rows), dtype=AGENT_DTYPE)
    for k, (x, y, vx, vy) in enumerate(rows):
        out[k] = (k, x, y, vx, vy, 0, 2.0)
    return out


def test_the_restatement_on_hand_cases():
    nan, inf = float("nan"), float("inf")
    d = desc(1.0, 10.0, 0.5, 2.0, 4, 3)  # x in [1, 3), y in [10, 16)
    rec = _records([(1.0, 10.0, 1.0, 0.0),      # 0: exactly on x0 and y0: in, bin (0, 0)
                    (3.0, 11.0, 1.0, 0.0),      # 1: exactly on x0 + nx * cell_w: out
                    (2.0, 12.0, 0.5, -1.0),     # 2: on inner edges of both axes: the upper bins, (2, 1)
                    (nan, 11.0, 1.0, 1.0),      # 3: a NaN coordinate: out
                    (2.25, 12.5, nan, 3.0),     # 4: a NaN velocity: counted in (2, 1), its vx sum NaN
                    (2.4, 13.0, 0.25, 0.5),     # 5: (2, 1) as well
                    (0.999, 10.0, 1.0, 1.0),    # 6: just below x0: out
                    (1.2, 16.0, 1.0, 1.0),      # 7: exactly on y0 + ny * cell_h: out
                    (inf, 11.0, 1.0, 1.0),      # 8: +inf: out
                    (1.2, -inf, 1.0, 1.0),      # 9: -inf: out
                    (np.nextafter(3.0, 0.0), np.nextafter(16.0, 0.0), -0.75, 2.0)])  # 10: the last bin (3, 2)
    inside, flat = bins_of(d, rec["x"], rec["y"])
    assert inside.tolist() == [True, False, True, False, True, True, False, False, False, False, True]
    assert flat.tolist() == [0, -1, 6, -1, 6, 6, -1, -1, -1, -1, 11]
    count, sums, mags = raster(d, rec)
    assert count.shape == (3, 4) and count.dtype == np.uint32
    assert count.tolist() == [[1, 0, 0, 0], [0, 0, 3, 0], [0, 0, 0, 1]]
    assert sums[0, 0].tolist() == [1.0, 0.0] and sums[2, 3].tolist() == [-0.75, 2.0]
    assert np.isnan(sums[1, 2, 0]) and sums[1, 2, 1] == 2.5  # the NaN stays in its component
    assert (sums[count == 0] == 0.0).all() and not np.signbit(sums[count == 0]).any()
    tol = tolerance(count, mags)
    assert tol[0, 0].tolist() == [2.0 ** -52, 0.0] and tol[1, 2, 1] == 3 * 2.0 ** -52 * 4.5
    # the filter is select_reference.pred
    from select_reference import selection
    none = np.zeros(len(rec))
    fast = selection(_abi.CS_SEL_SPEED, speed_lo=1.0, speed_hi=100.0)  # |v| of 0, 2, 5, 10: 1, 1.118, 0.559, 2.136
    count, sums, _ = raster(d, rec, fast, none, none, none)
    assert count.tolist() == [[1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]  # (agent 4 fails the speed term through its NaN)
    assert sums[1, 2].tolist() == [0.5, -1.0]


def test_the_restatement_divides_and_does_not_multiply_by_a_reciprocal():
    """A coordinate where (x - x0) / cell_w and (x - x0) * (1 / cell_w) fall on different sides of a bin edge."""
    cell = 0.1
    found = None
    for k in range(1, 4000):
        x = np.float64(k) * np.float64(cell)  # a product that may round onto, above or below the edge k
        by_div = np.float64(x) / np.float64(cell)
        by_mul = np.float64(x) * (np.float64(1.0) / np.float64(cell))
        if int(by_div) != int(by_mul):
            found = (k, float(x), int(by_div), int(by_mul))
            break
    assert found is not None
    k, x, ix_div, ix_mul = found
    print(f"x = {x.hex()}: the division gives bin {ix_div}, the reciprocal bin {ix_mul}")
    d = desc(0.0, 0.0, cell, 1.0, 4096, 1)
    _, flat = bins_of(d, [x], [0.5])
    assert flat.tolist() == [ix_div] and ix_div != ix_mul
    count, _, _ = raster(d, _records([(x, 0.5, 0.0, 0.0)]))
    assert count[0, ix_div] == 1 and count[0, ix_mul] == 0
