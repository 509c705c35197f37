"""Encounters (include/crowdstep_state.h, cs_encounters) without a GPU: the header declares the entry points and the
binding table binds them with these signatures, the cross-compiled library exports them, the ctypes Encounter and the
numpy dtype have the layout of the C struct, cs_selection is untouched, the C++ mirror compiles, a library without the
state header says so, and the restatement of the rule (tests/encounters_reference.py), which the GPU tests compare the
engine with, holds on hand cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE, ENCOUNTER_DTYPE
from encounters_reference import encounters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cs_encounters", "cs_mesh_encounters")
GRID = dict(width=20.0, height=16.0, cell_size=2.0, offset=(1.0, -3.0))  # x in [1, 17): 8 rows; y in [-3, 17): 10 columns
INF = float("inf")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_encounter_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    want = (C.c_size_t, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.POINTER(_abi.Selection),
                         C.POINTER(_abi.Selection), C.POINTER(_abi.Encounter), C.c_size_t])
    for name in CALLS:
        assert name in declared and _abi.STATE_SYMBOLS[name] == want, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    for call in CALLS:  # the argument list of the header, type by type
        args = re.search(r"\bsize_t " + call + r"\((.*?)\);", text, flags=re.S).group(1)
        kinds = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
        assert [re.sub(r" [a-z_0-9]+$", "", k) for k in kinds] == [
            "cs_mesh*" if "mesh" in call else "cs_engine*", "double", "double", "double", "const cs_selection*",
            "const cs_selection*", "cs_encounter*", "size_t"], kinds
        assert [k.split(" ")[-1] for k in kinds[1:4]] == ["distance", "horizon", "range"]
    assert "Encounters between steps" in _header()


def test_hip_library_exports_the_encounter_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in CALLS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_row_and_the_dtype_have_the_layout_of_the_c_struct(tmp_path):
    names = [f for f, _ in _abi.Encounter._fields_]
    assert names == ["a", "b", "t", "d2"] == list(ENCOUNTER_DTYPE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cs_encounter));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_encounter, {f}));\n' for f in names)
                   + '  printf("%zu\\n", sizeof(cs_selection));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.Encounter) == ENCOUNTER_DTYPE.itemsize == 32
    assert got[1:5] == [getattr(_abi.Encounter, f).offset for f in names] == [0, 8, 16, 24]
    assert [ENCOUNTER_DTYPE.fields[f][1] for f in names] == got[1:5]
    assert [ENCOUNTER_DTYPE.fields[f][0] for f in names] == [np.dtype("u8")] * 2 + [np.dtype("f8")] * 2
    assert got[5] == ctypes.sizeof(_abi.Selection) == 104  # (untouched)


def test_cpp_mirror_with_the_encounter_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_encounters"))


def test_oracle_does_not_pretend_to_forecast_encounters(oracle_lib):
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import CrowdSimError, LocationHash2D
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="encounters needs the HIP engine"):
        sim.encounters(0.5, 3.0, 4.0)
    with pytest.raises(CrowdSimError, match="encounters needs the HIP engine"):
        sim.count_encounters(0.5, 3.0, 4.0, dict(rect=(0.0, 0.0, 1.0, 1.0)))


def _records(rows, first_id=10):
    out = np.zeros(len(rows), dtype=AGENT_DTYPE)
    for k, (x, y, vx, vy) in enumerate(rows):
        out[k] = (first_id + k, x, y, vx, vy, 0, 2.0)
    return out


def _rows(table):
    return [(int(r["a"]), int(r["b"]), float(r["t"]), float(r["d2"])) for r in table]


def test_the_restatement_on_hand_cases():
    # head-on at 2 m, closing at 1 m/s: they meet after 2 s; with a horizon of 1 s they are 1 m apart at its end
    rec = _records([(10.0, 5.0, 0.5, 0.0), (12.0, 5.0, -0.5, 0.0)])
    assert _rows(encounters(rec, GRID, 0.5, 3.0, 4.0)) == [(10, 11, 2.0, 0.0)]
    assert _rows(encounters(rec, GRID, 0.5, 2.0, 4.0)) == [(10, 11, 2.0, 0.0)]  # (t == horizon: clamped to the same value)
    assert _rows(encounters(rec, GRID, 1.5, 1.0, 4.0)) == [(10, 11, 1.0, 1.0)]
    assert _rows(encounters(rec, GRID, 1.0, 1.0, 4.0)) == []                    # (the comparison is strict)
    assert _rows(encounters(rec, GRID, 0.5, 3.0, 2.0)) == []                    # (not in range: d2 == range^2)
    assert encounters(rec, GRID, 0.5, 3.0, 4.0, count_only=True) == 1
    # horizon 0: the pairs of close_pairs(min(distance, range)), m2 == d2
    assert _rows(encounters(rec, GRID, 2.5, 0.0, 4.0)) == [(10, 11, 0.0, 4.0)]
    assert _rows(encounters(rec, GRID, 4.0, 0.0, 2.0)) == [] and _rows(encounters(rec, GRID, 2.0, 0.0, 4.0)) == []
    # range 0, distance 0: none; distance +inf, horizon +inf, range +inf
    assert _rows(encounters(rec, GRID, 0.5, 3.0, 0.0)) == [] and _rows(encounters(rec, GRID, 0.0, 3.0, 4.0)) == []
    assert _rows(encounters(rec, GRID, INF, INF, INF)) == [(10, 11, 2.0, 0.0)]
    # equal velocities, and diverging: t == 0 and m2 == d2
    for va, vb in (((0.3, 0.1), (0.3, 0.1)), ((-0.5, 0.0), (0.5, 0.0)), ((0.0, 0.0), (0.0, 0.0)), ((0.0, 0.7), (0.0, -0.2))):
        rec = _records([(10.0, 5.0) + va, (12.0, 5.0) + vb])
        assert _rows(encounters(rec, GRID, 2.5, 3.0, 4.0)) == [(10, 11, 0.0, 4.0)], (va, vb)
        assert _rows(encounters(rec, GRID, 2.0, 3.0, 4.0)) == [], (va, vb)
    # two on one point with different velocities: rw == 0, so t == 0 and m2 == +0.0
    rec = _records([(6.0, 5.0, 0.4, 0.0), (6.0, 5.0, -0.3, 0.2)])
    got = encounters(rec, GRID, 1e-9, 3.0, 1e-9)
    assert _rows(got) == [(10, 11, 0.0, 0.0)] and not np.signbit(got["t"]).any() and not np.signbit(got["d2"]).any()
    # a perpendicular pass: q crosses 1 m in front of p at t = 2 (closest approach of the pair: 1 m at t = 2 exactly)
    rec = _records([(5.0, 5.0, 0.0, 0.0), (6.0, 3.0, 0.0, 1.0)])
    assert _rows(encounters(rec, GRID, 1.25, 3.0, 4.0)) == [(10, 11, 2.0, 1.0)]
    assert _rows(encounters(rec, GRID, 0.9, 3.0, 4.0)) == [] and _rows(encounters(rec, GRID, 1.0, 3.0, 4.0)) == []
    # velocities are f32 widened: 0.1 is not 0.1f
    rec = _records([(5.0, 5.0, 0.1, 0.0), (6.0, 5.0, 0.0, 0.0)])
    w = np.float64(0.0) - np.float64(np.float32(0.1))
    t = -(np.float64(1.0) * w) / (w * w)
    c = np.float64(1.0) + w * t
    assert _rows(encounters(rec, GRID, 0.5, 20.0, 4.0)) == [(10, 11, float(t), float(c * c))] and t != 10.0
    # an outsider just below gx0 heading for an insider: never reported, whatever the numbers
    below = float(np.nextafter(1.0, 0.0))
    rec = _records([(1.0, 0.1, 0.0, 0.0), (below, 0.0, 0.0, 0.1), (float("nan"), 0.1, 0.0, 0.0), (1.3, 0.1, -0.1, 0.0)])
    assert [r[:2] for r in _rows(encounters(rec, GRID, INF, INF, INF))] == [(10, 13)]
    assert [r[:2] for r in _rows(encounters(rec, GRID, 0.5, 1.0, 1.0))] == [(10, 13)]
    # roles: (A(p) && B(q)) || (A(q) && B(p))
    rec = _records([(10.0, 5.0, 0.5, 0.0), (12.0, 5.0, -0.5, 0.0), (11.0, 5.5, 0.0, 0.0)])
    first = np.array([True, False, False])
    assert [r[:2] for r in _rows(encounters(rec, GRID, 0.6, 3.0, 4.0))] == [(10, 11), (10, 12), (11, 12)]
    assert [r[:2] for r in _rows(encounters(rec, GRID, 0.6, 3.0, 4.0, first, None))] == [(10, 11), (10, 12)]
    assert [r[:2] for r in _rows(encounters(rec, GRID, 0.6, 3.0, 4.0, None, first))] == [(10, 11), (10, 12)]
    assert [r[:2] for r in _rows(encounters(rec, GRID, 0.6, 3.0, 4.0, first, first))] == []
    assert [r[:2] for r in _rows(encounters(rec, GRID, 0.6, 3.0, 4.0, first, ~first))] == [(10, 11), (10, 12)]
    # symmetry: reversing the record order (so who is p and who is q in the arithmetic of a test that walks slots) gives
    # the same bytes; and negating r and w by hand gives the same bits
    rng = np.random.default_rng(41)
    rec = _records([(float(x), float(y), float(vx), float(vy)) for x, y, vx, vy in
                    np.column_stack([rng.uniform(2.0, 16.0, 60), rng.uniform(-2.0, 16.0, 60), rng.normal(0.0, 0.8, 60),
                                     rng.normal(0.0, 0.8, 60)])])
    base = encounters(rec, GRID, 1.0, 2.0, 5.0)
    assert 10 < len(base) < 60 * 59 // 2 and (base["t"] == 0.0).any() and (base["t"] == 2.0).any()
    assert ((base["t"] > 0.0) & (base["t"] < 2.0)).any()
    assert encounters(rec[::-1], GRID, 1.0, 2.0, 5.0).tobytes() == base.tobytes()
    mirrored = rec.copy()
    mirrored["id"] = rec["id"].max() + rec["id"].min() - rec["id"]  # the larger id becomes the smaller: r and w negated
    flipped = encounters(mirrored, GRID, 1.0, 2.0, 5.0)
    key = lambda rows, a, b: sorted(zip(rows[a].tolist(), rows[b].tolist(), rows["t"].view(np.uint64).tolist(),  # noqa: E731
                                        rows["d2"].view(np.uint64).tolist()))
    back = flipped.copy()
    back["a"], back["b"] = rec["id"].max() + rec["id"].min() - flipped["b"], rec["id"].max() + rec["id"].min() - flipped["a"]
    assert key(back, "a", "b") == key(base, "a", "b")
