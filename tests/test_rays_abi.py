"""Rays against the crowd (include/crowdstep_state.h, cs_cast_rays) without a GPU: the header declares the entry points and
the binding table binds them with these signatures, the cross-compiled library exports them, the ctypes Ray / RayHit and
the numpy dtypes have the layout of the C structs, cs_selection is untouched, the C++ mirror compiles, and the restatement
of the rule (tests/rays_reference.py), which the GPU tests compare the engine with, holds on hand cases typed in as closed
forms."""
import ctypes
import os
import re
import subprocess

import numpy as np

from rmf_crowdsim_amd import _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE, RAY_DTYPE, RAY_HIT_DTYPE
from rays_reference import NO_HIT, cast, rays_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cs_cast_rays", "cs_mesh_cast_rays")
GRID = dict(width=20.0, height=16.0, cell_size=2.0, offset=(1.0, -3.0))  # x in [1, 17): 8 rows; y in [-3, 17): 10 columns
INF = float("inf")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_ray_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    want = (C.c_size_t, [C.c_void_p, C.POINTER(_abi.Ray), C.c_size_t, C.c_double, C.POINTER(_abi.Selection),
                         C.POINTER(_abi.RayHit)])
    for name in CALLS:
        assert name in declared and _abi.STATE_SYMBOLS[name] == want, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    for call in CALLS:  # the argument list of the header, type by type
        args = re.search(r"\bsize_t " + call + r"\((.*?)\);", text, flags=re.S).group(1)
        kinds = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
        assert [re.sub(r" [a-z_0-9]+$", "", k) for k in kinds] == [
            "cs_mesh*" if "mesh" in call else "cs_engine*", "const cs_ray*", "size_t", "double", "const cs_selection*",
            "cs_ray_hit*"], kinds
        assert [k.split(" ")[-1] for k in kinds[1:]] == ["rays", "n", "radius", "targets", "out"]
    assert "Rays against the crowd between steps" in _header()
    assert _abi.CS_NO_HIT == 2 ** 64 - 1 and _abi.CS_RAYS_MAX == 1 << 20
    assert re.search(r"#define\s+CS_NO_HIT\s+UINT64_MAX", text) and re.search(r"#define\s+CS_RAYS_MAX\s+\(1u << 20\)", text)


def test_hip_library_exports_the_ray_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in CALLS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_rows_and_the_dtypes_have_the_layout_of_the_c_structs(tmp_path):
    ray = [f for f, _ in _abi.Ray._fields_]
    hit = [f for f, _ in _abi.RayHit._fields_]
    assert ray == ["ox", "oy", "ux", "uy", "t_max", "ignore"] == list(RAY_DTYPE.names)
    assert hit == ["id", "t"] == list(RAY_HIT_DTYPE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cs_ray));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_ray, {f}));\n' for f in ray)
                   + '  printf("%zu\\n", sizeof(cs_ray_hit));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_ray_hit, {f}));\n' for f in hit)
                   + '  printf("%zu\\n", sizeof(cs_selection));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.Ray) == RAY_DTYPE.itemsize == 48
    assert got[1:7] == [getattr(_abi.Ray, f).offset for f in ray] == [0, 8, 16, 24, 32, 40]
    assert [RAY_DTYPE.fields[f][1] for f in ray] == got[1:7]
    assert [RAY_DTYPE.fields[f][0] for f in ray] == [np.dtype("f8")] * 5 + [np.dtype("u8")]
    assert got[7] == ctypes.sizeof(_abi.RayHit) == RAY_HIT_DTYPE.itemsize == 16
    assert got[8:10] == [getattr(_abi.RayHit, f).offset for f in hit] == [0, 8]
    assert [RAY_HIT_DTYPE.fields[f][1] for f in hit] == got[8:10]
    assert [RAY_HIT_DTYPE.fields[f][0] for f in hit] == [np.dtype("u8"), np.dtype("f8")]
    assert got[10] == ctypes.sizeof(_abi.Selection) == 104  # (untouched)


def test_cpp_mirror_with_the_ray_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_rays"))


def _records(rows, first_id=10):
    out = np.zeros(len(rows), dtype=AGENT_DTYPE)
    for k, (x, y) in enumerate(rows):
        out[k] = (first_id + k, x, y, 0.0, 0.0, 0, 2.0)
    return out


def _one(rec, o, u, radius, t_max=INF, ignore=None, targets=None):
    row = cast(rec, GRID, rays_array([o], [u], t_max, ignore), radius, targets)[0]
    return int(row["id"]), float(row["t"])


MISS = (int(NO_HIT), INF)


def test_the_restatement_on_hand_cases():
    # a disc dead ahead at 5 m with R = 0.5: entered at 4.5; a direction of length 2 halves t
    rec = _records([(10.0, 5.0)])
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 0.5) == (10, 4.5)
    assert _one(rec, (5.0, 5.0), (2.0, 0.0), 0.5) == (10, 2.25)
    assert _one(rec, (10.0, 1.0), (0.0, 0.5), 0.5) == (10, 7.0)  # along y, ux == 0
    # grazing at exactly |cr| == R * |u| is a miss; a hair inside is a hit
    assert _one(rec, (5.0, 5.5), (1.0, 0.0), 0.5) == MISS and _one(rec, (5.0, 4.5), (4.0, 0.0), 0.5) == MISS
    assert _one(rec, (5.0, float(np.nextafter(5.5, 0.0))), (1.0, 0.0), 0.5)[0] == 10
    # a disc behind the origin is a miss, and so is one abeam (b == 0)
    assert _one(rec, (12.0, 5.0), (1.0, 0.0), 0.5) == MISS and _one(rec, (10.0, 7.0), (1.0, 0.0), 0.5) == MISS
    # an origin inside a disc: t == +0.0, sign bit clear, whatever the direction
    for u in ((1.0, 0.0), (-1.0, 0.0), (0.0, -3.0)):
        got = cast(rec, GRID, rays_array([(10.25, 5.0)], [u]), 0.5)
        assert got["id"][0] == 10 and got["t"][0] == 0.0 and not np.signbit(got["t"][0])
    assert _one(rec, (10.5, 5.0), (1.0, 0.0), 0.5) == MISS  # on the circle, leaving: d2 == R2 is not inside, b < 0
    # t_max equal to t is a miss, its upper neighbour a hit; t_max == 0 and radius == 0 hit nothing
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 0.5, t_max=4.5) == MISS
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 0.5, t_max=float(np.nextafter(4.5, INF))) == (10, 4.5)
    assert _one(rec, (10.25, 5.0), (1.0, 0.0), 0.5, t_max=0.0) == MISS
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 0.0) == MISS and _one(rec, (10.0, 5.0), (1.0, 0.0), 0.0) == MISS
    # of two discs entered at the same t the smaller id wins, whichever comes first in the records
    rec = _records([(10.0, 6.0), (10.0, 4.0)])
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 1.25) == _one(rec[::-1], (5.0, 5.0), (1.0, 0.0), 1.25) == (10, 4.25)
    rec["id"] = [21, 20]
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 1.25) == (20, 4.25)
    # the first along the ray, not the nearest to the origin: 11 stands nearer (d2 8.6125 against 9) but off the axis
    # and is entered at about 2.68, 10 stands dead ahead and is entered at 2.5
    rec = _records([(8.0, 5.0), (7.9, 5.45)])
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 0.5) == (10, 2.5)
    assert 2.6 < _one(rec, (5.0, 5.0), (1.0, 0.0), 0.5, ignore=10)[1] < 2.7
    # ignore: the ray passes through that agent; an id nobody has ignores nobody
    rec = _records([(6.0, 5.0), (10.0, 5.0)])
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 0.5) == (10, 0.5)
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 0.5, ignore=10) == (11, 4.5)
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 0.5, ignore=12345) == (10, 0.5)
    assert _one(rec, (6.0, 5.0), (1.0, 0.0), 0.5, ignore=10) == (11, 3.5)  # the robot's own beam
    # targets: everybody else is transparent
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 0.5, targets=np.array([False, True])) == (11, 4.5)
    assert _one(rec, (5.0, 5.0), (1.0, 0.0), 0.5, targets=np.array([False, False])) == MISS
    # an outsider just below gx0, or at NaN, is never hit, whatever the numbers
    below = float(np.nextafter(1.0, 0.0))
    rec = _records([(below, 0.0), (float("nan"), 0.1), (1.0, 0.0)])
    assert _one(rec, (-4.0, 0.0), (1.0, 0.0), 0.5) == (12, 4.5)
    assert _one(rec, (below, 0.0), (0.0, 1.0), INF) == (12, 0.0)
    assert _one(rec[:2], (-4.0, 0.0), (1.0, 0.0), INF) == MISS
    # line of sight: o = A, u = B - A, t_max = 1, ignore = A; B is visible iff the hit is B
    rec = _records([(4.0, 4.0), (12.0, 10.0), (8.0, 7.2)])
    a, b = np.array([4.0, 4.0]), np.array([12.0, 10.0])
    assert _one(rec, a, b - a, 0.3, t_max=1.0, ignore=10)[0] == 12  # 12 stands in the way
    assert _one(rec[:2], a, b - a, 0.3, t_max=1.0, ignore=10)[0] == 11
    # reversing the record order gives the same bytes
    rng = np.random.default_rng(43)
    rec = _records([(float(x), float(y)) for x, y in zip(rng.uniform(2.0, 16.0, 80), rng.uniform(-2.0, 16.0, 80))])
    phi = rng.uniform(0.0, 2.0 * np.pi, 300)
    rays = rays_array(np.column_stack([rng.uniform(0.0, 18.0, 300), rng.uniform(-4.0, 18.0, 300)]),
                      np.column_stack([np.cos(phi), np.sin(phi)]) * rng.choice([1e-3, 1.0, 1e3], 300)[:, None],
                      rng.choice([0.5, 4.0, INF], 300), rng.choice(np.append(rec["id"][:5], _abi.CS_NO_HIT), 300))
    stats = {}
    base = cast(rec, GRID, rays, 0.4, stats=stats)
    hit = base["id"] != NO_HIT
    assert 40 < hit.sum() < 260 and (base["t"][hit] == 0.0).any() and (base["t"][hit] > 0.0).any()
    assert stats["not_nearest"] >= 3
    assert cast(rec[::-1], GRID, rays, 0.4).tobytes() == base.tobytes()
