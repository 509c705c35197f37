"""Paths against the moving crowd (include/crowdstep_state.h, cs_leg_conflicts) without a GPU: the header declares the entry
points and the binding table binds them with these signatures, the cross-compiled library exports them, the ctypes Leg /
LegHit and the numpy dtypes have the layout of the C structs, cs_selection is untouched, the C++ mirror compiles, and the
restatement of the rule (tests/legs_reference.py), which the GPU tests compare the engine with, holds on hand cases typed
in as closed forms."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE, LEG_DTYPE, LEG_HIT_DTYPE, paths_legs
from legs_reference import NO_HIT, conflicts, legs_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cs_leg_conflicts", "cs_mesh_leg_conflicts")
GRID = dict(width=40.0, height=40.0, cell_size=2.0, offset=(-20.0, -20.0))  # x and y in [-20, 20)
INF = float("inf")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_leg_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    want = (C.c_size_t, [C.c_void_p, C.POINTER(_abi.Leg), C.c_size_t, C.c_double, C.c_double, C.POINTER(_abi.Selection),
                         C.POINTER(_abi.LegHit)])
    for name in CALLS:
        assert name in declared and _abi.STATE_SYMBOLS[name] == want, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    for call in CALLS:  # the argument list of the header, type by type
        args = re.search(r"\bsize_t " + call + r"\((.*?)\);", text, flags=re.S).group(1)
        kinds = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
        assert [re.sub(r" [a-z_0-9]+$", "", k) for k in kinds] == [
            "cs_mesh*" if "mesh" in call else "cs_engine*", "const cs_leg*", "size_t", "double", "double",
            "const cs_selection*", "cs_leg_hit*"], kinds
        assert [k.split(" ")[-1] for k in kinds[1:]] == ["legs", "n", "distance", "speed_max", "targets", "out"]
    assert "Paths against the moving crowd between steps" in _header()
    assert _abi.CS_NO_HIT == 2 ** 64 - 1 and _abi.CS_LEGS_MAX == 1 << 20
    assert re.search(r"#define\s+CS_LEGS_MAX\s+\(1u << 20\)", text) and len(re.findall(r"#define\s+CS_NO_HIT\b", text)) == 1


def test_hip_library_exports_the_leg_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in CALLS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_rows_and_the_dtypes_have_the_layout_of_the_c_structs(tmp_path):
    leg = [f for f, _ in _abi.Leg._fields_]
    hit = [f for f, _ in _abi.LegHit._fields_]
    assert leg == ["x0", "y0", "vx", "vy", "t0", "t1", "ignore"] == list(LEG_DTYPE.names)
    assert hit == ["id", "s"] == list(LEG_HIT_DTYPE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cs_leg));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_leg, {f}));\n' for f in leg)
                   + '  printf("%zu\\n", sizeof(cs_leg_hit));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_leg_hit, {f}));\n' for f in hit)
                   + '  printf("%zu\\n", sizeof(cs_selection));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.Leg) == LEG_DTYPE.itemsize == 56
    assert got[1:8] == [getattr(_abi.Leg, f).offset for f in leg] == [0, 8, 16, 24, 32, 40, 48]
    assert [LEG_DTYPE.fields[f][1] for f in leg] == got[1:8]
    assert [LEG_DTYPE.fields[f][0] for f in leg] == [np.dtype("f8")] * 6 + [np.dtype("u8")]
    assert got[8] == ctypes.sizeof(_abi.LegHit) == LEG_HIT_DTYPE.itemsize == 16
    assert got[9:11] == [getattr(_abi.LegHit, f).offset for f in hit] == [0, 8]
    assert [LEG_HIT_DTYPE.fields[f][1] for f in hit] == got[9:11]
    assert [LEG_HIT_DTYPE.fields[f][0] for f in hit] == [np.dtype("u8"), np.dtype("f8")]
    assert got[11] == ctypes.sizeof(_abi.Selection) == 104  # (untouched)


def test_cpp_mirror_with_the_leg_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_legs"))


def _records(rows, first_id=10):
    out = np.zeros(len(rows), dtype=AGENT_DTYPE)
    for k, (x, y, vx, vy) in enumerate(rows):
        out[k] = (first_id + k, x, y, vx, vy, 0, 2.0)
    return out


def _one(rec, start, v, t0, t1, distance, speed_max=INF, ignore=None, targets=None):
    row = conflicts(rec, GRID, legs_array([start], [v], t0, t1, ignore), distance, speed_max, targets)[0]
    return int(row["id"]), float(row["s"])


MISS = (int(NO_HIT), INF)


def test_the_restatement_on_hand_cases():
    # head-on: the gap of 10 m closes at 2 m/s and D = 1: after 4.5 s
    rec = _records([(10.0, 0.0, -1.0, 0.0)])
    assert _one(rec, (0.0, 0.0), (1.0, 0.0), 0.0, 10.0, 1.0) == (10, 4.5)
    # the same 2 s later: the agent is at 8 by then, the probe starts at 2: a gap of 6 m, after 2.5 s
    assert _one(rec, (2.0, 0.0), (1.0, 0.0), 2.0, 10.0, 1.0) == (10, 2.5)
    # s == T is free, the next T is not
    assert _one(rec, (0.0, 0.0), (1.0, 0.0), 0.0, 4.5, 1.0) == MISS
    assert _one(rec, (0.0, 0.0), (1.0, 0.0), 0.0, float(np.nextafter(4.5, INF)), 1.0) == (10, 4.5)
    # a waiting probe that a walker reaches: 10 m at 1 m/s less D = 0.5
    assert _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5) == (10, 9.5)
    assert _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 9.0, 0.5) == MISS
    # equal velocities: inside D the conflict is at the start of the leg, outside D there is never one
    assert _one(rec, (9.5, 0.0), (-1.0, 0.0), 0.0, 5.0, 1.0) == (10, 0.0)
    assert _one(rec, (5.0, 0.0), (-1.0, 0.0), 0.0, 1e6, 1.0) == MISS
    got = conflicts(rec, GRID, legs_array([(9.5, 0.0)], [(-1.0, 0.0)], 0.0, 5.0), 1.0, INF)
    assert got["s"][0] == 0.0 and not np.signbit(got["s"][0])
    # a perpendicular crossing that grazes: the probe walks up x == 0, the agent stands 1 m to the side: |cr| == D |w|
    still = _records([(1.0, 5.0, 0.0, 0.0)])
    assert _one(still, (0.0, 0.0), (0.0, 1.0), 0.0, 20.0, 1.0) == MISS
    assert _one(still, (2.0 ** -52, 0.0), (0.0, 1.0), 0.0, 20.0, 1.0)[0] == 10  # (rx == 1 - 2^-52)
    # a crossing that does meet: the agent walks -x along y == 5 from x == 5, the probe +y from the origin, both at 1 m/s:
    # r = (5, 5), w = (-1, -1): a = -10, ww = 2, cr = 0, h2 = 2 D2: s = (10 - sqrt(2 D2)) / 2 with D2 = 2: 4
    cross = _records([(5.0, 5.0, -1.0, 0.0)])
    assert _one(cross, (0.0, 0.0), (0.0, 1.0), 0.0, 10.0, float(np.sqrt(2.0)))[0] == 10
    assert abs(_one(cross, (0.0, 0.0), (0.0, 1.0), 0.0, 10.0, float(np.sqrt(2.0)))[1] - 4.0) < 1e-14
    # an agent at or above speed_max is left out, so that a later one wins: 10 runs at 2 m/s, 11 walks at 1 m/s
    rec = _records([(10.0, 0.0, -2.0, 0.0), (10.0, 0.25, -1.0, 0.0)])
    assert _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5, speed_max=INF) == (10, 4.75)
    assert _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5, speed_max=2.5) == (10, 4.75)
    late = _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5, speed_max=2.0)  # (ss == 4 is not below 4)
    assert late[0] == 11 and 9.5 < late[1] < 9.6
    assert _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5, speed_max=1.0) == MISS
    assert _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5, speed_max=0.0) == MISS
    # two agents with the same s: the smaller id wins, whichever comes first in the records
    rec = _records([(10.0, 0.0, -1.0, 0.0), (-10.0, 0.0, 1.0, 0.0)])
    assert _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5) == _one(rec[::-1], (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5) == (10, 9.5)
    rec["id"] = [21, 20]
    assert _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5) == (20, 9.5)
    # T == 0 and distance == 0 give nothing, even on top of an agent
    assert _one(rec, (10.0, 0.0), (0.0, 0.0), 3.0, 3.0, 0.5) == MISS
    assert _one(rec, (10.0, 0.0), (0.0, 0.0), 0.0, 5.0, 0.0) == MISS and _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 50.0, 0.0) == MISS
    # ignore: the leg passes through that agent; an id nobody has ignores nobody
    assert _one(rec, (9.9, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5) == (21, 0.0)
    assert _one(rec, (9.9, 0.0), (0.0, 0.0), 0.0, 30.0, 0.5, ignore=21) == (20, 19.4)
    assert _one(rec, (9.9, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5, ignore=12345) == (21, 0.0)
    # targets: everybody else is transparent
    assert _one(rec, (9.9, 0.0), (0.0, 0.0), 0.0, 30.0, 0.5, targets=np.array([False, True])) == (20, 19.4)
    assert _one(rec, (9.9, 0.0), (0.0, 0.0), 0.0, 30.0, 0.5, targets=np.array([False, False])) == MISS
    # a far agent arrives first: 10 stands 3.6 m away and still, 11 is 12 m away and runs
    rec = _records([(2.0, 3.0, 0.0, 0.0), (12.0, 0.0, -3.0, 0.0)])
    stats = {}
    got = conflicts(rec, GRID, legs_array([(0.0, 0.0)], [(0.0, 0.0)], 0.0, 10.0), 0.5, INF, stats=stats)
    assert got["id"][0] == 11 and stats["not_nearest"] == 1
    # an outsider (beyond the grid's rectangle now, or at NaN) never conflicts, wherever it would walk to
    rec = _records([(20.0, 0.0, -1.0, 0.0), (float("nan"), 0.0, 0.0, 0.0), (19.0, 0.0, -1.0, 0.0)])
    assert _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 30.0, 0.5) == (12, 18.5)
    # the velocity is the f32 of the record, widened
    rec = _records([(10.0, 0.0, -0.1, 0.0)])
    v = float(np.float32(0.1))
    assert _one(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 200.0, 0.5)[1] == (10.0 * v - np.sqrt(0.25 * (v * v))) / (v * v)
    # reversing the record order gives the same bytes
    rng = np.random.default_rng(43)
    phi = rng.uniform(0.0, 2.0 * np.pi, 200)
    rec = _records([(float(x), float(y), float(1.3 * np.cos(p)), float(1.3 * np.sin(p)))
                    for x, y, p in zip(rng.uniform(-18.0, 18.0, 200), rng.uniform(-18.0, 18.0, 200), phi)])
    psi = rng.uniform(0.0, 2.0 * np.pi, 300)
    t0 = rng.choice([0.0, 0.5, 2.0], 300)
    legs = legs_array(np.column_stack([rng.uniform(-22.0, 22.0, 300), rng.uniform(-22.0, 22.0, 300)]),
                      np.column_stack([np.cos(psi), np.sin(psi)]) * rng.choice([0.0, 0.5, 1.0, 2.0], 300)[:, None],
                      t0, t0 + rng.choice([0.5, 1.0, 3.0], 300), rng.choice(np.append(rec["id"][:5], _abi.CS_NO_HIT), 300))
    stats = {}
    base = conflicts(rec, GRID, legs, 0.8, INF, stats=stats)
    hit = base["id"] != NO_HIT
    assert 40 < hit.sum() < 260 and (base["s"][hit] == 0.0).any() and (base["s"][hit] > 0.0).any()
    assert stats["not_nearest"] >= 3
    assert conflicts(rec[::-1], GRID, legs, 0.8, INF).tobytes() == base.tobytes()


def test_paths_become_legs():
    legs, owner = paths_legs([([(0.0, 0.0), (2.0, 0.0), (2.0, 0.0), (2.0, 3.0), (2.0, 3.0)], [0.0, 2.0, 3.5, 6.0, 6.0]),
                              ([(1.0, 1.0)], [0.0]), ([(1.0, 1.0), (1.0, 1.0)], [0.5, 5.0])])
    assert owner.tolist() == [0, 0, 0, 2] and legs.dtype == LEG_DTYPE
    assert legs[["x0", "y0", "vx", "vy", "t0", "t1"]].tolist() == [
        (0.0, 0.0, 1.0, 0.0, 0.0, 2.0), (2.0, 0.0, 0.0, 0.0, 2.0, 3.5), (2.0, 0.0, 0.0, 1.2, 3.5, 6.0),
        (1.0, 1.0, 0.0, 0.0, 0.5, 5.0)]
    assert (legs["ignore"] == _abi.CS_NO_HIT).all()
    assert legs_array([(0.0, 1.0)], [(1.0, 0.0)], 0.0, [1.0, 2.0, 3.0], 7)["ignore"].tolist() == [7, 7, 7]  # scalars broadcast
    for bad in (([(0.0, 0.0), (1.0, 0.0)], [1.0, 0.5]), ([(0.0, 0.0), (1.0, 0.0)], [-1.0, 0.5]),
                ([(0.0, 0.0), (1.0, 0.0)], [0.0, INF]), ([(0.0, 0.0)], [0.0, 1.0])):
        with pytest.raises(ValueError):
            paths_legs([bad])
