"""Every agent that enters a timed leg (include/crowdstep_state.h, cs_leg_intervals) without a GPU: the header declares the
entry points and the binding table binds them with these signatures, the cross-compiled library exports them, the ctypes
LegInterval and the numpy dtype have the layout of the C struct, cs_selection, cs_leg and cs_leg_hit are untouched, the C++
mirror compiles, the restatement of the rule (tests/leg_intervals_reference.py), which the GPU tests compare the engine
with, holds on hand cases typed in as closed forms, and merge_leg_intervals and the complement of free_intervals hold on
hand-typed rows."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE, LEG_INTERVAL_DTYPE, free_spans, merge_leg_intervals
from leg_intervals_reference import intervals, legs_array
from legs_reference import NO_HIT, conflicts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cs_leg_intervals", "cs_mesh_leg_intervals")
GRID = dict(width=40.0, height=40.0, cell_size=2.0, offset=(-20.0, -20.0))  # x and y in [-20, 20)
INF = float("inf")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_interval_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    want = (C.c_size_t, [C.c_void_p, C.POINTER(_abi.Leg), C.c_size_t, C.c_double, C.c_double, C.POINTER(_abi.Selection),
                         C.POINTER(C.c_uint64), C.POINTER(_abi.LegInterval), C.c_size_t])
    for name in CALLS:
        assert name in declared and _abi.STATE_SYMBOLS[name] == want, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    for call in CALLS:  # the argument list of the header, type by type
        args = re.search(r"\bsize_t " + call + r"\((.*?)\);", text, flags=re.S).group(1)
        kinds = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
        assert [re.sub(r" [a-z_0-9]+$", "", k) for k in kinds] == [
            "cs_mesh*" if "mesh" in call else "cs_engine*", "const cs_leg*", "size_t", "double", "double",
            "const cs_selection*", "uint64_t*", "cs_leg_interval*", "size_t"], kinds
        assert [k.split(" ")[-1] for k in kinds[1:]] == ["legs", "n", "distance", "speed_max", "targets", "out_counts", "out",
                                                         "cap"]
    assert "Every agent that enters a leg" in _header()
    assert re.search(r"#define\s+CS_ABI_VERSION\s+1\b", open(os.path.join(ROOT, "include", "crowdstep.h")).read())
    assert len(re.findall(r"#define\s+CS_NO_HIT\b", text)) == 1 and len(re.findall(r"#define\s+CS_PAIRS_MAX\b", text)) == 1


def test_hip_library_exports_the_interval_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in CALLS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_row_and_the_dtype_have_the_layout_of_the_c_struct(tmp_path):
    row = [f for f, _ in _abi.LegInterval._fields_]
    assert row == ["leg", "id", "s_in", "s_out"] == list(LEG_INTERVAL_DTYPE.names) == [f for f, _ in _abi.LEG_INTERVAL_DTYPE]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(cs_leg_interval));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_leg_interval, {f}));\n' for f in row)
                   + '  printf("%zu\\n%zu\\n%zu\\n", sizeof(cs_selection), sizeof(cs_leg), sizeof(cs_leg_hit));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.LegInterval) == LEG_INTERVAL_DTYPE.itemsize == 32
    assert got[1:5] == [getattr(_abi.LegInterval, f).offset for f in row] == [0, 8, 16, 24]
    assert [LEG_INTERVAL_DTYPE.fields[f][1] for f in row] == got[1:5]
    assert [LEG_INTERVAL_DTYPE.fields[f][0] for f in row] == [np.dtype("u8")] * 2 + [np.dtype("f8")] * 2
    assert got[5:] == [ctypes.sizeof(_abi.Selection), ctypes.sizeof(_abi.Leg), ctypes.sizeof(_abi.LegHit)] == [104, 56, 16]


def test_cpp_mirror_with_the_interval_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_leg_intervals"))


def _records(rows, first_id=10):
    out = np.zeros(len(rows), dtype=AGENT_DTYPE)
    for k, (x, y, vx, vy) in enumerate(rows):
        out[k] = (first_id + k, x, y, vx, vy, 0, 2.0)
    return out


def _all(rec, start, v, t0, t1, distance, speed_max=INF, ignore=None, targets=None):
    rows, counts = intervals(rec, GRID, legs_array([start], [v], t0, t1, ignore), distance, speed_max, targets)
    assert counts.tolist() == [len(rows)] and (rows["leg"] == 0).all()
    return [(int(r["id"]), float(r["s_in"]), float(r["s_out"])) for r in rows]


def test_the_restatement_on_hand_cases():
    # head-on: the gap of 10 m closes at 2 m/s and D = 1: inside from 4.5 s to 5.5 s
    rec = _records([(10.0, 0.0, -1.0, 0.0)])
    assert _all(rec, (0.0, 0.0), (1.0, 0.0), 0.0, 10.0, 1.0) == [(10, 4.5, 5.5)]
    # the same clipped by T = 5; s_in == T is no row
    assert _all(rec, (0.0, 0.0), (1.0, 0.0), 0.0, 5.0, 1.0) == [(10, 4.5, 5.0)]
    assert _all(rec, (0.0, 0.0), (1.0, 0.0), 0.0, 4.5, 1.0) == []
    # 2 s later the agent is at 8, the probe starts at 2: a gap of 6 m
    assert _all(rec, (2.0, 0.0), (1.0, 0.0), 2.0, 10.0, 1.0) == [(10, 2.5, 3.5)]
    # inside at the start and walking away: the probe waits 0.5 m behind an agent that leaves at 1 m/s, D = 1: out at 0.5 s
    away = _records([(0.5, 0.0, 1.0, 0.0)])
    assert _all(away, (0.0, 0.0), (0.0, 0.0), 0.0, 10.0, 1.0) == [(10, 0.0, 0.5)]
    got = intervals(away, GRID, legs_array([(0.0, 0.0)], [(0.0, 0.0)], 0.0, 10.0), 1.0, INF)[0]
    assert not np.signbit(got["s_in"][0])
    # inside at the start and passing through: from 0.5 m in front to 1 m behind at a closing speed of 2 m/s
    assert _all(rec, (9.5, 0.0), (1.0, 0.0), 0.0, 10.0, 1.0) == [(10, 0.0, 0.75)]
    # the same velocity: inside it never leaves, outside there is never a row
    assert _all(rec, (9.5, 0.0), (-1.0, 0.0), 0.0, 5.0, 1.0) == [(10, 0.0, 5.0)]
    assert _all(rec, (5.0, 0.0), (-1.0, 0.0), 0.0, 1e6, 1.0) == []
    # a graze is no row: the probe walks up x == 0, the agent stands 1 m to the side: |cr| == D |w|
    still = _records([(1.0, 5.0, 0.0, 0.0)])
    assert _all(still, (0.0, 0.0), (0.0, 1.0), 0.0, 20.0, 1.0) == []
    (who, s_in, s_out), = _all(still, (2.0 ** -52, 0.0), (0.0, 1.0), 0.0, 20.0, 1.0)  # (rx == 1 - 2^-52)
    assert who == 10 and s_in < 5.0 < s_out and s_out - s_in < 1e-6
    # a chord: the agent stands 0.6 m to the side, D = 1: the probe is inside for 2 * 0.8 m at 1 m/s
    chord = _records([(0.6, 5.0, 0.0, 0.0)])
    (who, s_in, s_out), = _all(chord, (0.0, 0.0), (0.0, 1.0), 0.0, 20.0, 1.0)
    assert who == 10 and abs(s_in - 4.2) < 1e-14 and abs(s_out - 5.8) < 1e-14
    # +inf distance: [0, T] for every slow participant, whichever way it walks, standing still included
    rec = _records([(10.0, 0.0, -2.0, 0.0), (10.0, 0.25, -1.0, 0.0), (-3.0, 4.0, 0.0, 0.0)])
    assert _all(rec, (0.0, 0.0), (0.0, 0.0), 1.0, 4.0, INF) == [(10, 0.0, 3.0), (11, 0.0, 3.0), (12, 0.0, 3.0)]
    assert _all(rec, (0.0, 0.0), (0.0, 0.0), 1.0, 4.0, INF, speed_max=2.0) == [(11, 0.0, 3.0), (12, 0.0, 3.0)]
    assert _all(rec, (0.0, 0.0), (0.0, 0.0), 1.0, 4.0, INF, speed_max=0.0) == []
    # several agents on one leg, ascending by id whatever their times; T == 0 and distance == 0 give nothing
    two = _all(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5)
    assert two[0] == (10, 4.75, 5.25) and two[1][0] == 11 and 9.5 < two[1][1] < 9.6 and 10.4 < two[1][2] < 10.5 and len(two) == 2
    assert two == _all(rec[::-1], (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5)
    assert _all(rec, (10.0, 0.0), (0.0, 0.0), 3.0, 3.0, 0.5) == [] and _all(rec, (10.0, 0.0), (0.0, 0.0), 0.0, 5.0, 0.0) == []
    # ignore and targets: the leg passes through that agent; everybody else is transparent
    assert [r[0] for r in _all(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5, ignore=10)] == [11]
    assert [r[0] for r in _all(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5, ignore=12345)] == [10, 11]
    assert [r[0] for r in _all(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5, targets=np.array([False, True, True]))] == [11]
    assert _all(rec, (0.0, 0.0), (0.0, 0.0), 0.0, 20.0, 0.5, targets=np.array([False, False, False])) == []
    # an outsider (beyond the grid's rectangle now, or at NaN) is never a row, wherever it would walk to
    out = _records([(20.0, 0.0, -1.0, 0.0), (float("nan"), 0.0, 0.0, 0.0), (19.0, 0.0, -1.0, 0.0)])
    assert _all(out, (0.0, 0.0), (0.0, 0.0), 0.0, 30.0, 0.5) == [(12, 18.5, 19.5)]
    # a random scene: the order of the records does not matter, every row is a sane interval, the first row of a leg by
    # (s_in, id) is the answer of the leg-conflict restatement, and what the interval says is true of the motion
    rng = np.random.default_rng(43)
    phi = rng.uniform(0.0, 2.0 * np.pi, 200)
    speed = np.where(np.arange(200) % 3 == 0, 1.3, 0.0)  # (two thirds stand)
    rec = _records([(float(x), float(y), float(s * np.cos(p)), float(s * np.sin(p)))
                    for x, y, p, s in zip(rng.uniform(-18.0, 18.0, 200), rng.uniform(-18.0, 18.0, 200), phi, speed)])
    psi = rng.uniform(0.0, 2.0 * np.pi, 300)
    t0 = rng.choice([0.0, 0.5, 2.0], 300)
    legs = legs_array(np.column_stack([rng.uniform(-22.0, 22.0, 300), rng.uniform(-22.0, 22.0, 300)]),
                      np.column_stack([np.cos(psi), np.sin(psi)]) * rng.choice([0.0, 0.5, 1.0, 2.0], 300)[:, None],
                      t0, t0 + rng.choice([0.5, 1.0, 3.0], 300), rng.choice(np.append(rec["id"][:5], _abi.CS_NO_HIT), 300))
    for distance in (0.8, 2.5):
        stats = {}
        rows, counts = intervals(rec, GRID, legs, distance, INF, stats=stats)
        print(f"  distance {distance}: {len(rows)} rows, {stats}")
        assert len(rows) >= 100 and stats["at_start"] and stats["later"] and stats["leaves"] and stats["stays"]
        again = intervals(rec[::-1], GRID, legs, distance, INF)
        assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == counts.tobytes()
        k = rows["leg"].astype(np.int64)
        T = (legs["t1"] - legs["t0"])[k]
        assert (0.0 <= rows["s_in"]).all() and (rows["s_in"] <= rows["s_out"]).all() and (rows["s_out"] <= T).all()
        assert (np.diff(k) >= 0).all() and (np.diff(rows["id"].astype(np.int64))[np.diff(k) == 0] > 0).all()
        first = conflicts(rec, GRID, legs, distance, INF)
        assert ((first["id"] != NO_HIT) == (counts > 0)).all()
        for j in np.nonzero(counts)[0]:
            mine = rows[k == j]
            best = mine[np.lexsort((mine["id"], mine["s_in"]))[0]]
            assert (best["id"], best["s_in"]) == (first["id"][j], first["s"][j])
        who = {int(r["id"]): r for r in rec}

        def apart(row, s):
            l, q = legs[int(row["leg"])], who[int(row["id"])]
            dx = (q["x"] + float(np.float32(q["vx"])) * (l["t0"] + s)) - (l["x0"] + l["vx"] * s)
            dy = (q["y"] + float(np.float32(q["vy"])) * (l["t0"] + s)) - (l["y0"] + l["vy"] * s)
            return float(np.hypot(dx, dy))
        early = rows[rows["s_out"] < T]
        assert len(early) >= 20
        for r in early:
            assert apart(r, 0.5 * (r["s_in"] + r["s_out"])) < distance < apart(r, r["s_out"] + 1e-6)


def _rows(spec):
    out = np.zeros(len(spec), dtype=LEG_INTERVAL_DTYPE)
    for k, r in enumerate(spec):
        out[k] = r
    return out


def test_merge_leg_intervals_and_the_free_spans():
    rows = _rows([(0, 7, 1.0, 2.0), (0, 8, 1.5, 3.0),                    # overlapping
                  (1, 7, 0.0, 1.0), (1, 9, 1.0, 2.5),                    # touching
                  (2, 5, 0.5, 4.0), (2, 6, 1.0, 2.0), (2, 9, 3.0, 3.5),  # nested
                  (4, 3, 2.0, 5.0), (4, 4, 0.0, 0.5), (4, 5, 0.25, 0.25)])  # apart, one reaching T = 5, one of no length
    want_offsets, want_spans = [0, 1, 2, 3, 3, 5], [(1.0, 3.0), (0.0, 2.5), (0.5, 4.0), (0.0, 0.5), (2.0, 5.0)]
    for order in (np.arange(len(rows)), np.arange(len(rows))[::-1], np.random.default_rng(1).permutation(len(rows))):
        offsets, spans = merge_leg_intervals(rows[order], 5)
        assert offsets.tolist() == want_offsets and spans.tolist() == [list(s) for s in want_spans]
        assert offsets.dtype == np.int64 and spans.dtype == np.float64 and spans.shape == (5, 2)
    offsets, spans = merge_leg_intervals(rows[:0], 3)
    assert offsets.tolist() == [0, 0, 0, 0] and spans.shape == (0, 2)
    with pytest.raises(ValueError):
        merge_leg_intervals(rows, 4)
    # spans that touch in the last bit only if they are equal: 0.1 + 0.2 is above 0.3
    close = _rows([(0, 1, 0.0, 0.3), (0, 2, 0.1 + 0.2, 1.0), (1, 1, 0.0, 0.1 + 0.2), (1, 2, 0.3, 1.0)])
    offsets, spans = merge_leg_intervals(close, 2)
    assert offsets.tolist() == [0, 2, 3] and spans.tolist() == [[0.0, 0.3], [0.1 + 0.2, 1.0], [0.0, 1.0]]
    # the complement, in absolute time: legs from t0 = 10 to 15 (leg 3 has no rows: free throughout)
    offsets, spans = merge_leg_intervals(rows, 5)
    free = free_spans(offsets, spans, np.full(5, 10.0), np.full(5, 15.0))
    assert free == [[(10.0, 11.0), (13.0, 15.0)], [(12.5, 15.0)], [(10.0, 10.5), (14.0, 15.0)], [(10.0, 15.0)],
                    [(10.5, 12.0)]]
    assert free_spans(*merge_leg_intervals(_rows([(0, 1, 0.0, 5.0)]), 1), [10.0], [15.0]) == [[]]
