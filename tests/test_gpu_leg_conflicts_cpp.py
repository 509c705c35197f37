"""tests/cpp/test_legs.cpp on the GPU: leg_conflicts / count_leg_conflicts through include/crowdsim.hpp, on one engine and
on a 2 x 2 mesh, against a brute-force loop over `agents`; and the conflicts and the bits it prints for one query against
what the Python side computes for the same scene (the restatement of tests/legs_reference.py and the Python surface)."""
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi
from legs_reference import NO_HIT, conflicts, legs_array
from test_gpu_cpp_api import build_cpp_test
from test_gpu_encounters_cpp import _python_side

pytestmark = pytest.mark.gpu


def _legs(rec):
    """The legs of the C++ program, formed by the same arithmetic."""
    order = rec[np.argsort(rec["id"])]
    start, v, t0, t1, ignore = [], [], [], [], []
    for c in range(6):
        frm = order[c * 67 + 3]
        x, y = float(frm["x"]), float(frm["y"])
        for k in range(15):
            vx = 0.0 if k % 3 == 2 else 0.25 * float((k + c) % 5 - 2)
            vy = 0.0 if k % 3 == 2 else 0.25 * float(k % 4 - 1)
            start.append((x, y))
            v.append((vx, vy))
            t0.append(float(k))
            t1.append(float(k) + 1.0)
            ignore.append(int(frm["id"]))
            x, y = x + vx, y + vy
    for k in range(60):
        start += [(-5.0, 16.0 + 0.45 * k), (17.0 + 0.4 * k, 66.0), (64.0, 50.0 - 0.5 * k), (30.0, 18.0 + 0.4 * k),
                  (18.0 + 0.4 * k, 30.0)]
        v += [(2.0, 0.0), (0.0, -4.0), (-1.0, -0.25 + 0.01 * k), (0.0, 0.0), (0.0, 0.0)]
        t0 += [0.0, 0.5, 1.0, 0.25 * k, 0.0]
        t1 += [35.0, 12.0, 1.0 + 0.5 * k, 0.25 * k + 4.0, 0.1 * k]
        ignore += [_abi.CS_NO_HIT] * 5
    return legs_array(start, v, t0, t1, np.array(ignore, dtype=np.uint64))


def test_cpp_leg_conflicts_on_an_engine_and_a_mesh():
    out = subprocess.run([build_cpp_test("test_legs")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "legs: passed" in out.stdout
    m = re.search(r"legs: check 0.5 2.0 legs (\d+) conflicts (\d+) ids ([0-9a-f]{16}) s ([0-9a-f]{16})", out.stdout)
    assert m, out.stdout
    sim, grid = _python_side()
    rec = sim.read_agents()
    legs = _legs(rec)
    want = conflicts(rec, grid, legs, 0.5, 2.0)
    got = sim.leg_conflicts(legs, 0.5, 2.0)
    hits = int((want["id"] != NO_HIT).sum())
    assert got.tobytes() == want.tobytes() and 50 < hits < len(legs) - 50
    xor = lambda v: int(np.bitwise_xor.reduce(v.view(np.uint64)))  # noqa: E731
    ids = xor(want["id"] * (2 * np.arange(len(want), dtype=np.uint64) + np.uint64(1)))
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3), 16), int(m.group(4), 16)) == \
        (len(legs), hits, ids, xor(np.ascontiguousarray(want["s"])))
