"""tests/cpp/test_rays.cpp on the GPU: cast_rays / count_ray_hits through include/crowdsim.hpp, on one engine and on a 2 x 2
mesh, against a brute-force loop over `agents`; and the hits and the bits it prints for one query against what the Python
side computes for the same scene (the restatement of tests/rays_reference.py and the Python surface)."""
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import _abi
from rays_reference import NO_HIT, cast, rays_array
from test_gpu_cpp_api import build_cpp_test
from test_gpu_encounters_cpp import _python_side

pytestmark = pytest.mark.gpu


def _rays(rec):
    """The rays of the C++ program, formed by the same arithmetic."""
    order = rec[np.argsort(rec["id"])]
    o, u, t_max, ignore = [], [], [], []
    for c in range(6):
        frm = order[c * 67 + 3]
        for k in range(90):
            o.append((frm["x"], frm["y"]))
            u.append((float(k % 10) - 4.5, float(k // 10) - 4.0))
            t_max.append(0.25 + 0.05 * k)
            ignore.append(int(frm["id"]))
    for k in range(60):
        o += [(-5.0, 16.0 + 0.45 * k), (17.0 + 0.4 * k, 66.0), (64.0, 50.0 - 0.5 * k)]
        u += [(1.0, 0.0), (0.0, -2.0), (-1.0, -0.25 + 0.01 * k)]
        t_max += [np.inf, 40.0, 80.0]
        ignore += [_abi.CS_NO_HIT] * 3
    return rays_array(o, u, t_max, np.array(ignore, dtype=np.uint64))


def test_cpp_rays_on_an_engine_and_a_mesh():
    out = subprocess.run([build_cpp_test("test_rays")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "rays: passed" in out.stdout
    m = re.search(r"rays: check 0.2 rays (\d+) hits (\d+) ids ([0-9a-f]{16}) t ([0-9a-f]{16})", out.stdout)
    assert m, out.stdout
    sim, grid = _python_side()
    rec = sim.read_agents()
    rays = _rays(rec)
    want = cast(rec, grid, rays, 0.2)
    got = sim.cast_rays(np.column_stack([rays["ox"], rays["oy"]]), np.column_stack([rays["ux"], rays["uy"]]), 0.2,
                        t_max=rays["t_max"], ignore=rays["ignore"])
    hits = int((want["id"] != NO_HIT).sum())
    assert got.tobytes() == want.tobytes() and 100 < hits < len(rays) - 100
    xor = lambda v: int(np.bitwise_xor.reduce(v.view(np.uint64)))  # noqa: E731
    ids = xor(want["id"] * (2 * np.arange(len(want), dtype=np.uint64) + np.uint64(1)))
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3), 16), int(m.group(4), 16)) == \
        (len(rays), hits, ids, xor(np.ascontiguousarray(want["t"])))
