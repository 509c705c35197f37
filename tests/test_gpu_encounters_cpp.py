"""tests/cpp/test_encounters.cpp on the GPU: encounters / count_encounters through include/crowdsim.hpp, on one engine and on
a 2 x 2 mesh, against a brute-force double loop over `agents`; and the count and the bits it prints for one query against
what the Python side computes for the same scene (the restatement of tests/encounters_reference.py and the Python
surface)."""
import re
import subprocess

import numpy as np
import pytest

from rmf_crowdsim_amd import LocationHash2D, Simulation, StubHighLevelPlan, Zanlungo
from encounters_reference import encounters
from test_gpu_cpp_api import build_cpp_test

pytestmark = pytest.mark.gpu


def _python_side():
    """The scene of the C++ program, built and stepped from Python."""
    grid = dict(width=60.0, height=60.0, cell_size=2.0, offset=(0.0, 0.0))
    sim = Simulation(LocationHash2D(**grid))
    pts = {0: [], 1: []}
    for ix in range(20):
        for iy in range(20):
            pts[(ix + iy) % 2].append((18.0 + 1.1 * ix + 0.01 * iy, 17.0 + 1.2 * iy + 0.02 * ix))
    zan = Zanlungo(1.0, 1.0, 0.0, 0.4, 2.0, 0.2)
    sim.add_agents(np.array(pts[1]), StubHighLevelPlan((0.3, 0.2)), zan, 2.0)   # (the C++ program's pts_e, added first)
    sim.add_agents(np.array(pts[0]), StubHighLevelPlan((-0.6, 0.1)), zan, 2.0)
    for _ in range(20):
        sim.step(0.05)
    return sim, grid


def test_cpp_encounters_on_an_engine_and_a_mesh():
    out = subprocess.run([build_cpp_test("test_encounters")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "encounters: passed" in out.stdout
    m = re.search(r"encounters: check 0.8 2.0 2.0 count (\d+) ids ([0-9a-f]{16}) t ([0-9a-f]{16}) d2 ([0-9a-f]{16})", out.stdout)
    assert m, out.stdout
    sim, grid = _python_side()
    want = encounters(sim.read_agents(), grid, 0.8, 2.0, 2.0)
    got = sim.encounters(0.8, 2.0, 2.0)
    assert got.tobytes() == want.tobytes() and sim.count_encounters(0.8, 2.0, 2.0) == len(want) > 7
    xor = lambda v: int(np.bitwise_xor.reduce(v.view(np.uint64))) if len(v) else 0  # noqa: E731
    ids = int(np.bitwise_xor.reduce((want["a"] << np.uint64(20)) ^ want["b"]))
    assert (int(m.group(1)), int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16)) == \
        (len(want), ids, xor(np.ascontiguousarray(want["t"])), xor(np.ascontiguousarray(want["d2"])))
