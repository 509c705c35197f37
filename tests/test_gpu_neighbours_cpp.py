"""tests/cpp/test_neighbours.cpp on the GPU: agent_neighbours / count_agents_with_neighbours through include/crowdsim.hpp, on
one engine and on a 2 x 2 mesh, against a brute-force double loop over `agents`."""
import subprocess

import pytest

from test_gpu_cpp_api import build_cpp_test

pytestmark = pytest.mark.gpu


def test_cpp_neighbours_on_an_engine_and_a_mesh():
    out = subprocess.run([build_cpp_test("test_neighbours")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "neighbours: passed" in out.stdout
