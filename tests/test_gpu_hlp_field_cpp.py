"""tests/cpp/test_hlp_field.cpp on the GPU: crowdsim::FieldPlanner through include/crowdsim.hpp, on a Simulation against
the same rule through the host callback path, and on a 2 x 2 TiledSimulation, with update()."""
import subprocess

import pytest

from test_gpu_cpp_api import build_cpp_test

pytestmark = pytest.mark.gpu


def test_cpp_field_planner_on_an_engine_and_a_mesh():
    out = subprocess.run([build_cpp_test("test_hlp_field")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "hlp field: passed" in out.stdout
