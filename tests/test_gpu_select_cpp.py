"""tests/cpp/test_select.cpp on the GPU: select_agents, count_agents, remove_selected and remove_source_sink(id, true)
through include/crowdsim.hpp, on one engine and on a 2 x 2 mesh."""
import subprocess

import pytest

from test_gpu_cpp_api import build_cpp_test

pytestmark = pytest.mark.gpu


def test_cpp_select_count_and_remove_selected():
    out = subprocess.run([build_cpp_test("test_select")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "select: passed" in out.stdout
