"""tests/cpp/test_zone_agents.cpp on the GPU: zone_agents / count_zone_agents through include/crowdsim.hpp, on one engine
and on a 2 x 2 mesh, against a brute-force loop over `agents` by the rule of the header."""
import re
import subprocess

import pytest

from test_gpu_cpp_api import build_cpp_test

pytestmark = pytest.mark.gpu


def test_cpp_zone_agents_on_an_engine_and_a_mesh():
    out = subprocess.run([build_cpp_test("test_zone_agents")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "zone agents: passed" in out.stdout
    assert re.search(r"zone agents: \d+ rows compared, \d+ zones with five agents or more, \d+ empty", out.stdout)
