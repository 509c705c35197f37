"""tests/cpp/test_leg_intervals.cpp on the GPU: leg_intervals / count_leg_intervals through include/crowdsim.hpp, on one
engine and on a 2 x 2 mesh, against a brute-force loop over `agents` by the rule of the header."""
import re
import subprocess

import pytest

from test_gpu_cpp_api import build_cpp_test

pytestmark = pytest.mark.gpu


def test_cpp_leg_intervals_on_an_engine_and_a_mesh():
    out = subprocess.run([build_cpp_test("test_leg_intervals")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "leg intervals: passed" in out.stdout
    assert re.search(r"leg intervals: \d+ rows compared, \d+ stay until the leg ends, \d+ leave, \d+ inside at the start", out.stdout)
