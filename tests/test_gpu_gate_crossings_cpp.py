"""tests/cpp/test_gate_crossings.cpp on the GPU: gate_crossings / count_gate_crossings through include/crowdsim.hpp, on
one engine and on a 2 x 2 mesh, against a brute-force loop over `agents` by the rule of the header."""
import re
import subprocess

import pytest

from test_gpu_cpp_api import build_cpp_test

pytestmark = pytest.mark.gpu


def test_cpp_gate_crossings_on_an_engine_and_a_mesh():
    out = subprocess.run([build_cpp_test("test_gate_crossings")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "gate crossings: passed" in out.stdout
    assert re.search(r"gate crossings: \d+ rows compared, \d+ to the left, \d+ to the right, \d+ after t0", out.stdout)
