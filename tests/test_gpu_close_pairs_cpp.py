"""tests/cpp/test_close_pairs.cpp on the GPU: close_pairs / count_close_pairs through include/crowdsim.hpp, on one engine
and on a 2 x 2 mesh, against a brute-force double loop over `agents`."""
import subprocess

import pytest

from test_gpu_cpp_api import build_cpp_test

pytestmark = pytest.mark.gpu


def test_cpp_close_pairs_on_an_engine_and_a_mesh():
    out = subprocess.run([build_cpp_test("test_close_pairs")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "close pairs: passed" in out.stdout
