"""Writing agents between steps (include/crowdstep_state.h) without a GPU: the HIP library exports what the header
declares and the separate binding table binds it, the C++ mirror compiles, and the two conversions a write relies on
(to_global after a read, to_cell in the write) give the stored cell and offset back."""
import ctypes
import os
import re

import numpy as np

from rmf_crowdsim_amd import _abi, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))


def test_state_header_is_bound_apart_from_the_base_abi():
    assert sorted(_abi.STATE_SYMBOLS) == _declared("crowdstep_state.h")
    assert not set(_abi.STATE_SYMBOLS) & set(_abi.SYMBOLS)
    assert not set(_abi.STATE_SYMBOLS) & set(_declared("crowdstep.h"))
    assert (_abi.CS_WRITE_POSITION, _abi.CS_WRITE_VELOCITY, _abi.CS_WRITE_NEXT_WAYPOINT) == (1, 2, 4)


def test_hip_library_exports_the_state_header():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name, (restype, argtypes) in _abi.STATE_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_editing_the_state_header_rebuilds_the_library(monkeypatch):
    path = _native.build()
    header = os.path.join(ROOT, "include", "crowdstep_state.h")
    real = os.path.getmtime
    monkeypatch.setattr(os.path, "getmtime", lambda p: real(path) + 10 if os.path.abspath(p) == header else real(p))
    assert _native._stale()
    monkeypatch.setattr(os.path, "getmtime", real)
    assert not _native._stale()


def test_cpp_mirror_with_write_agents_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_agent_write"))


def test_oracle_does_not_pretend_to_write(oracle_lib):
    import pytest
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import CrowdSimError, LocationHash2D
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="write_agents needs the HIP engine"):
        sim.write_agents(np.zeros(1, dtype=[("id", "<u8"), ("x", "<f8")]))


def test_to_cell_of_to_global_gives_the_stored_state_back():
    """cs_read_agents reports offset_x + (cell * cell_size + (double)offset_f32) (cs_engine::to_global); a write places
    that point with to_cell: cell = floor((x - offset_x) / cell_size), offset = f32((x - offset_x) - cell * cell_size).
    The cell always comes back.  The offset comes back bit for bit unless it is so small that its f32 bits lie below
    the f64 ulp of the global coordinate (micrometres from a cell's low edge, hundreds of metres out): DESIGN.md
    section 2."""
    rng = np.random.default_rng(7)
    n = 200_000
    for cs in (0.3, 0.5, 0.7, 1.0, 1.3, 1.7, 2.0):
        for off in (0.0, -13.7, 97.25, 250.1, -500.0, 500.0):
            cell = rng.integers(0, 2000, n).astype(np.float64)
            ox = np.minimum((rng.random(n) * cs).astype(np.float32), np.nextafter(np.float32(cs), np.float32(0)))
            ox[: n // 20] = (rng.random(n // 20) * 1e-5).astype(np.float32)  # next to the low edge
            x = off + (cell * cs + ox.astype(np.float64))
            back_cell = np.floor((x - off) / cs)
            back = ((x - off) - back_cell * cs).astype(np.float32)
            assert (back_cell == cell).all(), (cs, off)
            lost = back != ox
            ulp = np.spacing(np.maximum(np.maximum(np.abs(x), abs(off)), cell * cs))  # (of the f64 terms involved)
            assert (ox[lost] < 2.0**26 * ulp[lost]).all(), (cs, off)
            assert (np.abs(back[lost].astype(np.float64) - ox[lost]) <= 2 * ulp[lost]).all(), (cs, off)
            assert not lost[n // 20:].mean() > 1e-4, (cs, off)  # (uniform offsets: rare)
