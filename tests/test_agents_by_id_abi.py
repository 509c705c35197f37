"""Reading and removing agents by id in batches (include/crowdstep_state.h) without a GPU: the HIP library exports the
four entry points with the signatures the separate binding table binds, the C++ mirror compiles, and a library without
the state header (the test oracle) says so instead of pretending."""
import ctypes
import os
import re

import pytest

from rmf_crowdsim_amd import _abi, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_ID = ("cs_read_agents_by_id", "cs_remove_agents", "cs_mesh_read_agents_by_id", "cs_mesh_remove_agents")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))


def test_the_state_header_declares_and_binds_the_batched_read_and_remove():
    declared = _declared("crowdstep_state.h")
    for name in BY_ID:
        assert name in declared and name in _abi.STATE_SYMBOLS, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    assert not set(_abi.STATE_SYMBOLS) & set(_abi.SYMBOLS)
    assert not set(_abi.STATE_SYMBOLS) & set(_declared("crowdstep.h"))
    C = ctypes
    ids, views, flags = C.POINTER(C.c_uint64), C.POINTER(_abi.AgentView), C.POINTER(C.c_uint8)
    for name in ("cs_read_agents_by_id", "cs_mesh_read_agents_by_id"):
        assert _abi.STATE_SYMBOLS[name] == (C.c_int, [C.c_void_p, ids, C.c_size_t, views, flags])
    for name in ("cs_remove_agents", "cs_mesh_remove_agents"):
        assert _abi.STATE_SYMBOLS[name] == (C.c_int, [C.c_void_p, ids, C.c_size_t])


def test_hip_library_exports_the_batched_read_and_remove():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in BY_ID:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_cpp_mirror_with_the_batched_read_and_remove_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_agents_by_id"))


def test_oracle_does_not_pretend_to_read_or_remove_by_id(oracle_lib):
    from oracle_sim import OracleSimulation
    from rmf_crowdsim_amd import CrowdSimError, LocationHash2D
    sim = OracleSimulation(LocationHash2D(10.0, 10.0, 1.0, (0.0, 0.0)))
    with pytest.raises(CrowdSimError, match="read_agents_by_id needs the HIP engine"):
        sim.read_agents_by_id([0])
    with pytest.raises(CrowdSimError, match="remove_agents_by_id needs the HIP engine"):
        sim.remove_agents_by_id([0])


def test_id_batches_are_uint64_in_the_order_given():
    import numpy as np
    from rmf_crowdsim_amd import CrowdSimError
    from rmf_crowdsim_amd.simulation import id_batch
    got = id_batch([7, 2 ** 40 + 3, 7, 0])
    assert got.dtype == np.uint64 and got.tolist() == [7, 2 ** 40 + 3, 7, 0] and got.flags["C_CONTIGUOUS"]
    assert id_batch([]).shape == (0,)
    assert id_batch(np.array([2 ** 63 + 5], dtype=np.uint64)).tolist() == [2 ** 63 + 5]
    for bad in ([1.5], [-1]):
        with pytest.raises(CrowdSimError):
            id_batch(bad)
