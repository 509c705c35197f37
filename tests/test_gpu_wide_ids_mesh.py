"""CS_CFG_WIDE_IDS on a mesh: every tile renumbers together (cs_mesh), and the mesh equals one engine bit for bit, ids
included, through several renumberings: in-process 2 x 2 tiles, and two ranks over a host transport (gloo) on one GPU."""
import numpy as np
import pytest

from rmf_crowdsim_amd import (CS_CFG_WIDE_IDS, IdParityHighLevelPlan, LocationHash2D, MonotonicCrowd, NoLocalPlan,
                              Simulation, SourceSink, StubHighLevelPlan, Zanlungo, _abi, scenes)
from rmf_crowdsim_amd.tiles import NativeTileMesh

pytestmark = pytest.mark.gpu

FIRST, LIMIT, STEPS = 2 ** 33 + 6, 4096, 130
GRID = dict(width=64.0, height=64.0, cell_size=2.0, offset=(0.0, 0.0))


def _scene(sim):
    """~900 agents in contact (id-parity planner: parity must survive), 64 source-sinks whose agents reach their sink in
    the step they spawn (64 ids per step), and a removal by external id every 20 steps: ~9,000 ids through a 4,096-id
    device space.  Returns the ids read every 10 steps."""
    crowd = scenes.jittered_lattice(900, 0.6, (14.0, 14.0), 0.2, 21, columns=30)
    sim.add_agents(crowd, IdParityHighLevelPlan((0.0, 0.02)), Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    for k in range(64):  # a band across all four tiles
        x, y = 4.0 + 0.9 * k, 56.0 + (k % 3)
        sim.add_source_sink(SourceSink((x, y), 1.0, MonotonicCrowd(20.0), StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(),
                                       [(x, y)], False, 1.0))
    seen = []
    for s in range(STEPS):
        sim.step(0.05, report=False)
        if s % 20 == 19:
            sim.remove_agents(int(sim.read_agents()["id"].max()))
        if s % 10 == 9:
            seen.append(sim.read_agents()["id"].copy())
    return seen


def _single(monkeypatch):
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(FIRST))
    monkeypatch.setenv("CS_DEVICE_ID_LIMIT", str(LIMIT))
    single = Simulation(LocationHash2D(**GRID), flags=CS_CFG_WIDE_IDS)
    seen = _scene(single)
    tail = single.add_agents([(2.0, 2.0)], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.0)[0]
    return single, seen, tail


def test_an_in_process_mesh_renumbers_like_one_engine(monkeypatch):
    single, seen, tail = _single(monkeypatch)
    mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 2), 2, flags=CS_CFG_WIDE_IDS)
    mseen = _scene(mesh)
    assert mesh.add_agents([(2.0, 2.0)], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.0)[0] == tail
    assert tail - FIRST > 2 * LIMIT  # ids beyond two device id spaces: renumbered at least twice
    assert single.kernel_stat(_abi.CS_STAT_RENUMBERINGS) >= 2
    assert all(mesh.tile(k).kernel_stat(_abi.CS_STAT_RENUMBERINGS) >= 2 for k in range(4))
    assert len(mseen) == len(seen) and all((a == b).all() for a, b in zip(seen, mseen))
    a = single.read_agents()
    assert len(a) > 800 and a.tobytes() == mesh.read_agents().tobytes()
    probes = [(20.0, 20.0), (31.0, 33.0)]
    assert mesh.get_neighbours_in_radius_batch([3.0, 5.0], probes) == single.query_radius_batch([3.0, 5.0], probes)


def _rank(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import TorchHostTransport
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 1), 2, device=0, rank=rank, n_ranks=world,
                              flags=CS_CFG_WIDE_IDS, host_transport=TorchHostTransport(dist))
        seen = _scene(mesh)
        tail = mesh.add_agents([(2.0, 2.0)], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.0)[0]
        a = mesh.read_agents()
        n = mesh.tile(0).kernel_stat(_abi.CS_STAT_RENUMBERINGS)
        if rank == 0:
            with open(out_path, "wb") as f:
                pickle.dump((seen, tail, a, n), f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_renumber_like_one_engine(monkeypatch, tmp_path):
    import pickle
    import torch.multiprocessing as mp
    single, seen, tail = _single(monkeypatch)  # (the knobs are in the environment the ranks inherit)
    out = str(tmp_path / "wide_ids_mesh.pkl")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank, args=(r, 2, 29761, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    with open(out, "rb") as f:
        mseen, mtail, a, n = pickle.load(f)
    assert mtail == tail and n >= 2
    assert len(mseen) == len(seen) and all((x == y).all() for x, y in zip(seen, mseen))
    assert a.tobytes() == single.read_agents().tobytes()
