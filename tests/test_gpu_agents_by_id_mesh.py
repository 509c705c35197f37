"""Reading and removing agents by id in batches on a tile mesh (cs_mesh_read_agents_by_id, cs_mesh_remove_agents;
NativeTileMesh.read_agents_by_id / remove_agents_by_id): every tile matches the batch against the agents it owns, the
outcome is agreed on before any slot dies, a refused batch removes nothing on any tile.  The mesh stays equal to one
engine, bit for bit, in process and over two ranks of a host transport."""
import numpy as np
import pytest

from rmf_crowdsim_amd import CrowdSimError, LocationHash2D, NoLocalPlan, Simulation, StubHighLevelPlan, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from test_gpu_agent_write_mesh import GRID, _scene

pytestmark = pytest.mark.gpu


def _keep_events(mesh):
    """Record events and leave them in the tiles' queues."""
    mesh._lib.cs_mesh_event_recording(mesh._mesh, 1)
    mesh._dispatch = lambda: None


def _events(mesh):
    """cs_mesh_drain_events: (kind, source_sink, id), tile by tile."""
    buf, out = (_abi.Event * 4096)(), []
    while True:
        n = mesh._lib.cs_mesh_drain_events(mesh._mesh, buf, len(buf))
        out += [(int(buf[i].kind), int(buf[i].source_sink), int(buf[i].id)) for i in range(n)]
        if n < len(buf):
            return out


def _batch(a, seed=41, per_tile=12):
    """Seeded ids from every quadrant of the 2 x 2 cut at 30 m, and the source-sink agents on their way (x < 17)."""
    rng = np.random.default_rng(seed)
    parts = []
    for in_x in (a["x"] < 30.0, a["x"] >= 30.0):
        for in_y in (a["y"] < 30.0, a["y"] >= 30.0):
            ids = a["id"][in_x & in_y & (a["x"] >= 17.0)]
            assert len(ids) >= per_tile
            parts.append(rng.choice(ids, per_tile, replace=False))
    parts.append(a["id"][a["x"] < 17.0])
    batch = np.concatenate(parts).astype(np.uint64)
    rng.shuffle(batch)
    return batch


def _rows(full, ids):
    at = np.searchsorted(full["id"], ids)
    assert (full["id"][at] == ids).all()
    return full[at]


def test_mesh_reads_and_removes_equal_one_engine_and_the_loop_of_single_removes():
    meshes = [NativeTileMesh(LocationHash2D(**GRID), (2, 2), 1) for _ in range(2)]
    single = Simulation(LocationHash2D(**GRID))
    for t in meshes + [single]:
        _scene(t)
    for m in meshes:
        _keep_events(m)
    for _ in range(25):
        for t in meshes + [single]:
            t.step(0.05)
    mesh, loop = meshes
    _events(mesh), _events(loop)  # (the spawns so far)
    a = single.read_agents()
    assert a.tobytes() == mesh.read_agents().tobytes()
    batch = _batch(a)
    assert (a["x"] < 17.0).sum() >= 2
    # read: the engine's rows, in the order asked, repeats included
    ask = np.concatenate([batch, batch[:5]])
    got = mesh.read_agents_by_id(ask)
    assert got.tobytes() == _rows(a, ask).tobytes() == single.read_agents_by_id(ask).tobytes()
    got, found = mesh.read_agents_by_id(np.concatenate([batch[:3], [10 ** 9]]).astype(np.uint64), missing_ok=True)
    assert found.tolist() == [True, True, True, False] and got[:3].tobytes() == _rows(a, batch[:3]).tobytes()
    assert int(got["id"][3]) == 10 ** 9 and got["x"][3] == 0.0
    # refused: one unknown id, or one id twice, removes nothing on any tile
    counts = mesh.tile_counts().copy()
    for bad, msg in ((np.concatenate([batch, [10 ** 9]]), "unknown agent id"), (np.concatenate([batch, batch[:1]]), "twice")):
        with pytest.raises(CrowdSimError, match=msg):
            mesh.remove_agents_by_id(bad.astype(np.uint64))
        assert mesh.read_agents().tobytes() == a.tobytes() and (mesh.tile_counts() == counts).all()
        assert _events(mesh) == []
    with pytest.raises(CrowdSimError, match="unknown agent id"):
        mesh.read_agents_by_id(np.concatenate([batch, [10 ** 9]]).astype(np.uint64))
    # removed: at once on the mesh and on the engine, one by one on the second mesh
    mesh.remove_agents_by_id(batch)
    single.remove_agents_by_id(batch)
    for i in batch:
        loop.remove_agents(int(i))
    assert (mesh.tile_counts() < counts).all()  # (every tile lost agents)
    assert (mesh.tile_counts() == loop.tile_counts()).all()
    assert mesh.read_agents().tobytes() == single.read_agents().tobytes() == loop.read_agents().tobytes()
    ev = _events(mesh)
    assert ev == _events(loop)
    assert sorted(e[2] for e in ev) == sorted(int(i) for i in batch) and {e[0] for e in ev} == {_abi.CS_EVENT_DESTROYED}
    sink_ids = set(int(i) for i in a["id"][a["x"] < 17.0])
    assert {e[1] for e in ev if e[2] in sink_ids} == {0} and {e[1] for e in ev if e[2] not in sink_ids} == {0xFFFFFFFF}
    for _ in range(20):
        for t in meshes + [single]:
            t.step(0.05)
    assert mesh.read_agents().tobytes() == single.read_agents().tobytes() == loop.read_agents().tobytes()
    assert _events(mesh) == _events(loop)


def test_agents_the_mesh_index_refused_are_read_and_removed_by_id():
    meshes = [NativeTileMesh(LocationHash2D(**GRID), (2, 2), 1) for _ in range(2)]
    for m in meshes:
        _scene(m)
        _keep_events(m)
        for _ in range(3):
            m.step(0.05)
        with pytest.raises(CrowdSimError):
            m.add_agents([(GRID["width"] * 5, 1.0)], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.5)
        _events(m)
    mesh, loop = meshes
    full = mesh.read_agents()
    assert full.tobytes() == loop.read_agents().tobytes()
    limbo = int(full["id"][full["x"] > GRID["width"]][0])
    ask = np.array([full["id"][4], limbo, full["id"][300]], dtype=np.uint64)
    assert mesh.read_agents_by_id(ask).tobytes() == _rows(full, ask).tobytes()
    mesh.remove_agents_by_id(ask)
    for i in ask:
        loop.remove_agents(int(i))
    assert len(mesh) == len(loop) == len(full) - 3
    assert mesh.read_agents().tobytes() == loop.read_agents().tobytes()
    assert _events(mesh) == _events(loop)
    for _ in range(5):
        for m in meshes:
            m.step(0.05)
    assert mesh.read_agents().tobytes() == loop.read_agents().tobytes()


def _rank_removes(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import TorchHostTransport
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 1), 1, device=0, rank=rank, n_ranks=world,
                              host_transport=TorchHostTransport(dist))
        _scene(mesh)
        for _ in range(25):
            mesh.step(0.05, report=False)
        a = mesh.read_agents()  # (the whole crowd on every rank)
        batch = _batch(a)
        notes = {"read": mesh.read_agents_by_id(batch).tobytes() == _rows(a, batch).tobytes()}
        ids = batch.ctypes.data_as(mesh._C.POINTER(mesh._C.c_uint64))
        bad = np.concatenate([batch, [10 ** 9]]).astype(np.uint64)
        notes["refused_rc"] = int(mesh._lib.cs_mesh_remove_agents(mesh._mesh, bad.ctypes.data_as(
            mesh._C.POINTER(mesh._C.c_uint64)), len(bad)))
        notes["refused_left"] = mesh.read_agents().tobytes() == a.tobytes()
        notes["removed_rc"] = int(mesh._lib.cs_mesh_remove_agents(mesh._mesh, ids, len(batch)))
        notes["local_lost"] = int(len(a) - len(mesh.read_agents()))
        for _ in range(20):
            mesh.step(0.05, report=False)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_a_batch_is_removed_across_two_ranks_over_a_host_transport(tmp_path):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU (the set-up of
    test_gpu_agent_write_mesh.py::test_a_mover_crosses_ranks_over_a_host_transport): the batch's ids live on both
    ranks; both return the same code, for the refused batch too; the whole crowd equals one engine's."""
    import pickle
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "removes.pkl")
    procs = [ctx.Process(target=_rank_removes, args=(r, 2, 29773, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    notes = []
    for r in range(2):
        with open(f"{out}.{r}", "rb") as f:
            notes.append(pickle.load(f))
    single = Simulation(LocationHash2D(**GRID))
    _scene(single)
    for _ in range(25):
        single.step(0.05, report=False)
    a = single.read_agents()
    batch = _batch(a)
    assert (a["x"][np.isin(a["id"], batch)] < 30.0).any() and (a["x"][np.isin(a["id"], batch)] >= 30.0).any()
    single.remove_agents_by_id(batch)
    for _ in range(20):
        single.step(0.05, report=False)
    want = single.read_agents()
    for n in notes:
        assert n["read"] and n["refused_rc"] == 2 and n["refused_left"] and n["removed_rc"] == 0
        assert n["local_lost"] == len(batch)
        assert len(want) > 500 and n["agents"].tobytes() == want.tobytes()
