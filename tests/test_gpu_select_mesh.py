"""Selecting, counting and removing agents on a tile mesh (cs_mesh_select_agents, cs_mesh_count_agents,
cs_mesh_remove_selected; NativeTileMesh.select_agents / count_agents / remove_selected): every tile selects among the
agents it owns and the mesh gives the single engine's answer, ids and order, rectangles that straddle the cuts included,
in process and over two ranks of a host transport.  After a mesh remove_selected the mesh stays equal to one engine, bit
for bit."""
import numpy as np
import pytest

from rmf_crowdsim_amd import CrowdSimError, LocationHash2D, NoLocalPlan, Selection, Simulation, StubHighLevelPlan, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from select_reference import NO_SINK, Ledger, count, drain, keep_events, select, selection
from test_gpu_agent_write_mesh import GRID, _scene

pytestmark = pytest.mark.gpu
INF = float("inf")


def _selections():
    """(name, selection): the cuts of a 2 x 2 mesh lie at 30 m, those of the 2 x 1 mesh of the two ranks at x = 30 m."""
    return [("everybody", selection(0)),
            ("a rectangle across both cuts", selection(_abi.CS_SEL_RECT, x0=24.0, y0=22.5, x1=37.25, y1=36.0)),
            ("a rectangle that ends on the cuts", selection(_abi.CS_SEL_RECT, x0=20.0, y0=20.0, x1=30.0, y1=30.0)),
            ("a rectangle that starts on the cuts", selection(_abi.CS_SEL_RECT, x0=30.0, y0=30.0, x1=INF, y1=INF)),
            ("a strip along the x cut", selection(_abi.CS_SEL_RECT, x0=29.0, y0=-INF, x1=31.0, y1=INF)),
            ("a circle on the corner of the four tiles", selection(_abi.CS_SEL_CIRCLE, cx=30.0, cy=30.0, r=6.0)),
            ("the sink's crowd", selection(_abi.CS_SEL_SOURCE_SINK, source_sink=0)),
            ("the sink's crowd past the cut", selection(_abi.CS_SEL_SOURCE_SINK | _abi.CS_SEL_RECT, source_sink=0, x0=9.0,
                                                        y0=0.0, x1=60.0, y1=60.0)),
            ("nobody's crowd", selection(_abi.CS_SEL_SOURCE_SINK, source_sink=NO_SINK)),
            ("planner 0 on local planner 0", selection(_abi.CS_SEL_HLP | _abi.CS_SEL_LP, hlp=0, lp=0)),
            ("on their first leg", selection(_abi.CS_SEL_WAYPOINT | _abi.CS_SEL_SPEED, wp_lo=0, wp_hi=0, speed_lo=0.5,
                                             speed_hi=3.0)),
            ("nobody", selection(_abi.CS_SEL_RECT, x0=30.0, y0=0.0, x1=30.0, y1=60.0))]


def _answers(t):
    """What a mesh or an engine answers to every selection, by the C entry points: ids, counts of one counting call, and
    the first ids under a cap."""
    sels = _selections()
    out = {}
    for name, sel in sels:
        n, ids = select(t, sel)
        assert n == len(ids), name
        n_cap, few = select(t, sel, cap=3)
        assert n_cap == n and few.tolist() == ids[:3].tolist(), name
        out[name] = ids.tolist()
    rc, counts = count(t, [s for _, s in sels])
    assert rc == 0
    out["counts"] = counts.tolist()
    return out


def test_a_mesh_selects_counts_and_removes_as_one_engine():
    mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 2), 1)
    single = Simulation(LocationHash2D(**GRID))
    led = Ledger(single).watch()
    for t in (mesh, single):
        _scene(t)
        keep_events(t)
    for _ in range(25):
        for t in (mesh, single):
            t.step(0.05)
    led.hear(drain(single))
    drain(mesh)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    assert (mesh.tile_counts() > 0).all()
    on_mesh, on_engine = _answers(mesh), _answers(single)
    for name, sel in _selections():
        want = led.expected(sel, rec).tolist()
        print(f"{name}: {len(want)}")
        assert on_engine[name] == want and on_mesh[name] == want, name
    assert on_mesh["counts"] == on_engine["counts"] == [len(on_engine[name]) for name, _ in _selections()]
    assert len(on_engine["the sink's crowd"]) >= 2 and len(on_engine["a rectangle across both cuts"]) > 50
    assert on_engine["nobody"] == [] and len(on_engine["a strip along the x cut"]) > 10
    # the Python surface of the mesh
    ids = mesh.select_agents(rect=(24.0, 22.5, 37.25, 36.0))
    assert ids.dtype == np.uint64 and ids.tolist() == on_engine["a rectangle across both cuts"]
    assert mesh.select_agents(Selection(source_sink=0), limit=1).tolist() == on_engine["the sink's crowd"][:1]
    assert mesh.count_agents([Selection(), dict(circle=(30.0, 30.0, 6.0))]).tolist() == [
        len(rec), len(on_engine["a circle on the corner of the four tiles"])]
    with pytest.raises(CrowdSimError, match="select_agents"):
        mesh.select_agents(circle=(30.0, 30.0, -1.0))
    assert mesh.read_agents().tobytes() == rec.tobytes()
    # remove_selected: the rectangle across the cuts and the sink's crowd, on the mesh and on the engine
    counts = mesh.tile_counts().copy()
    for terms in (dict(rect=(24.0, 22.5, 37.25, 36.0)), dict(source_sink=0)):
        gone = mesh.remove_selected(**terms)
        assert gone.tolist() == single.remove_selected(**terms).tolist() and len(gone) >= 2
        ev = drain(mesh)
        assert sorted(e[2] for e in ev) == gone.tolist() and {e[0] for e in ev} == {_abi.CS_EVENT_DESTROYED}
        assert [e[2] for e in drain(single)] == gone.tolist()
        assert len(mesh.select_agents(**terms)) == 0
    assert (mesh.tile_counts() < counts).all()  # (every tile lost agents)
    assert mesh.read_agents().tobytes() == single.read_agents().tobytes()
    for _ in range(10):
        for t in (mesh, single):
            t.step(0.05)
    assert mesh.read_agents().tobytes() == single.read_agents().tobytes()
    # with_agents: the sink goes with the crowd it spawned since
    assert len(mesh.select_agents(source_sink=0)) >= 1
    mesh.remove_source_sink(0, with_agents=True)
    single.remove_source_sink(0, with_agents=True)
    for _ in range(10):
        for t in (mesh, single):
            t.step(0.05)
    assert len(mesh.select_agents(source_sink=0)) == 0
    assert mesh.read_agents().tobytes() == single.read_agents().tobytes()


def test_a_mesh_selects_the_agent_its_index_refused():
    mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 2), 1)
    _scene(mesh)
    for _ in range(3):
        mesh.step(0.05)
    still = StubHighLevelPlan((0.0, 0.0))
    with pytest.raises(CrowdSimError):
        mesh.add_agents([(GRID["width"] * 5, 1.0)], still, NoLocalPlan(), 1.5)
    hlp = mesh._handles[id(still)]
    full = mesh.read_agents()
    limbo = int(full["id"][full["x"] > GRID["width"]][0])
    n, ids = select(mesh, selection(0))
    assert n == len(full) and ids.tolist() == full["id"].tolist()
    n, ids = select(mesh, selection(_abi.CS_SEL_RECT, x0=GRID["width"], y0=0.0, x1=INF, y1=2.0))
    assert ids.tolist() == [limbo]
    n, ids = select(mesh, selection(_abi.CS_SEL_RECT, x0=0.0, y0=0.0, x1=GRID["width"], y1=GRID["height"]))
    assert n == len(full) - 1 and limbo not in ids
    rc, counts = count(mesh, [selection(0), selection(_abi.CS_SEL_HLP, hlp=hlp),
                              selection(_abi.CS_SEL_CIRCLE, cx=GRID["width"] * 5, cy=0.0, r=1.5),
                              selection(_abi.CS_SEL_HLP | _abi.CS_SEL_SOURCE_SINK, hlp=hlp, source_sink=0)])
    assert rc == 0 and counts.tolist() == [len(full), 1, 1, 0]
    assert mesh.remove_selected(high_level_planner=still).tolist() == [limbo]
    assert len(mesh) == len(full) - 1
    mesh.step(0.05)


def _rank_selects(rank, world, port, out_path):
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
        notes = {"before": mesh.read_agents(), "answers": _answers(mesh)}
        bad = selection(_abi.CS_SEL_CIRCLE, r=-1.0)
        notes["refused"] = select(mesh, bad)[0] == mesh._C.c_size_t(-1).value
        notes["removed"] = mesh.remove_selected(rect=(24.0, 22.5, 37.25, 36.0)).tolist()
        notes["after_remove"] = mesh.read_agents()
        for _ in range(10):
            mesh.step(0.05, report=False)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_select_as_one_engine(tmp_path):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU: every rank passes the same selections and
    gets the whole answer, the single engine's."""
    import pickle
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "selects.pkl")
    procs = [ctx.Process(target=_rank_selects, args=(r, 2, 29781, out)) for r in range(2)]
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
    before = single.read_agents()
    want = _answers(single)
    across = want["a rectangle across both cuts"]
    x_of = dict(zip(before["id"].tolist(), before["x"].tolist()))
    assert any(x_of[i] < 30.0 for i in across) and any(x_of[i] >= 30.0 for i in across)  # (agents of both ranks)
    removed = single.remove_selected(rect=(24.0, 22.5, 37.25, 36.0)).tolist()
    after_remove = single.read_agents()
    for _ in range(10):
        single.step(0.05, report=False)
    end = single.read_agents()
    for n in notes:
        assert n["before"].tobytes() == before.tobytes()
        assert n["answers"] == want
        assert n["refused"] and n["removed"] == removed == across
        assert n["after_remove"].tobytes() == after_remove.tobytes()
        assert len(end) > 400 and n["agents"].tobytes() == end.tobytes()
