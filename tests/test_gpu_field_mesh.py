"""Rasterising the crowd on a tile mesh (cs_mesh_agent_field; NativeTileMesh.agent_field): every tile rasterises the agents
it owns, only the part of the raster a tile touched travels, and the mesh gives the single engine's raster: counts equal,
sums within the bound of tests/field_reference.py, in process (2 x 2 tiles) and over two ranks of a host transport, where
every rank gets the same bytes.  What a rank contributes does not grow with the crowd."""
import numpy as np
import pytest

from rmf_crowdsim_amd import CrowdSimError, LocationHash2D, NoLocalPlan, Selection, Simulation, StubHighLevelPlan, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from field_reference import check, desc, field, last_error, raster
from select_reference import Ledger, drain, keep_events, selection
from test_gpu_agent_write_mesh import GRID, _scene

pytestmark = pytest.mark.gpu


def _rasters():
    """(name, desc): the cuts of a 2 x 2 mesh lie at 30 m, that of the 2 x 1 mesh of the two ranks at x = 30 m."""
    return [("one bin", desc(0.0, 0.0, 60.0, 60.0, 1, 1)),
            ("across all four tiles", desc(10.0, 10.0, 2.5, 2.5, 16, 16)),
            ("bin edges on the cuts", desc(0.0, 0.0, 3.0, 3.0, 20, 20)),
            ("inside one tile", desc(31.0, 31.0, 0.5, 0.5, 20, 20)),
            ("fine, non-square, across the cuts", desc(5.0, 5.0, 0.2, 0.35, 256, 150)),
            ("half outside the grid", desc(25.0, -30.0, 1.0, 1.0, 64, 64)),
            ("nobody", desc(200.0, 200.0, 1.0, 1.0, 8, 8))]


def _filters():
    return [("no filter", None),
            ("a rectangle across both cuts", selection(_abi.CS_SEL_RECT, x0=24.0, y0=22.5, x1=37.25, y1=36.0)),
            ("the sink's crowd", selection(_abi.CS_SEL_SOURCE_SINK, source_sink=0)),
            ("on their first leg", selection(_abi.CS_SEL_WAYPOINT | _abi.CS_SEL_SPEED, wp_lo=0, wp_hi=0, speed_lo=0.3,
                                             speed_hi=3.0))]


def _answers(t):
    """What a mesh or an engine answers to every raster and filter, by the C entry points"""
    out = {}
    for name, d in _rasters():
        for f_name, sel in _filters():
            rc, count, sums = field(t, d, sel)
            assert rc == 0, (name, f_name, last_error(t))
            rc, only, none = field(t, d, sel, want="count")
            assert rc == 0 and none is None and np.array_equal(only, count), (name, f_name)
            out[(name, f_name)] = (count, sums)
    return out


def _compare(answers, rec, cols, who):
    crowded = 0
    for name, d in _rasters():
        for f_name, sel in _filters():
            count, sums = answers[(name, f_name)]
            n, _ = check(f"{who}: {name}, {f_name}", count, sums, raster(d, rec, sel, *cols))
            crowded += n
    return crowded


def test_a_mesh_rasterises_as_one_engine():
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
    cols = led.columns(rec)
    on_mesh, on_engine = _answers(mesh), _answers(single)
    assert _compare(on_engine, rec, cols, "engine") > 100
    assert _compare(on_mesh, rec, cols, "mesh") > 100
    for key in on_engine:
        assert on_mesh[key][0].tobytes() == on_engine[key][0].tobytes(), key
    count = on_engine[("across all four tiles", "no filter")][0]
    assert count[:6, :6].sum() > 0 and count[:6, 10:].sum() > 0 and count[10:, :6].sum() > 0 and count[10:, 10:].sum() > 0
    assert on_engine[("inside one tile", "no filter")][0].sum() > 20
    assert on_engine[("one bin", "the sink's crowd")][0].sum() >= 2 and on_engine[("nobody", "no filter")][0].sum() == 0
    # the Python surface of the mesh
    d = _rasters()[1][1]
    count, sum_v = mesh.agent_field((10.0, 10.0), 2.5, (16, 16), velocity=True)
    check("NativeTileMesh.agent_field", count, sum_v, raster(d, rec))
    only = mesh.agent_field((10.0, 10.0), (2.5, 2.5), (16, 16), selection=Selection(rect=(24.0, 22.5, 37.25, 36.0)))
    assert only.dtype == np.uint32 and np.array_equal(only, on_engine[("across all four tiles", "a rectangle across both cuts")][0])
    # a refused raster, and the mesh steps on as the engine does
    with pytest.raises(CrowdSimError, match="agent_field"):
        mesh.agent_field((0.0, 0.0), 0.0, (4, 4))
    rc, count, sums = field(mesh, desc(0.0, 0.0, 1.0, float("nan"), 4, 4), fill=0xAB)
    assert rc == 3 and "agent_field" in last_error(mesh)
    assert (count.view(np.uint8) == 0xAB).all() and (sums.view(np.uint8) == 0xAB).all()
    assert mesh.read_agents().tobytes() == rec.tobytes()
    for _ in range(10):
        for t in (mesh, single):
            t.step(0.05)
    assert mesh.read_agents().tobytes() == single.read_agents().tobytes()


def test_what_a_rank_contributes_does_not_grow_with_the_crowd():
    """The same raster over a crowd and over the same crowd with a second one standing inside it: the bounding boxes of
    the bins the tiles touch are the same, so the contribution is the same number of bytes; after steps (the denser crowd
    spreads differently) it stays below what the raster and the tiles alone allow."""
    d = desc(10.0, 10.0, 2.5, 2.5, 16, 16)
    ix, iy = np.meshgrid(np.arange(24), np.arange(24), indexing="ij")
    pts = np.stack([18.0 + 1.05 * ix.ravel() + 0.01 * iy.ravel(), 17.5 + 1.1 * iy.ravel() + 0.02 * ix.ravel()], axis=1)
    centre = pts.mean(axis=0)
    inner = centre + 0.93 * (pts - centre) + 0.013
    still = StubHighLevelPlan((0.2, 0.1))
    sent = {}
    for crowd in ("once", "twice"):
        mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 2), 1)
        mesh.add_agents(pts, still, NoLocalPlan(), 2.0)
        if crowd == "twice":
            mesh.add_agents(inner, still, NoLocalPlan(), 2.0)
        for velocity in (False, True):
            rc, count, sums = field(mesh, d, want="both" if velocity else "count")
            assert rc == 0 and int(count.sum()) == len(mesh)
            sent[(crowd, velocity, 0)] = int(mesh._lib.cs_mesh_field_gather_bytes(mesh._mesh))
        for _ in range(5):
            mesh.step(0.05)
        rc, count, sums = field(mesh, d)
        assert rc == 0 and int(count.sum()) == len(mesh)
        check(f"the crowd {crowd}", count, sums, raster(d, mesh.read_agents()))
        sent[(crowd, True, 5)] = int(mesh._lib.cs_mesh_field_gather_bytes(mesh._mesh))
    print(sent)
    assert len(pts) * 2 == 1152
    for velocity in (False, True):
        assert sent[("twice", velocity, 0)] == sent[("once", velocity, 0)] > 0
    assert sent[("once", False, 0)] < sent[("once", True, 0)]
    # the most a rank of 4 tiles may send: a header word, per tile 4 words of box and at most the whole raster (a word
    # of padding for the counts)
    most = 8 * (1 + 4 * 4) + 4 * (d.nx * d.ny * 20 + 8)
    assert sent[("twice", True, 5)] <= most and sent[("once", True, 5)] <= most
    # and far less than a whole raster per tile here: the four boxes tile the raster, give or take the bins on the cuts
    assert sent[("twice", True, 5)] <= 8 * (1 + 4 * 4) + (d.nx + 2) * (d.ny + 2) * 20 + 4 * 8


def test_a_mesh_bins_the_agent_its_index_refused():
    mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 2), 1)
    _scene(mesh)
    for _ in range(3):
        mesh.step(0.05)
    where = (GRID["width"] * 5 + 0.75, 1.0)
    with pytest.raises(CrowdSimError):
        mesh.add_agents([where], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.5)
    full = mesh.read_agents()
    assert (full["x"] > GRID["width"]).sum() == 1
    round_it = desc(where[0] - 1.0, 0.0, 0.5, 0.5, 4, 4)
    rc, count, sums = field(mesh, round_it)
    assert rc == 0 and count[2, 2] == 1 and int(count.sum()) == 1
    check("round the agent", count, sums, raster(round_it, full))
    everything = desc(-10.0, -10.0, GRID["width"] * 6.0, GRID["height"] * 6.0, 2, 2)
    rc, count, sums = field(mesh, everything)
    assert rc == 0 and int(count.sum()) == len(full)
    check("the whole plane", count, sums, raster(everything, full))


def _rank_fields(rank, world, port, out_path):
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
        rc, count, sums = field(mesh, _rasters()[3][1])
        notes["sent_inside_one_tile"] = int(mesh._lib.cs_mesh_field_gather_bytes(mesh._mesh))
        rc, count, sums = field(mesh, desc(0.0, 0.0, -1.0, 1.0, 4, 4), fill=0xAB)
        notes["refused"] = (rc == 3 and "agent_field" in last_error(mesh) and bool((count.view(np.uint8) == 0xAB).all())
                            and bool((sums.view(np.uint8) == 0xAB).all()))
        for _ in range(10):
            mesh.step(0.05, report=False)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_rasterise_as_one_engine(tmp_path):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU: every rank passes the same rasters and gets
    the whole raster, the single engine's counts and, both ranks alike to the bit, sums within the bound."""
    import pickle
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "fields.pkl")
    procs = [ctx.Process(target=_rank_fields, args=(r, 2, 29787, out)) for r in range(2)]
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
    led = Ledger(single).watch()
    _scene(single)
    keep_events(single)
    for _ in range(25):
        single.step(0.05, report=False)
    led.hear(drain(single))
    before = single.read_agents()
    cols = led.columns(before)
    want = _answers(single)
    for _ in range(10):
        single.step(0.05, report=False)
    end = single.read_agents()
    for r, n in enumerate(notes):
        assert n["before"].tobytes() == before.tobytes()
        assert _compare(n["answers"], before, cols, f"rank {r}") > 100
        for key in want:
            assert n["answers"][key][0].tobytes() == want[key][0].tobytes(), key
            assert n["answers"][key][0].tobytes() == notes[0]["answers"][key][0].tobytes(), key
            assert n["answers"][key][1].tobytes() == notes[0]["answers"][key][1].tobytes(), key  # (the same order of adding)
        assert n["refused"]
        assert len(end) > 400 and n["agents"].tobytes() == end.tobytes()
    across = want[("across all four tiles", "no filter")][0]
    assert across[:, :8].sum() > 0 and across[:, 8:].sum() > 0  # (agents of both ranks)
    # the raster inside the tile of rank 1: rank 0 touched no bin and sent a header and an empty box
    print([n["sent_inside_one_tile"] for n in notes])
    assert notes[0]["sent_inside_one_tile"] == 8 * 5 and notes[1]["sent_inside_one_tile"] > 8 * 5
