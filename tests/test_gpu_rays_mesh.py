"""Rays on a tile mesh (cs_mesh_cast_rays; NativeTileMesh.cast_rays / count_ray_hits): every tile casts all rays against
the agents it owns, its walk clipped to its owned cells, and the rows are merged by the minimum of (t, id); the mesh gives
the single engine's answer byte for byte, which is also the restatement's (tests/rays_reference.py), whatever t_max and
radius are.  No halo exchange is made for it: the next steps of the mesh are those of a mesh that never asked."""
import numpy as np
import pytest

from rmf_crowdsim_amd import CS_CFG_WIDE_IDS, LocationHash2D, Simulation, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from rays_reference import NO_HIT, SIZE_MAX, agree, call, cast, last_error, rays_array
from select_reference import selection
from test_gpu_agent_write import _add_crossing
from test_gpu_encounters_mesh import _crowd
from test_gpu_rays import ray_sets

pytestmark = pytest.mark.gpu
INF = float("inf")


def _same(mesh, single, rec, grid, rays, radius, sel=None, name=""):
    """mesh == single engine == restatement; `sel` is a rectangle (no ledger needed)"""
    want = agree(single, rec, grid, rays, radius, sel, name=name + " (engine)")
    agree(mesh, rec, grid, rays, radius, sel, name=name + " (mesh)", want=want)
    return want


def _long_rays(rec, grid, cuts_x, cuts_y):
    """Rays that cross every cut: a comb of rays along x and along y over the whole grid, from outside it, in both
    senses, diagonals from corner to corner, and +inf for t_max"""
    size = grid["width"]
    at = np.linspace(42.0, 126.0, 57)
    o = [np.column_stack([np.full_like(at, -7.0), at]), np.column_stack([np.full_like(at, size + 7.0), at + 0.3]),
         np.column_stack([at, np.full_like(at, -7.0)]), np.column_stack([at + 0.3, np.full_like(at, size + 7.0)]),
         np.column_stack([at - 50.0, np.full_like(at, -3.0)]), np.column_stack([at + 60.0, np.full_like(at, size + 3.0)])]
    u = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (0.6, 0.8), (-0.8, -0.6)]
    rays = rays_array(np.concatenate(o), np.concatenate([np.repeat([d], len(at), axis=0) for d in u]))
    assert cuts_x or cuts_y
    return rays


@pytest.mark.parametrize("shape,halo", [((2, 2), 1), ((1, 3), 1)])
def test_a_mesh_casts_the_rays_of_one_engine(shape, halo):
    pts, group, grid = _crowd()
    mesh = NativeTileMesh(LocationHash2D(**grid), shape, halo)
    single = Simulation(LocationHash2D(**grid))
    for t in (mesh, single):
        _add_crossing(t, pts, group)
        for _ in range(40):
            t.step(0.05)
    rec = single.read_agents()
    # a few agents written far beyond the crowd, so that every tile of three holds somebody: x and y in [150, 200]
    w = rec[50:90].copy()
    rng = np.random.default_rng(5)
    w["x"], w["y"] = rng.uniform(150.0, 200.0, len(w)), rng.uniform(150.0, 200.0, len(w))
    w["x"][:10] = rng.uniform(42.0, 100.0, 10)
    for t in (mesh, single):
        t.write_agents(w, fields=("position",))
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    assert (mesh.tile_counts() > 0).sum() >= 3
    cell = grid["cell_size"]
    rows_, cols_ = int(grid["height"] / cell), int(grid["width"] / cell)
    cuts_x = [round(k * rows_ / shape[0]) * cell for k in range(1, shape[0])]
    cuts_y = [round(k * cols_ / shape[1]) * cell for k in range(1, shape[1])]
    for radius, reach in ((0.4, 2.0), (0.2, INF), (3.0, 30.0)):  # (3 m: wider than a halo of one cell)
        _same(mesh, single, rec, grid, ray_sets(rec, grid, reach), radius, name=f"{shape}, the ray sets, {(radius, reach)}")
    rays = _long_rays(rec, grid, cuts_x, cuts_y)
    pos = {int(r["id"]): (float(r["x"]), float(r["y"])) for r in rec}
    sides = 0  # hits on the far side of a cut from the origin
    for radius in (0.2, 0.02):
        want = _same(mesh, single, rec, grid, rays, radius, name=f"{shape}, long rays, radius {radius}")
        hit = want["id"] != NO_HIT
        for r, h in zip(rays[hit], want[hit]):
            x, y = pos[int(h["id"])]
            sides += any((r["ox"] < c) != (x < c) for c in cuts_x) or any((r["oy"] < c) != (y < c) for c in cuts_y)
        print(f"{shape}, radius {radius}: {int(hit.sum())} of {len(rays)} long rays hit, {sides} so far beyond a cut")
    assert sides >= 20
    # the first hit two tiles away: only the agents beyond 144 m are targets, the rays start below 72 m
    far = selection(_abi.CS_SEL_RECT, x0=144.0, y0=144.0, x1=INF, y1=INF)
    there = rec[(rec["x"] >= 144.0) & (rec["y"] >= 144.0)]
    assert len(there) >= 20
    aimed = rays_array(np.column_stack([np.full(len(there), 50.0), np.full(len(there), 45.0)]),
                       np.column_stack([there["x"] - 50.0, there["y"] - 45.0]), 1.5)
    want = _same(mesh, single, rec, grid, aimed, 0.3, far, name=f"{shape}, two tiles away")
    assert (want["id"] != NO_HIT).all() and np.isin(want["id"], there["id"]).all() and (want["t"] > 0.5).all()
    nobody = _same(mesh, single, rec, grid, aimed, 0.3, None, name=f"{shape}, the same through the crowd")
    assert (nobody["t"] <= want["t"]).all()
    # refusals leave the mesh usable and write nothing
    bad = rays.copy()
    bad["uy"][5] = float("nan")
    for rays_, radius in ((bad, 0.2), (rays, -1.0)):
        n, out = call(mesh, rays_, radius, fill=0xAB)
        assert n == SIZE_MAX and "cast_rays" in last_error(mesh) and (out.view(np.uint8) == 0xAB).all()
    assert "ray 5" in (call(mesh, bad, 0.2), last_error(mesh))[1]
    # the Python surface of the mesh
    o, u = np.column_stack([rays["ox"], rays["oy"]]), np.column_stack([rays["ux"], rays["uy"]])
    want = cast(rec, grid, rays, 0.2)
    assert mesh.cast_rays(o, u, 0.2).tobytes() == want.tobytes()
    assert mesh.count_ray_hits(o, u, 0.2) == int((want["id"] != NO_HIT).sum())
    assert mesh.cast_rays(np.zeros((0, 2)), np.zeros((0, 2)), 0.2).shape == (0,)
    assert mesh.read_agents().tobytes() == rec.tobytes()


def test_twins_and_wide_ids(monkeypatch):
    """2 x 2 tiles with 64-bit ids from 2^40 on: `ignore` in external ids, ids above 2^32 back; and the next steps of the
    mesh that asked are those of the mesh that never did."""
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(2 ** 40 + 1))
    pts, group, grid = _crowd()
    meshes = [NativeTileMesh(LocationHash2D(**grid), (2, 2), 1, flags=CS_CFG_WIDE_IDS) for _ in range(2)]
    single = Simulation(LocationHash2D(**grid), flags=CS_CFG_WIDE_IDS)
    monkeypatch.delenv("CS_FIRST_AGENT_ID")
    mesh, twin = meshes
    for t in (mesh, twin, single):
        _add_crossing(t, pts, group)
        for _ in range(10):
            t.step(0.05)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes() and int(rec["id"].min()) > 2 ** 40
    for k in range(10):
        rays = ray_sets(rec, grid, 6.0, beams=90)
        if k in (0, 9):
            want = _same(mesh, single, rec, grid, rays, 0.25, name=f"wide ids, step {k}")
            hit = want["id"] != NO_HIT
            fans = rays["ignore"] != _abi.CS_NO_HIT
            assert hit.sum() > 360 and int(want["id"][hit].min()) > 2 ** 40
            assert fans.sum() == 360 and (want["id"][fans] != rays["ignore"][fans]).all()
        else:
            assert 0 < call(mesh, rays, 0.25, rows=False)[0] < len(rays)
        for t in (mesh, twin, single):
            t.step(0.05)
        rec = single.read_agents()
    assert mesh.read_agents().tobytes() == twin.read_agents().tobytes() == rec.tobytes()


def _two_rank_rays(rec, grid):
    rays = ray_sets(rec, grid, 8.0, beams=90)
    comb = np.linspace(5.0, 55.0, 26)
    across = rays_array(np.column_stack([np.full_like(comb, -4.0), comb]), np.repeat([[1.0, 0.0]], len(comb), axis=0))
    return np.concatenate([rays, across])


def _two_rank_answers(t, rec, grid):
    rays = _two_rank_rays(rec, grid)
    left = selection(_abi.CS_SEL_RECT, x0=0.0, y0=0.0, x1=30.0, y1=60.0)  # one rank's side
    out = []
    for radius, sel in ((0.2, None), (0.5, None), (0.3, left), (0.0, None)):
        n, rows = call(t, rays, radius, sel, fill=0xEE)
        out.append((n, rows.tobytes(), call(t, rays, radius, sel, rows=False)[0]))
    return out


def _rank_casts_rays(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import TorchHostTransport
    from test_gpu_agent_write_mesh import GRID, _scene
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 1), 1, device=0, rank=rank, n_ranks=world,
                              host_transport=TorchHostTransport(dist))
        _scene(mesh)
        for _ in range(25):
            mesh.step(0.05, report=False)
        before = mesh.read_agents()
        notes = {"before": before, "answers": _two_rank_answers(mesh, before, GRID)}
        notes["refused"] = call(mesh, _two_rank_rays(before, GRID), float("nan"))[0] == SIZE_MAX
        rays = _two_rank_rays(before, GRID)
        o, u = np.column_stack([rays["ox"], rays["oy"]]), np.column_stack([rays["ux"], rays["uy"]])
        notes["python"] = mesh.cast_rays(o, u, 0.2, t_max=rays["t_max"], ignore=rays["ignore"])
        for _ in range(10):
            mesh.count_ray_hits(o, u, 0.2)
            mesh.step(0.05, report=False)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_give_the_rows_of_one_engine(tmp_path):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU: the rows travel through the host transport's
    gather, every rank gets the whole answer, the single engine's, and steps on as it."""
    import pickle
    import torch.multiprocessing as mp
    from test_gpu_agent_write_mesh import GRID, _scene
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "rays.pkl")
    procs = [ctx.Process(target=_rank_casts_rays, args=(r, 2, 29817, out)) for r in range(2)]
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
    want = _two_rank_answers(single, before, GRID)
    rays = _two_rank_rays(before, GRID)
    rows = cast(before, GRID, rays, 0.2)
    assert want[0][1] == rows.tobytes() and 0 < want[0][0] < len(rays) and want[3][0] == 0
    x_of = dict(zip(before["id"].tolist(), before["x"].tolist()))
    hit = rows["id"] != NO_HIT
    assert any((float(r["ox"]) < 30.0) != (x_of[int(h["id"])] < 30.0) for r, h in zip(rays[hit], rows[hit]))  # (the other rank's)
    for _ in range(10):
        single.step(0.05, report=False)
    end = single.read_agents()
    for n in notes:
        assert n["before"].tobytes() == before.tobytes()
        assert n["answers"] == want and n["refused"]
        assert n["python"].tobytes() == rows.tobytes()
        assert len(end) > 400 and n["agents"].tobytes() == end.tobytes()
