"""The between-step device calls on a tile mesh (NativeTileMesh, in process) over the grids of
tests/test_gpu_queries_odd_grids.py: tiles with a non-zero origin on grids far longer than wide, of two-launch size, and
with a cell size whose multiples are inexact.  For every query family the mesh equals the single engine equals the numpy
restatement on the engine's OWN read_agents(), byte for byte (the raster's velocity sums within
field_reference.tolerance), at distances up to halo_cells * cell_size, where a mesh sees across a cut; the rays and the
two leg calls (cs_mesh_leg_conflicts, cs_mesh_leg_intervals) have no such limit.

A mesh takes no tile thinner than two halo rings along EITHER axis, cut or not, so the one-cell corridor and strip are
refused (asserted below); their place is taken by the nearest grids it accepts, two cells wide: 2 x 2,000,003 in
(3, 1) tiles and 2,000,003 x 2 in (1, 3).  Four agents are written astride every cut, so that pairs across each cut
exist whatever the crowd; the restatement alone counts them first.  The agents written astride the cuts are then read
by id, and at the end the agents of a rectangle are removed from the mesh and from the engine alike.  Needs an MI355X."""
import pytest

import odd_grids as og
from rmf_crowdsim_amd import CrowdSimError, LocationHash2D, Simulation
from rmf_crowdsim_amd.tiles import NativeTileMesh

pytestmark = pytest.mark.gpu

MESHES = [("two-launch", (2, 2), 1, 4.0), ("tall5", (3, 1), 1, 1.0), ("tall5", (1, 2), 1, 1.0),
          ("corridor2", (3, 1), 1, 1.0), ("strip2", (1, 3), 1, 1.0), ("odd-cell", (2, 2), 3, 1.0)]


@pytest.mark.parametrize("name,shape", [("corridor", (3, 1)), ("strip", (1, 3))])
def test_a_mesh_refuses_a_grid_one_cell_across(name, shape):
    sc = og.scene(name)
    with pytest.raises(CrowdSimError, match="thinner than two halo rings"):
        NativeTileMesh(LocationHash2D(**sc.grid), shape, 1)


@pytest.mark.parametrize("name,shape,halo,scale", MESHES, ids=[f"{m[0]}-{m[1][0]}x{m[1][1]}" for m in MESHES])
def test_a_mesh_answers_every_call_as_one_engine(name, shape, halo, scale, monkeypatch):
    sc = og.scene(name)
    mesh = og.stepped(sc, lambda grid: NativeTileMesh(LocationHash2D(**grid), shape, halo))
    single = og.stepped(sc, lambda grid: Simulation(LocationHash2D(**grid)))
    with og.released(mesh, single):
        rects = mesh.tile_rects()
        assert len(rects) == shape[0] * shape[1] and int((rects[:, [0, 2]] > 0).any(axis=1).sum()) == len(rects) - 1
        assert single.read_agents().tobytes() == mesh.read_agents().tobytes()
        w = og.astride_cuts(sc, single.read_agents(), rects)
        for t in (mesh, single):
            t.write_agents(w, fields=("position",))
        rec = single.read_agents()
        assert rec.tobytes() == mesh.read_agents().tobytes()
        assert int((mesh.tile_counts() > 0).sum()) >= 2
        limit = halo * sc.cell
        og.cut_floor(sc, rec, rects, limit)
        # (every family, the by-id reads and at the end the removal: odd_grids.ask_mesh_as_engine)
        og.ask_mesh_as_engine(mesh, single, sc, rec, f"{name} in {shape[0]} x {shape[1]} tiles", halo, scale, monkeypatch,
                              longest=1000.0 if name == "corridor2" else og.INF, by_id=w["id"][::-1])
