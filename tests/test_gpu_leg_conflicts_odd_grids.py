"""Paths against the moving crowd (cs_leg_conflicts, cs_mesh_leg_conflicts) on the grids of tests/odd_grids.py: one cell
wide or high and two million cells long, a cell size whose multiples are inexact, an offset that dwarfs the cell; on one
engine and on tile meshes.  Distances are scaled to the cell size; the engine (and the mesh) equal the numpy restatement
(tests/legs_reference.py) on the engine's OWN read_agents(), byte for byte.  (tests/test_gpu_queries_odd_grids.py and its
mesh twin ask the same, and cs_leg_intervals, on the rest of the grids of tests/odd_grids.py.)"""
import pytest

import close_pairs_reference as pairs_ref
import odd_grids as og
from rmf_crowdsim_amd import LocationHash2D, Simulation
from rmf_crowdsim_amd.tiles import NativeTileMesh

pytestmark = pytest.mark.gpu
# (shared with the other odd-grid modules since cs_leg_intervals is asked there too: they live in tests/odd_grids.py)
from odd_grids import WHOLE_WALK, ask_legs, long_axis_legs  # noqa: F401


@pytest.mark.parametrize("name", ["corridor", "strip", "odd-cell", "odd-far"])
def test_legs_on_one_engine(name):
    sc = og.scene(name)
    sim = og.stepped(sc, lambda grid: Simulation(LocationHash2D(**grid)))
    with og.released(sim):
        rec = sim.read_agents()
        assert pairs_ref.takes_part(rec, sc.grid).all()
        ask_legs(sim, sc, rec, name)
        assert sim.read_agents().tobytes() == rec.tobytes()


@pytest.mark.parametrize("name,shape,halo", [("odd-cell", (2, 2), 3), ("corridor2", (3, 1), 1)])
def test_legs_on_a_mesh(name, shape, halo):
    sc = og.scene(name)
    mesh = og.stepped(sc, lambda grid: NativeTileMesh(LocationHash2D(**grid), shape, halo))
    single = og.stepped(sc, lambda grid: Simulation(LocationHash2D(**grid)))
    with og.released(mesh, single):
        rec = single.read_agents()
        assert rec.tobytes() == mesh.read_agents().tobytes()
        assert int((mesh.tile_counts() > 0).sum()) >= 2
        want = ask_legs(single, sc, rec, f"{name} (engine)")
        ask_legs(mesh, sc, rec, f"{name} in {shape[0]} x {shape[1]} tiles", want=want)
        assert rec.tobytes() == mesh.read_agents().tobytes() == single.read_agents().tobytes()
