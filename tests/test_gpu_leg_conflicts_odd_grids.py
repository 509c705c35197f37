"""Paths against the moving crowd (cs_leg_conflicts, cs_mesh_leg_conflicts) on the grids of tests/odd_grids.py: one cell
wide or high and two million cells long, a cell size whose multiples are inexact, an offset that dwarfs the cell; on one
engine and on tile meshes.  Distances are scaled to the cell size; the engine (and the mesh) equal the numpy restatement
(tests/legs_reference.py) on the engine's OWN read_agents(), byte for byte."""
import numpy as np
import pytest

import close_pairs_reference as pairs_ref
import legs_reference as legs_ref
import odd_grids as og
from rmf_crowdsim_amd import LocationHash2D, Simulation
from rmf_crowdsim_amd.tiles import NativeTileMesh
from test_gpu_leg_conflicts import leg_sets, speeds

pytestmark = pytest.mark.gpu
INF = float("inf")
# (a wave walks the rows of a grid one after the other: the two-million-row corridors are not walked whole)
WHOLE_WALK = {"corridor": False, "corridor2": False, "strip": True, "odd-cell": True, "odd-far": True}


def long_axis_legs(sc, rec, stretch=800.0):
    """16 legs along the grid's long axis (y on a grid wider than high) from 5 m outside its low end, or from 200 m before
    the crowd where that is nearer, through the first `stretch` metres of the crowd in 8 s; spread over the crowd's
    extent across that axis and 2 m to either side of it"""
    gx0, gx1, gy0, gy1 = pairs_ref.rectangle(sc.grid)
    k = np.arange(16) / 15.0
    along, across, g_lo = (rec["x"], rec["y"], gx0) if sc.rows >= sc.cols else (rec["y"], rec["x"], gy0)
    begin = max(g_lo - 5.0, float(along.min()) - 200.0)
    run = (float(along.min()) - begin) + min(stretch, float(along.max() - along.min())) + 5.0
    side = (float(across.min()) - 2.0) + k * (float(across.max() - across.min()) + 4.0)
    if sc.rows >= sc.cols:
        return legs_ref.legs_array(np.column_stack([np.full(16, begin), side]), (run / 8.0, 0.0), 0.0, 8.0)
    return legs_ref.legs_array(np.column_stack([side, np.full(16, begin)]), (0.0, run / 8.0), 0.0, 8.0)


def ask_legs(sim, sc, rec, name, want=None):
    """The leg sets and the long-axis legs at distances of 0.4 and 0.8 cells, the second with the speed filter between
    the two walking speeds of the scene; where the grid allows, the first hundred legs at speed_max = +inf (the whole
    walk).  The classes by the restatement alone (printed, then asserted), then the engine.  -> the restatement's rows"""
    pace = float(np.median(speeds(rec)))
    legs = np.concatenate([leg_sets(rec, sc.grid), long_axis_legs(sc, rec)])
    asks = [(legs, 0.4 * sc.cell, 2.0), (legs, 0.8 * sc.cell, pace)]
    if WHOLE_WALK[sc.name]:
        asks.append((np.concatenate([legs[:100], legs[-16:]]), 0.4 * sc.cell, INF))
    out = []
    for k, (l, distance, speed_max) in enumerate(asks):
        w = legs_ref.conflicts(rec, sc.grid, l, distance, speed_max) if want is None else want[k]
        moving, still, miss = legs_ref.classes(w)
        along = int((w["id"][-16:] != legs_ref.NO_HIT).sum())
        print(f"{name}, legs {(distance, speed_max)}: restatement alone: {still} conflicts at s == 0, {moving} at s > 0, "
              f"{miss} misses; {along} of the 16 long-axis legs conflict")
        assert (still >= 5 and moving >= 5 and miss >= 5) if k < 2 else (still + moving >= 5 and miss >= 1)
        legs_ref.agree(sim, rec, sc.grid, l, distance, speed_max, name=f"{name}, legs {(distance, speed_max)}", want=w)
        out.append(w)
    assert (out[0]["id"][-16:] != legs_ref.NO_HIT).sum() >= 2  # (somebody stands in the way of the long-axis legs)
    return out


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
