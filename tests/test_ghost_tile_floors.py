"""The floors of tests/test_gpu_queries_ghost_tiles.py without a GPU: the conditions that let those tests fail, counted by
tiles.TileLayout and the numpy restatements alone, on the scenes' crowds stepped ten times by the f64 oracle (the engine's
records differ from the oracle's in the last bits of an f32 offset; the floors are counts with room to spare, and the GPU
tests assert them again on the engine's own records before a tile is asked)."""
import numpy as np
import pytest

import odd_grids as og
from oracle_sim import OracleSimulation
from rmf_crowdsim_amd import LocationHash2D


@pytest.fixture(scope="module")
def stepped():
    """scene name -> (the oracle's records after og.STEPS steps, agent id -> the part of the scene it was added with)"""
    out = {}
    for name in sorted({case[0] for case in og.GHOST_CASES}):
        sc = og.scene(name)
        sim = OracleSimulation(LocationHash2D(**sc.grid))
        kept = og.populate_kept(sc, sim)
        for _ in range(og.STEPS):
            sim.step(og.DT)
        out[name] = (sim.read_agents(), {int(i): k for k, (_, ids) in enumerate(kept) for i in ids.tolist()})
    return out


@pytest.mark.parametrize("case", og.GHOST_CASES, ids=og.GHOST_IDS)
def test_the_floors_of_the_ghost_tile_tests_hold_by_the_restatements_alone(case, stepped, monkeypatch):
    rec, part_of = stepped[case[0]]
    sc, rects, held = og.ghost_case_floors(case, rec)  # (at least 20 ghosts a tile, the sides of the cuts, four own_*)
    for k, (own, ghosts) in enumerate(held):
        elsewhere = rec[~np.isin(rec["id"], np.concatenate([own["id"], ghosts["id"]]))]
        met = og.ask_tile_with_ghosts(None, sc, rects[k], own, ghosts, elsewhere, case[2], f"tile {k}", monkeypatch,
                                      part_of.__getitem__)
        print(f"tile {k}: {len(met)} floors met: {met}")
        assert len(met) == 24  # (every call of ask_tile_with_ghosts on every tile: none is left out)


def test_the_floors_of_the_recut_with_ghosts_hold_by_the_restatements_alone(stepped):
    sc = og.scene("lopsided")
    lay = og.layout(sc, (2, 2), 1, points=og.placed_cut_weights(sc, (2, 2), og.RECUT_FROM[0], og.RECUT_FROM[1], 1))
    og.ghost_recut_floors(sc, stepped["lopsided"][0], og.rects_of(lay.x_edges, lay.y_edges))
