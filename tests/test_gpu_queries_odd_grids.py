"""The between-step device calls of one engine (select / count / remove by selection, cs_agent_field, cs_close_pairs,
cs_agent_clusters, cs_agent_neighbours, cs_encounters, cs_cast_rays, cs_leg_conflicts, cs_leg_intervals, write_agents and
the by-id reads) on the grids
their own tests leave out: those all run on square grids of 2 m cells (a power of two: index * cell is exact) of a few
thousand cells from offset (0, 0).  Here: grids with far more rows than columns and the reverse, one cell wide and one
cell high, 16.8M cells (the two-launch scan) 50 km from the origin, cell indices near 2^31, a cell of 0.7 m and of
2.3 m (no multiple is exact, the last partial cell is cut off) under an offset of millions of metres.

Every comparison is against the numpy restatements (tests/*_reference.py) applied to the engine's OWN read_agents(),
through tests/odd_grids.py: ids, counts, orders and the bits of every f64 are exact, the raster's velocity sums keep
field_reference.tolerance.  Crowds are 1,300 to 3,700 agents (the 64 x 64 crowd of the corner test: 4,498), stepped 10
steps of 0.1 s before they are asked.  What a test must not pass on nothing (pairs, pairs across scan tiles, the classes
of the rays and of the leg intervals, the agents written onto the edges and the legs that meet them) is counted by the
restatement alone, printed and asserted before the engine is asked.  Needs an MI355X."""
import numpy as np
import pytest

import close_pairs_reference as pairs_ref
import neighbours_reference as neighbours_ref
import odd_grids as og
from rmf_crowdsim_amd import LocationHash2D, Simulation

pytestmark = pytest.mark.gpu

# grid: (pairs within one cell at least, of them across a scan-tile boundary at least, cell scale of the encounters and
# the rays, the longest ray in metres: a wave walks the corridor's rows one after the other)
ONE_SIDED = {"corridor": (400, None, 1.0, 1000.0), "strip": (400, None, 1.0, og.INF), "tall5": (1500, None, 1.0, og.INF),
             "two-launch": (2500, 1000, 4.0, og.INF)}


ALL = ("row", "column", "cells")  # agents were written into the last cell or onto the high edges: somebody is there


def _engine(grid):
    return Simulation(LocationHash2D(**grid))


@pytest.mark.parametrize("name", list(ONE_SIDED))
def test_every_call_on_one_sided_and_two_launch_grids(name, monkeypatch):
    """1 x 2,000,003 (rows >> columns, one column), 2,000,003 x 1 (one row: the rays' chunk loop runs 125,000 chunks),
    5 x 200,000, and 4097 x 4097 cells of 4 m from (-30000, 45000): every call against its restatement; on the strip and
    on tall5 also 16 rays along the long axis from outside the low end, some of which walk the whole grid and hit nobody;
    then a twin loses the agents of a rectangle."""
    least, least_across, scale, longest = ONE_SIDED[name]
    sc = og.scene(name)
    sim, twin = og.stepped(sc, _engine), og.stepped(sc, _engine)
    with og.released(sim, twin):
        rec = sim.read_agents()
        assert 1300 <= len(rec) <= 3700 and pairs_ref.takes_part(rec, sc.grid).all()
        og.pair_floor(sc, rec, least, least_across)
        og.ask_everything(sim, sc, rec, name, monkeypatch, scale, longest)
        if name in ("strip", "tall5"):
            og.ask_long_axis_rays(sim, sc, rec, name)
        og.ask_removal(twin, sc, rec, name)


@pytest.mark.parametrize("name", ["corridor", "tall5", "two-launch"])
def test_writes_between_steps_then_every_call_with_no_step_between(name, monkeypatch):
    """write_agents moves 16 agents into the grid's last cell, 16 into cell 0 and 8 to either side of a scan-tile
    boundary (flat index k * 1,024 - 1 | k * 1,024); every call is asked at once, and the moved agents are read by id;
    then one step, and every call again."""
    least, _, scale, longest = ONE_SIDED[name]
    sc = og.scene(name)
    sim = og.stepped(sc, _engine)
    with og.released(sim):
        w, k = og.move_into_cells(sc, sim.read_agents())
        sim.write_agents(w, fields=("position", "velocity"))
        rec = og.check_moved(sim, sc, w, k, f"{name}, written")
        og.ask_everything(sim, sc, rec, f"{name}, written", monkeypatch, scale, longest, ray_floors=False,
                          at_end=ALL)
        sim.step(og.DT)
        rec = sim.read_agents()
        assert np.isfinite(rec["x"]).all() and np.isfinite(rec["y"]).all()
        og.pair_floor(sc, rec, least)
        og.ask_everything(sim, sc, rec, f"{name}, one step later", monkeypatch, scale, longest, ray_floors=False,
                          at_end=ALL)


@pytest.mark.parametrize("name", ["odd-cell", "odd-far"])
def test_cells_whose_multiples_are_inexact_and_an_offset_that_dwarfs_the_cell(name, monkeypatch):
    """176 x 111 cells of 0.7 m from (-1234.5, 6789.25) (the grid's width ends in a partial cell that is cut off), and
    900 x 700 cells of 2.3 m from (3.0e6, -2.0e6) with the crowd by the high corner.  Eight agents are written just
    inside every edge and corner of the participants' rectangle (close_pairs_reference.rectangle), each with a partner a
    third of a cell further in, and two outside it that the index still takes: one below the low x edge, one beyond the
    last column (10 cm from the agent on that edge, and in no pair).  Both leg calls are also asked legs made for those
    agents (odd_grids.edge_legs).  The distance wider than the grid is asked on the 0.7 m grid, of the leg calls too; the
    Python surface of the leg calls (free_intervals, path_conflict) on the 2.3 m grid."""
    sc = og.scene(name)
    sim, twin = og.stepped(sc, _engine), og.stepped(sc, _engine)
    with og.released(sim, twin):
        w, ids = og.edge_agents(sc, sim.read_agents(), outsiders=2)
        for s in (sim, twin):
            s.write_agents(w, fields=("position",))
        rec = sim.read_agents()
        og.check_edges(sc, rec, w, ids, outsiders=2)
        og.pair_floor(sc, rec, 1500)
        # random legs seldom meet sixteen agents on the edges: legs made for them (and for the outsiders) are asked with
        # the others, by both leg calls
        edge, n_waits = og.edge_legs(sc, rec, w)
        og.check_edge_legs(sc, rec, w, ids, edge)
        lattice = rec[~np.isin(rec["id"], w["id"])]  # (the long-axis legs go through the crowd, not from edge to edge)
        pairs, _ = og.ask_everything(sim, sc, rec, name, monkeypatch, at_end=ALL, extra_legs=edge, legs_crowd=lattice)
        part = int(pairs_ref.takes_part(rec, sc.grid).sum())
        assert len(rec) - 2 - 5 <= part <= len(rec) - 2  # (the outsiders, and edge agents whose f32 offset rounds onto the edge)
        assert not np.isin(pairs[2.5][0], w["id"][16:].astype(np.uint64)).any()  # (the outsiders are in no pair)
        assert np.isin(ids.astype(np.uint64), pairs[0.6][0]).sum() >= 4  # (the edge agents are, with their partners)
        if name == "odd-cell":
            for distance in (2.0 * sc.grid["width"], og.INF):
                want, _ = pairs_ref.agree(sim, rec, sc.grid, distance, name=f"{name}, wider than the grid: {distance}")
                assert len(want) == part * (part - 1) // 2
                rows = neighbours_ref.agree(sim, rec, sc.grid, distance, name=f"{name}, wider than the grid: {distance}",
                                            min_counts=(0,))
                assert (rows["count"] == part - 1).all()
            og.ask_legs_wider_than_the_grid(sim, sc, rec, w, edge[:n_waits], name)
        else:  # (the Python surface of the leg calls where the offset is 3.0e6)
            og.ask_python_surface_of_the_legs(sim, sc, rec, name, lattice)
        og.ask_removal(twin, sc, rec, name)


def _dyadic(sim, rec, shift):
    """Write the positions of `rec` rounded to multiples of 2^-16 m, plus `shift`: exact in f64 and, relative to the
    cell, in f32, so that a crowd and its whole-cell translation hold the same numbers.  -> the engine's records"""
    w = rec.copy()
    w["x"] = np.round(rec["x"] * 65536.0) / 65536.0 + shift
    w["y"] = np.round(rec["y"] * 65536.0) / 65536.0 + shift
    sim.write_agents(w, fields=("position",))
    back = sim.read_agents()
    assert back["x"].tobytes() == w["x"].tobytes() and back["y"].tobytes() == w["y"].tobytes()
    return back


def _moved_legs(legs, shift):
    """The starts rounded to multiples of 2^-16 m, as the rays' origins are, plus `shift`"""
    l = legs.copy()
    l["x0"], l["y0"] = np.round(l["x0"] * 65536.0) / 65536.0 + shift, np.round(l["y0"] * 65536.0) / 65536.0 + shift
    return l


def _alike_where_t0_is_0(what, asked, small, big, rows_of):
    """The restatement's answers to the same asks on the small records and on the shifted ones: equal byte for byte for
    every leg with t0 == 0, where px = x + v * 0 is the dyadic x itself and every difference of the rule is the same
    number on both grids.  With t0 > 0 the sum x + v * t0 is rounded at another magnitude once the steps have given the
    velocities low bits (it is exact for the preferred velocities the crowd starts with): those legs are counted and
    printed, and each grid answers for them to its own restatement only."""
    for k, (l, s, b) in enumerate(zip(asked, small, big)):
        at_0 = l["t0"] == 0.0
        alike = rows_of(s, at_0).tobytes() == rows_of(b, at_0).tobytes()
        rest = rows_of(s, ~at_0).tobytes() == rows_of(b, ~at_0).tobytes()
        print(f"{what}, ask {k}: restatement alone: the {int(at_0.sum())} legs with t0 == 0 have {len(rows_of(s, at_0))} "
              f"rows, alike on both grids: {alike}; the other {int((~at_0).sum())} legs alike: {rest}")
        assert at_0.sum() >= 25 and len(rows_of(s, at_0)) >= 20 and alike, (what, k)


def test_every_call_in_the_top_corner_of_a_grid_at_the_31_bit_limit(monkeypatch):
    """The 64 x 64 crowd of the translation test of tests/test_gpu_large_grids.py on its own grid and shifted by 46,276
    whole cells into the top corner of the 46,340 x 46,340 grid (43 GB of cell tables: one such engine, here only, and
    the agents of the rectangle are removed from it at the end rather than from a twin).  After the 10 steps both crowds
    are written back with positions rounded to 2^-16 m (the read-back of the large grid rounds cell + offset once, so
    a stepped position may differ from the shifted one in its last bit): then the subtractions of every rule are the
    same numbers, and the large grid answers with the small grid's ids, counts and the bits of every d2 and t.  Each is
    also compared with the restatement on its own read-back.  The two leg calls are asked the small grid's legs, their
    starts rounded likewise and shifted with the crowd (_alike_where_t0_is_0 says for which legs the bytes are the same)."""
    shift = float(og.BIG - 64)
    small_sc, big_sc = og.corner_scene(64), og.corner_scene(og.BIG)
    small = og.stepped(small_sc, _engine)
    with og.released(small):
        rec_s = _dyadic(small, small.read_agents(), 0.0)
        og.pair_floor(small_sc, rec_s, 2500)
        pairs_s, enc_s = og.ask_everything(small, small_sc, rec_s, "64 x 64", monkeypatch, legs=False)
        # the two leg calls: the small grid's legs with dyadic starts, and the same legs shifted with the crowd.  Before
        # either engine is asked, the restatement alone says that both grids have the same answer
        rec_moved = rec_s.copy()
        rec_moved["x"], rec_moved["y"] = rec_s["x"] + shift, rec_s["y"] + shift
        legs_s = [_moved_legs(og.conflict_leg_set(small_sc, rec_s), 0.0), _moved_legs(og.interval_leg_set(small_sc, rec_s), 0.0)]
        legs_b = [_moved_legs(l, shift) for l in legs_s]
        pace = og.walking_pace(rec_s)
        asks = list(zip((0.4, 0.8, 0.4), (2.0, pace, og.INF)))
        hits = [[og.legs_ref.conflicts(r, sc.grid, l, d, v) for l, (d, v) in zip(og.asked_legs(sc, legs[0], conflicts=True), asks)]
                for sc, r, legs in ((small_sc, rec_s, legs_s), (big_sc, rec_moved, legs_b))]
        _alike_where_t0_is_0("leg conflicts", og.asked_legs(big_sc, legs_s[0], conflicts=True), hits[0], hits[1], lambda w, m: w[m])
        _, ivs_s = og.intervals_alone(small_sc, rec_s, "64 x 64, dyadic starts", legs_s[1])
        _, ivs_b = og.intervals_alone(big_sc, rec_moved, "the crowd and the legs shifted", legs_b[1])
        _alike_where_t0_is_0("leg intervals", og.asked_legs(small_sc, legs_s[1]), ivs_s, ivs_b,
                             lambda w, m: w[0][m[w[0]["leg"].astype(np.int64)]])
        og.ask_legs(small, small_sc, rec_s, "64 x 64, dyadic starts", want=hits[0], legs=legs_s[0])
        og.ask_intervals(small, small_sc, rec_s, "64 x 64, dyadic starts", want=ivs_s, legs=legs_s[1])
        rays_s = og.ray_queries(small_sc)
        sets = []
        for radius, reach in rays_s:
            r = og.ray_sets(rec_s, small_sc.grid, reach, beams=90)
            r["ox"], r["oy"] = np.round(r["ox"] * 65536.0) / 65536.0, np.round(r["oy"] * 65536.0) / 65536.0
            sets.append(r)
        hits_s = og.ask_rays(small, small_sc, rec_s, "64 x 64, dyadic origins", rays=sets)

    big = og.stepped(big_sc, _engine, shift=shift)
    with og.released(big):
        stepped = big.read_agents()
        rec_b = _dyadic(big, rec_s, shift)
        assert np.array_equal(stepped["vx"], rec_s["vx"]) and np.array_equal(stepped["vy"], rec_s["vy"])  # (stepped alike)
        for c in ("x", "y"):  # (where the steps left it, to the rounding to 2^-16 m)
            assert (np.abs(stepped[c] - (rec_s[c] + shift)) < 1e-4).all(), c
        assert (rec_b["id"] == rec_s["id"]).all() and rec_b["vx"].tobytes() == rec_s["vx"].tobytes()
        assert int(big_sc.flat_of(rec_b).max()) == og.BIG * og.BIG - 1  # (somebody stands in the last cell)
        pairs_b, enc_b = og.ask_everything(big, big_sc, rec_b, "46,340 x 46,340", monkeypatch, legs=False)
        # (the read-back IS the shifted crowd the restatement answered for above, in every field the leg rules read: the
        # large grid is compared with the restatement on its own read-back, and its bytes are the small grid's for every
        # leg with t0 == 0)
        assert all(rec_b[c].tobytes() == rec_moved[c].tobytes() for c in ("id", "x", "y", "vx", "vy"))
        og.ask_legs(big, big_sc, rec_b, "46,340 x 46,340, the small grid's legs", want=hits[1], legs=legs_b[0])
        og.ask_intervals(big, big_sc, rec_b, "46,340 x 46,340, the small grid's legs", want=ivs_b, legs=legs_b[1])
        moved = []
        for r in sets:
            r = r.copy()
            r["ox"], r["oy"] = r["ox"] + shift, r["oy"] + shift
            moved.append(r)
        hits_b = og.ask_rays(big, big_sc, rec_b, "46,340 x 46,340, the small grid's rays", rays=moved)
        for c in pairs_s:
            assert pairs_b[c][0].tobytes() == pairs_s[c][0].tobytes() and pairs_b[c][1].tobytes() == pairs_s[c][1].tobytes(), c
        assert enc_b.tobytes() == enc_s.tobytes()
        for (_, b), (_, s) in zip(hits_b, hits_s):
            assert b.tobytes() == s.tobytes()
        og.ask_removal(big, big_sc, rec_b, "46,340 x 46,340")
