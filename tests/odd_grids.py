"""What tests/test_gpu_queries_odd_grids.py and its mesh twin share: the grids none of the between-step query tests runs
on (one-sided, one cell wide or high, two-launch scans, cell indices near 2^31, a cell size whose multiples are inexact,
an offset that dwarfs the cell) and one function per query family that asks the engine (or a mesh) and compares the
answer with the numpy restatement on `records`, its OWN read_agents(), exactly as the query tests do on their square
grids of 2 m cells.  Ids, counts, orders and the bits of every f64 are exact; the raster's velocity sums keep
field_reference.tolerance.  The families: selections, rasters, the distance queries, encounters, rays, and the timed legs
(ask_legs for cs_leg_conflicts, ask_intervals for cs_leg_intervals); ask_everything asks them all.

x runs over the grid's ny = height / cell rows, y over one row's nx = width / cell columns; the flat cell index is
row * nx + column (tests/test_gpu_large_grids.py)."""
import time

import numpy as np

import close_pairs_reference as pairs_ref
import clusters_reference as clusters_ref
import encounters_reference as encounters_ref
import field_reference as field_ref
import leg_intervals_reference as intervals_ref
import legs_reference as legs_ref
import neighbours_reference as neighbours_ref
import rays_reference as rays_ref
from rmf_crowdsim_amd import StubHighLevelPlan, _abi, scenes
from select_reference import count, pred, select, selection
from test_gpu_large_grids import BIG, LP, SCAN_TILE, WALK, _cluster, _grid, _line_crowd, tile_crowd
from test_gpu_leg_conflicts import leg_sets, speeds
from test_gpu_leg_intervals import interval_legs
from test_gpu_rays import ray_sets

INF = float("inf")
DT, STEPS = 0.1, 10
CELLS = (0.6, 1.0, 2.5)  # the distances of the distance queries, in cells (and 0)


class Scene:
    """A grid description (the keywords of LocationHash2D) and the crowd on it: `parts` = (points, preferred velocity),
    added in this order with local planner LP and an eyesight of one cell (the lattices: 0.7 m)."""

    def __init__(self, name, grid, parts, eyesight=None, at_end=("row", "column", "cells")):
        self.name, self.grid, self.parts = name, grid, parts
        self.at_end = frozenset(at_end)  # which of the grid's last row, last column and last 32 x 32 cells the crowd stands in
        self.cell = float(grid["cell_size"])
        self.eyesight = self.cell if eyesight is None else eyesight
        self.rows, self.cols = int(grid["height"] / self.cell), int(grid["width"] / self.cell)

    def populate(self, sim, shift=0.0):
        for pts, vel in self.parts:
            sim.add_agents(np.asarray(pts) + shift, StubHighLevelPlan(vel), LP, self.eyesight)
        return sim

    def cells_of(self, rec):
        """(row, column) of every record, by the division the index makes; records outside are not to be asked"""
        ox, oy = self.grid["offset"]
        return (np.floor((rec["x"] - ox) / self.cell).astype(np.int64), np.floor((rec["y"] - oy) / self.cell).astype(np.int64))

    def flat_of(self, rec):
        row, col = self.cells_of(rec)
        return row * self.cols + col


def _one_sided(name, nx, ny):
    walkers, along_x = _line_crowd(nx, ny, 2100, 11)
    fast, slow = ((WALK, 0.0), (0.8 * WALK, 0.0)) if along_x else ((0.0, WALK), (0.0, 0.8 * WALK))
    # (the last cluster stands 2 to 14 cells before the high end of the long side: in the last 32 cells, not in the last one)
    return Scene(name, _grid(nx, ny), [(walkers[0], fast), (walkers[1], slow)], at_end=("column" if along_x else "row", "cells"))


def _lattice(origin, n=2025, files=45, seed=3):
    """2,025 agents 0.5 m apart, each moved by up to 0.125 m: 22.5 m x 22.5 m from `origin`; nothing dyadic.  Everybody
    walks along y, in files; every other file is slower and drifts 1.5 cm a second towards its neighbour, so that the model
    turns it aside (walkers of one file keep their distance: crossing files meet within the model's collision distance
    and the step gives NaN).  n, files: another size, `files` files side by side along x, n / files walkers in each."""
    pts = scenes.jittered_lattice(n, 0.5, origin, 0.25, seed, columns=files)
    even = (np.arange(len(pts)) % files) % 2 == 0
    return [(pts[even], (0.0, WALK)), (pts[~even], (0.015, 0.8 * WALK))]


def scene(name):
    if name == "corridor":
        return _one_sided(name, 1, 2_000_003)
    if name == "strip":
        return _one_sided(name, 2_000_003, 1)
    if name == "tall5":
        return _one_sided(name, 5, 200_000)
    if name == "corridor2":  # (a mesh takes no tile thinner than two halo rings: its corridor is two cells wide)
        return _one_sided(name, 2, 2_000_003)
    if name == "strip2":
        return _one_sided(name, 2_000_003, 2)
    if name == "two-launch":
        n, cell, off = 4097, 4.0, np.array([-30000.0, 45000.0])
        walkers, standers = tile_crowd(n, n)
        grid = dict(width=n * cell, height=n * cell, cell_size=cell, offset=tuple(off))
        return Scene(name, grid, [(walkers[0] * cell + off, (0.0, WALK)), (walkers[1] * cell + off, (0.0, -WALK)),
                                  (standers * cell + off, (0.0, 0.0))])
    if name == "odd-cell":  # 176 columns x 111 rows; 123.4 / 0.7 = 176.29: the last 0.2 m of every row lie in no cell
        grid = dict(width=123.4, height=77.7, cell_size=0.7, offset=(-1234.5, 6789.25))
        # (the lattice stands in the middle of the grid: astride a mesh's cuts)
        s = Scene(name, grid, _lattice((-1234.5 + 27.6, 6789.25 + 50.4)), eyesight=0.7, at_end=())
        assert (s.rows, s.cols) == (111, 176)
        return s
    if name == "odd-far":  # half a cell more than 900 x 700 cells of 2.3 m: the quotient is not left to the rounding
        grid = dict(width=900.5 * 2.3, height=700.5 * 2.3, cell_size=2.3, offset=(3.0e6, -2.0e6))
        # (the lattice ends 5 m from the high corner)
        s = Scene(name, grid, _lattice((3.0e6 + 700 * 2.3 - 27.5, -2.0e6 + 900 * 2.3 - 27.5)), eyesight=0.7, at_end=("cells",))
        assert (s.rows, s.cols) == (700, 900)
        return s
    if name in ("lopsided", "diagonal"):  # 172 columns x 118 rows of 0.7 m: even 2 x 2 cuts at row 59 and column 86
        ox, oy = -1234.5, 6789.25
        grid = dict(width=121.0, height=83.0, cell_size=0.7, offset=(ox, oy))
        if name == "lopsided":
            # three lattices in an L, the corner of the L in the low quadrant: 1,800 agents over rows 8-40 and columns
            # 10-38, 900 over the same rows and columns 100-114, 400 over rows 70-84 and columns 10-24; nobody in the high
            # quadrant.  The row and the column that halve the crowd both pass through the largest lattice.
            parts = _lattice((ox + 5.6, oy + 7.0), 1800, 45, 3) + _lattice((ox + 5.6, oy + 70.0), 900, 45, 4) + \
                _lattice((ox + 49.0, oy + 7.0), 400, 20, 5)
        else:
            # two lattices of 1,000 on the diagonal: rows 8-36 and columns 10-27, rows 70-98 and columns 110-127.  Two tiles
            # of a 2 x 2 mesh hold nobody, with even cuts and with the crowd's own (right behind the first lattice)
            parts = _lattice((ox + 5.6, oy + 7.0), 1000, 40, 3) + _lattice((ox + 49.0, oy + 77.0), 1000, 40, 4)
        s = Scene(name, grid, parts, eyesight=0.7, at_end=())
        assert (s.rows, s.cols) == (118, 172)
        return s
    raise KeyError(name)


def corner_scene(n):
    """The 64 x 64 crowd of test_a_crowd_shifted_into_the_top_corner_of_a_grid_at_the_limit_steps_alike on an n x n grid
    (populate it with shift = n - 64)."""
    w = 64
    p, a, b = _cluster(30.0, 30.0, w, w, 80, 56, (0.7, 1.0), 21, margin=2.0)
    standers = np.concatenate([_cluster(0.5, 0.5, w, w, 4, 4, (0.6, 0.6), 22)[0],
                               _cluster(w - 0.5, w - 0.5, w, w, 4, 4, (0.6, 0.6), 23)[0]])
    return Scene(f"corner {n}", _grid(n, n), [(p[(a + b) % 2 == 0], (0.0, WALK)), (p[(a + b) % 2 == 1], (0.0, 0.8 * WALK)),
                                               (standers, (0.0, 0.0))])


def stepped(sc, make, shift=0.0, steps=STEPS):
    """make(grid keywords) -> an engine or a mesh; populated and stepped"""
    sim = sc.populate(make(sc.grid), shift)
    for _ in range(steps):
        sim.step(DT)
    return sim


# ---- floors: counted by the restatement alone, printed, asserted before the engine is asked --------------------------
def pair_floor(sc, rec, least, least_across_tiles=None, cache=None):
    """The pairs within one cell: at least `least`, `least_across_tiles` of them with their agents in different
    1,024-cell scan tiles.  -> the restatement's pairs"""
    want, _ = pairs_ref.pairs(rec, sc.grid, sc.cell, cache=cache)
    tile_of = dict(zip(rec["id"].tolist(), (sc.flat_of(rec) // SCAN_TILE).tolist()))
    across = sum(1 for p, q in want.tolist() if tile_of[p] != tile_of[q])
    print(f"{sc.name}: restatement alone: {len(want)} pairs within one cell, {across} across a scan-tile boundary")
    assert len(want) >= least
    assert least_across_tiles is None or across >= least_across_tiles
    return want


# ---- the query families -----------------------------------------------------------------------------------------------
def _sorted(rec):
    return rec[np.argsort(rec["id"], kind="stable")]


def _speeds(rec):
    """(the speeds of the records with finite state, the middle between the slowest and the fastest)"""
    speed = np.hypot(rec["vx"].astype(np.float64), rec["vy"].astype(np.float64))
    speed = speed[np.isfinite(speed)]
    return speed, float((speed.min() + speed.max()) / 2.0)


def role_selections(rec):
    """Two selections that need no ledger: the half of the crowd with the smaller x, and the slower walkers (or the
    standers)."""
    half = selection(_abi.CS_SEL_RECT, x0=-INF, y0=-INF, x1=float(np.nanmedian(rec["x"])), y1=INF)
    slow = selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=_speeds(rec)[1])
    return half, slow


def ask_distance_queries(sim, sc, rec, name, cells=CELLS, roles=True, cache=None):
    """cs_close_pairs, cs_agent_clusters and cs_agent_neighbours at 0 and at `cells` cells through each module's agree
    (listing, count-only and capped forms), and once with two role selections.  -> {distance in cells: (pairs, d2)}"""
    lhs = {} if cache is None else cache  # (the left-hand sides of this crowd, computed once for all its distances)
    out = {}
    for c in (0.0,) + tuple(cells):
        d = c * sc.cell
        want = pairs_ref.agree(sim, rec, sc.grid, d, name=f"{name}, pairs, {c} cells", cache=lhs)
        clusters_ref.agree(sim, rec, sc.grid, d, name=f"{name}, clusters, {c} cells", cache=lhs)
        neighbours_ref.agree(sim, rec, sc.grid, d, name=f"{name}, neighbours, {c} cells", cache=lhs, min_counts=(0, 2))
        out[c] = want
    assert len(out[0.0][0]) == 0 and len(out[1.0][0]) > 0
    if roles:
        half, slow = role_selections(rec)
        d = sc.cell
        both, _ = pairs_ref.agree(sim, rec, sc.grid, d, half, slow, name=f"{name}, pairs, two roles", cache=lhs)
        assert 0 < len(both) < len(out[1.0][0])
        neighbours_ref.agree(sim, rec, sc.grid, d, half, slow, name=f"{name}, neighbours, two roles", cache=lhs)
        clusters_ref.agree(sim, rec, sc.grid, d, half, min_size=2, name=f"{name}, clusters of one role", cache=lhs)
    return out


def ask_encounters(sim, sc, rec, name, scale=1.0, range_=None, want=None):
    """(distance, horizon, range) = (0.5 m, 3 s, 4 m) times the scale; range_: another range (a mesh sees as far as its halo)"""
    rows = encounters_ref.agree(sim, rec, sc.grid, 0.5 * scale, 3.0, 4.0 * scale if range_ is None else range_,
                                name=f"{name}, encounters", want=want)
    assert len(rows) > 0 and (rows["t"] > 0.0).any()
    return rows


def ray_queries(sc, scale=1.0, longest=INF):
    """(radius, reach) of the two ray queries, in metres"""
    return [(0.2 * scale, min(30.0 * scale, longest)), (0.4 * scale, min(INF, longest))]


def ask_rays(sim, sc, rec, name, scale=1.0, longest=INF, floors=True, want=None, rays=None):
    """ray_sets(rec, grid, reach, beams=90) at both queries: the classes by the restatement alone (printed, then
    asserted), then the engine.  -> [(rays, rows)]"""
    out = []
    for k, (radius, reach) in enumerate(ray_queries(sc, scale, longest)):
        r = ray_sets(rec, sc.grid, reach, beams=90) if rays is None else rays[k]
        stats = {}
        w = rays_ref.cast(rec, sc.grid, r, radius, stats=stats) if want is None else want[k]
        moving, still, miss = rays_ref.classes(w)
        print(f"{name}, rays {(radius, reach)}: restatement alone: {moving} hits with t > 0, {still} with t == 0, {miss} "
              f"misses, {stats.get('not_nearest')} winners that are not the candidate nearest the origin")
        if floors:
            assert moving >= 20 and still >= 20 and miss >= 20 and stats["not_nearest"] >= 5
        rays_ref.agree(sim, rec, sc.grid, r, radius, name=f"{name}, rays {(radius, reach)}", want=w)
        out.append((r, w))
    return out


def long_axis_rays(sc):
    """16 rays from 5 m outside the low end of a one-sided grid along its long axis, spread over its short side,
    t_max = +inf"""
    gx0, gx1, gy0, gy1 = pairs_ref.rectangle(sc.grid)
    k = np.arange(16) / 15.0  # (the first and the last run along the edges: nobody stands that close to them)
    if sc.rows > sc.cols:
        o, u = np.column_stack([np.full(16, gx0 - 5.0), gy0 + k * (gy1 - gy0)]), (1.0, 0.0)
    else:
        o, u = np.column_stack([gx0 + k * (gx1 - gx0), np.full(16, gy0 - 5.0)]), (0.0, 1.0)
    return rays_ref.rays_array(o, np.repeat([u], 16, axis=0))


def ask_long_axis_rays(sim, sc, rec, name, radius=0.2):
    rays = long_axis_rays(sc)
    want = rays_ref.cast(rec, sc.grid, rays, radius)
    moving, still, miss = rays_ref.classes(want)
    print(f"{name}, long-axis rays: restatement alone: {moving + still} hits, {miss} misses")
    assert moving + still >= 8 and miss >= 2
    t0 = time.perf_counter()
    rays_ref.call(sim, rays[want["id"] == rays_ref.NO_HIT], radius)
    dt = time.perf_counter() - t0
    print(f"{name}: {miss} rays the whole length of {max(sc.rows, sc.cols):,} cells and back to the host in {dt * 1e3:.1f} ms")
    rays_ref.agree(sim, rec, sc.grid, rays, radius, name=f"{name}, long-axis rays", want=want)
    return want


# ---- timed legs: cs_leg_conflicts and cs_leg_intervals ------------------------------------------------------------------
# May a leg be asked at speed_max = +inf (or distance = +inf)?  Its reach is then without bound and its wave visits every
# row of the grid one after the other: the two-million-row corridors are not walked whole.
WHOLE_WALK = {"corridor": False, "corridor2": False, "strip": True, "strip2": True, "tall5": True, "two-launch": True,
              "odd-cell": True, "odd-far": True, "lopsided": True, "diagonal": True, "corner 64": True, f"corner {BIG}": True}
# k_leg_intervals takes the columns of a row as one run of slots, k_leg_conflicts 16 columns at a time: without a reach it
# looks at 4,097 x 257 = 1.05M chunks of the two-launch grid, one after the other, and at 46,340 x 2,897 = 134M of the
# 31-bit grid, whatever the number of legs (a leg is a wave): with it the corner test took 114 s on an MI355X, 9 s
# without.  Those two grids are walked whole by cs_leg_intervals only.
WHOLE_WALK_CONFLICTS = dict(WHOLE_WALK, **{"two-launch": False, f"corner {BIG}": False})
# the random legs of leg_sets where they are not its 500: the restatement is legs x agents, and the tests of the
# two-launch grid take about a second in all
SEGMENTS = {"two-launch": 60}


def long_axis_floor(sc):
    """Must somebody stand in the way of the long-axis legs?  Not on the square grids whose crowd is a few clusters far
    apart (the legs still run there)."""
    return sc.name != "two-launch" and not sc.name.startswith("corner")


def has_standers(sc):
    """does a part of the scene's crowd prefer to stand still (the clusters in the corners of the square grids)"""
    return any(tuple(vel) == (0.0, 0.0) for _, vel in sc.parts)


def walking_pace(rec):
    """The median speed of those who walk (faster than half the fastest): where everybody walks, the median speed, which
    lies between the two walking speeds of a scene; a few dozen agents written to a standstill do not move it onto the
    slower of the two (the filter is strict: it would admit them alone)."""
    s = speeds(rec)
    return float(np.median(s[s > 0.5 * s.max()]))


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


def _with_long_axis(sc, rec, legs, extra, crowd=None):
    """legs, then `extra` (a test's own legs), then the 16 long-axis legs: they are the last 16 of every set.  crowd: the
    records the long-axis legs are laid through, where a test has written agents far from the crowd (None: rec)"""
    return np.concatenate([legs] + ([] if extra is None else [extra]) + [long_axis_legs(sc, rec if crowd is None else crowd)])


def asked_legs(sc, legs, extra=None, conflicts=False):
    """The legs of each ask of ask_legs (conflicts=True) and ask_intervals: all of them twice and, where the grid allows
    the whole walk, the first hundred, a test's own and the long-axis legs, which are asked at speed_max = +inf"""
    n = 0 if extra is None else len(extra)
    whole = (WHOLE_WALK_CONFLICTS if conflicts else WHOLE_WALK)[sc.name]
    return [legs, legs] + ([np.concatenate([legs[:100], legs[len(legs) - 16 - n:]])] if whole else [])


def conflict_leg_set(sc, rec, extra=None, crowd=None):
    return _with_long_axis(sc, rec, leg_sets(rec, sc.grid, segments=SEGMENTS.get(sc.name, 500)), extra, crowd)


def interval_leg_set(sc, rec, extra=None, crowd=None):
    return _with_long_axis(sc, rec, interval_legs(rec, sc.grid, segments=SEGMENTS.get(sc.name, 500)), extra, crowd)


def ask_legs(sim, sc, rec, name, want=None, legs=None, extra=None, crowd=None):
    """The leg sets and the long-axis legs at distances of 0.4 and 0.8 cells, the second with the speed filter between
    the two walking speeds of the scene; where the grid allows, the first hundred legs at speed_max = +inf (the whole
    walk).  The classes by the restatement alone (printed, then asserted), then the engine.  -> the restatement's rows.
    legs: the whole set where it is not made here (its last 16 the long-axis legs); extra: legs of the test's own, asked
    with the others; crowd: the records the long-axis legs are laid through (None: rec)."""
    pace = walking_pace(rec)
    if legs is None:
        legs = conflict_leg_set(sc, rec, extra, crowd)
    asks = list(zip(asked_legs(sc, legs, extra, conflicts=True), (0.4 * sc.cell, 0.8 * sc.cell, 0.4 * sc.cell), (2.0, pace, INF)))
    out = []
    for k, (l, distance, speed_max) in enumerate(asks):
        w = legs_ref.conflicts(rec, sc.grid, l, distance, speed_max) if want is None else want[k]
        moving, still, miss = legs_ref.classes(w)
        along = int((w["id"][-16:] != legs_ref.NO_HIT).sum())
        print(f"{name}, legs {(distance, speed_max)}: restatement alone: {still} conflicts at s == 0, {moving} at s > 0, "
              f"{miss} misses; {along} of the 16 long-axis legs conflict")
        if k == 1 and has_standers(sc):
            # (walkers of one speed and standers: the median speed admits the standers alone, and few legs pass them.
            # The first query carries the classes; this one is compared all the same)
            assert miss >= 5
        else:
            assert (still >= 5 and moving >= 5 and miss >= 5) if k < 2 else (still + moving >= 5 and miss >= 1)
        legs_ref.agree(sim, rec, sc.grid, l, distance, speed_max, name=f"{name}, legs {(distance, speed_max)}", want=w)
        out.append(w)
    if long_axis_floor(sc):
        assert (out[0]["id"][-16:] != legs_ref.NO_HIT).sum() >= 2  # (somebody stands in the way of the long-axis legs)
    return out


def interval_queries(sc, rec):
    """(distance, speed_max) of the interval queries: everybody slower than 2 m/s within 0.4 cell, the speed filter
    between the slowest and the fastest within 0.8 cell, and (where the grid allows the whole walk) everybody"""
    return [(0.4 * sc.cell, 2.0), (0.8 * sc.cell, _speeds(rec)[1]), (0.4 * sc.cell, INF)]


def intervals_alone(sc, rec, name, legs, extra=None):
    """The restatement ALONE on the asks of ask_intervals: the classes of every ask printed, then the floors asserted.
    The first query carries them all; the second is there for its filter (where somebody stands still it admits the
    standers alone, who enter few legs later than at once), the third for the walk without a reach.
    -> [(legs, distance, speed_max)], [(rows, counts)]"""
    asks = [(l, d, v) for l, (d, v) in zip(asked_legs(sc, legs, extra), interval_queries(sc, rec))]
    out = []
    for k, (l, distance, speed_max) in enumerate(asks):
        stats = {}
        rows, counts = intervals_ref.intervals(rec, sc.grid, l, distance, speed_max, stats=stats)
        along = int((counts[-16:] > 0).sum())
        print(f"{name}, intervals {(distance, speed_max)}: restatement alone: {len(rows)} rows, {stats}; {along} of the 16 "
              f"long-axis legs have rows")
        if k == 0:
            assert min(stats["at_start"], stats["later"], stats["leaves"], stats["stays"], stats["same_velocity"]) >= 15, stats
            assert stats["crowded_legs"] >= 10 and stats["free_legs"] >= 5, stats
            assert along >= 2 or not long_axis_floor(sc)
        elif k == 1:
            assert len(rows) > 0 and stats["at_start"] >= 15, stats
        else:
            assert len(rows) > 0
        out.append((rows, counts))
    return asks, out


def ask_intervals(sim, sc, rec, name, want=None, legs=None, extra=None, crowd=None):
    """interval_legs and the long-axis legs, from `rec`, at interval_queries and, where the grid allows, the first hundred
    legs at speed_max = +inf (the whole walk): the classes by the restatement alone (intervals_alone), then the engine:
    ids, per-leg counts and the bits of s_in and s_out through leg_intervals_reference.agree.  -> the restatement's
    [(rows, counts)].  want: that list, where a test has it already (a mesh after the engine: the floors were asserted
    then); legs, extra, crowd: as for ask_legs."""
    if legs is None:
        legs = interval_leg_set(sc, rec, extra, crowd)
    if want is None:
        asks, want = intervals_alone(sc, rec, name, legs, extra)
    else:
        asks = [(l, d, v) for l, (d, v) in zip(asked_legs(sc, legs, extra), interval_queries(sc, rec))]
    for (l, distance, speed_max), w in zip(asks, want):
        intervals_ref.agree(sim, rec, sc.grid, l, distance, speed_max, name=f"{name}, intervals {(distance, speed_max)}",
                            want=w)
    return want


def region_selections(sc, rec):
    """The cells of the last row, of the last column, the quadrant from the median agent to the high corner, a circle
    round the agent in the first occupied cell, the faster walkers by a speed term."""
    gx0, gx1, gy0, gy1 = pairs_ref.rectangle(sc.grid)
    cell = sc.cell
    first = rec[np.argmin(sc.flat_of(rec) + np.where(pairs_ref.takes_part(rec, sc.grid), 0, 2 ** 62))]
    return [("the last row", selection(_abi.CS_SEL_RECT, x0=float(gx1 - cell), y0=float(gy0), x1=float(gx1), y1=float(gy1))),
            ("the last column", selection(_abi.CS_SEL_RECT, x0=float(gx0), y0=float(gy1 - cell), x1=float(gx1), y1=float(gy1))),
            ("the high quadrant", selection(_abi.CS_SEL_RECT, x0=float(np.nanmedian(rec["x"])), y0=float(np.nanmedian(rec["y"])),
                                            x1=float(gx1), y1=float(gy1))),
            ("round the first agent", selection(_abi.CS_SEL_CIRCLE, cx=float(first["x"]), cy=float(first["y"]), r=1.5 * cell)),
            ("a speed", selection(_abi.CS_SEL_SPEED, speed_lo=_speeds(rec)[1], speed_hi=INF))]


def ask_selections(sim, sc, rec, name, at_end=None):
    """cs_select_agents (all ids, and under a cap) and cs_count_agents against select_reference.pred -> {name: ids}.
    at_end: which of ("row", "column") must select somebody (None: where the scene's stepped crowd stands, sc.at_end; a
    test that has written agents into the last cell or onto the edges passes both)."""
    at_end = sc.at_end if at_end is None else frozenset(at_end)
    sels = region_selections(sc, rec)
    out = {}
    for what, sel in sels:
        want = rec["id"][pred(sel, rec, None, None, None)]
        n, got = select(sim, sel)
        print(f"{name}, select {what}: restatement {len(want)}, engine {n}")
        assert n == len(want) and got.tolist() == want.tolist(), (name, what)
        if len(want) > 3:
            n, few = select(sim, sel, cap=len(want) // 2)
            assert n == len(want) and few.tolist() == want[:len(want) // 2].tolist(), (name, what)
        out[what] = want
    rc, counts = count(sim, [s for _, s in sels])
    assert rc == 0 and counts.tolist() == [len(out[what]) for what, _ in sels], name
    assert len(out["the high quadrant"]) > 0 and len(out["round the first agent"]) > 0 and 0 < len(out["a speed"]) < len(rec)
    for end in ("row", "column"):
        if end in at_end:
            assert len(out[f"the last {end}"]) > 0, (name, end)
        else:
            print(f"{name}: nobody is asked for in the last {end}: this crowd does not stand there")
    return out


def ask_removal(twin, sc, rec, name):
    """remove_selected by the high quadrant on a twin: what is left is what the restatement leaves"""
    what, sel = region_selections(sc, rec)[2]
    gone = pred(sel, rec, None, None, None)
    assert twin.read_agents().tobytes() == rec.tobytes(), name
    ids = twin.remove_selected(rect=(sel.x0, sel.y0, sel.x1, sel.y1))
    print(f"{name}, remove {what}: restatement {int(gone.sum())} of {len(rec)}, engine {len(ids)}")
    assert 0 < gone.sum() < len(rec) and ids.tolist() == rec["id"][gone].tolist(), name
    assert twin.read_agents().tobytes() == rec[~gone].tobytes(), name


def ask_by_id(sim, rec, ids, name):
    """read_agents_by_id gives the rows of read_agents(), in the order asked"""
    at = {int(i): j for j, i in enumerate(rec["id"])}
    assert sim.read_agents_by_id(ids).tobytes() == rec[[at[int(i)] for i in ids]].tobytes(), name


class released:
    """with released(engine, mesh, ...): every one gives its device memory back on the way out, also out of a failing
    test (tiles of 2M cells and the 43 GB engine run in the same session as everything after them)."""

    def __init__(self, *sims):
        self.sims = sims

    def __enter__(self):
        return self.sims

    def __exit__(self, *exc):
        for s in self.sims:
            s.close() if hasattr(s, "close") else s.__del__()
        return False


def rasters(sc, rec):
    """(name, desc): the grid's last 32 x 32 cells (or its whole width), cell by cell; 16 x 16 and 130 x 130 bins of 1.3
    cells from an origin 0.37 cell off the cell corners, over the cluster round the median agent.  The last is above
    field_lds_limit() even without sums (67,600 B of counts)."""
    ox, oy = sc.grid["offset"]
    cell = sc.cell
    nr, nc = min(32, sc.rows), min(32, sc.cols)
    part = _sorted(rec[pairs_ref.takes_part(rec, sc.grid)])
    row, col = sc.cells_of(part[len(part) // 2:len(part) // 2 + 1])
    out = [("the last cells", field_ref.desc(ox + (sc.rows - nr) * cell, oy + (sc.cols - nc) * cell, cell, cell, nr, nc))]
    for n in (16, 130):
        out.append((f"{n} x {n} bins of 1.3 cells", field_ref.desc(
            ox + (int(row[0]) + 0.37) * cell - 0.65 * n * cell, oy + (int(col[0]) + 0.37) * cell - 0.65 * n * cell,
            1.3 * cell, 1.3 * cell, n, n)))
    return out


def ask_fields(sim, sc, rec, name, monkeypatch, at_end=None):
    """Every raster as counts alone and with sums, in the form cs_agent_field picks and (CS_FIELD_LDS_BYTES=0) in the
    global form.  at_end: with "cells" in it the raster of the last cells must hold somebody (None: sc.at_end)."""
    at_end = sc.at_end if at_end is None else frozenset(at_end)
    for what, d in rasters(sc, rec):
        want = field_ref.raster(d, rec)
        print(f"{name}, raster {what}: {int(want[0].sum())} agents in {int((want[0] > 0).sum())} of {want[0].size} bins")
        assert want[0].sum() > 0 or (what == "the last cells" and "cells" not in at_end), (name, what)
        for limit in (None, "0"):
            if limit is None:
                monkeypatch.delenv("CS_FIELD_LDS_BYTES", raising=False)
            else:
                monkeypatch.setenv("CS_FIELD_LDS_BYTES", limit)
            for form in ("count", "both"):
                rc, cnt, sums = field_ref.field(sim, d, None, want=form)
                assert rc == 0, (name, what, field_ref.last_error(sim))
                field_ref.check(f"{name}, {what}, {form}, LDS limit {limit}", cnt, sums, want)
    monkeypatch.delenv("CS_FIELD_LDS_BYTES", raising=False)


def ask_everything(sim, sc, rec, name, monkeypatch, scale=1.0, longest=INF, ray_floors=True, at_end=None, legs=True,
                   extra_legs=None, legs_crowd=None):
    """legs=False: the test asks the two leg calls itself, with legs of its own; extra_legs, legs_crowd: the extra and
    crowd of ask_legs and ask_intervals"""
    ask_selections(sim, sc, rec, name, at_end)
    ask_fields(sim, sc, rec, name, monkeypatch, at_end)
    pairs = ask_distance_queries(sim, sc, rec, name)
    rows = ask_encounters(sim, sc, rec, name, scale)
    ask_rays(sim, sc, rec, name, scale, longest, floors=ray_floors)
    if legs:
        ask_legs(sim, sc, rec, name, extra=extra_legs, crowd=legs_crowd)
        ask_intervals(sim, sc, rec, name, extra=extra_legs, crowd=legs_crowd)
    assert sim.read_agents().tobytes() == rec.tobytes(), name  # (asking changes nothing)
    return pairs, rows


# ---- writes between steps ---------------------------------------------------------------------------------------------
def boundary_tile(sc):
    """k with the cells k * 1,024 - 1 and k * 1,024 in one row (where a row has more than one cell), a third of the way up
    the grid"""
    k = max(1, (sc.rows * sc.cols // SCAN_TILE) // 3)
    while SCAN_TILE % sc.cols and (k * SCAN_TILE) % sc.cols == 0:  # (1 or 2 columns: the two cells are two rows)
        k += 1
    return k


def move_into_cells(sc, rec, seed=5):
    """Records of 48 agents with new positions: 16 in the grid's last cell, 16 in cell 0, 8 either side of the scan-tile
    boundary boundary_tile() * 1,024.  In a cell they stand on a 4 x 4 (or 4 x 2) lattice 0.22 cell apart, 0.15 cell from
    its low corner, so that no two are closer than the model's collision distance where the cell is 1 m."""
    k = boundary_tile(sc)
    part = _sorted(rec[pairs_ref.takes_part(rec, sc.grid)])
    w = part[np.linspace(0, len(part) - 1, 48).astype(np.int64)].copy()
    assert len(np.unique(w["id"])) == 48
    ox, oy = sc.grid["offset"]
    flats = [sc.rows * sc.cols - 1] * 16 + [0] * 16 + [k * SCAN_TILE - 1] * 8 + [k * SCAN_TILE] * 8
    rng = np.random.default_rng(seed)
    for j, flat in enumerate(flats):
        row, col = divmod(flat, sc.cols)
        slot = j % 16 if j < 32 else j % 8
        fx = 0.15 + 0.22 * (slot % 4) + rng.uniform(0.0, 0.01)
        fy = 0.15 + 0.22 * (slot // 4) + rng.uniform(0.0, 0.01)
        w["x"][j] = ox + (row + fx) * sc.cell
        w["y"][j] = oy + (col + fy) * sc.cell
    w["vx"], w["vy"] = 0.0, 0.0  # (written with the position: nobody closes in on a neighbour 0.22 m away in the next step)
    return w, k


def check_moved(sim, sc, w, k, name):
    """After write_agents(w): the agents are where they were written, by id and in read_agents(); the last cell and cell 0
    hold at least 16 each; at least 10 pairs within one cell involve a moved agent (all by the restatement alone).
    -> the records"""
    rec = sim.read_agents()
    back = sim.read_agents_by_id(w["id"])
    at = {int(i): j for j, i in enumerate(rec["id"])}
    assert back.tobytes() == rec[[at[int(i)] for i in w["id"]]].tobytes(), name
    flat = sc.flat_of(rec)
    held = [int((flat == f).sum()) for f in (sc.rows * sc.cols - 1, 0, k * SCAN_TILE - 1, k * SCAN_TILE)]
    want, _ = pairs_ref.pairs(rec, sc.grid, sc.cell)
    moved = int(np.isin(want, w["id"].astype(np.uint64)).any(axis=1).sum())
    print(f"{name}: the last cell, cell 0 and the cells either side of tile boundary {k} hold {held}; {moved} of "
          f"{len(want)} pairs within one cell involve a moved agent")
    assert held[0] >= 16 and held[1] >= 16 and held[2] >= 8 and held[3] >= 8 and moved >= 10
    assert np.array_equal(sc.flat_of(back), sc.flat_of(w)), name  # (each stands in the cell it was written into)
    return rec


def edge_agents(sc, rec, outsiders):
    """Records of eight agents with new positions just inside every edge and corner of the participants' rectangle
    (the low edges themselves, nextafter(high edge, -inf), the middle), of eight partners a third of a cell further in,
    so that every edge agent is in a pair, and of `outsiders` more outside the rectangle that the index
    still takes: one 0.3 cell below the low x edge (clamped into row 0), one 0.1 m beyond the last column where the grid's
    width holds a partial cell (aliased into the next row; a mesh refuses that one).  -> (records, ids of the eight)"""
    gx0, gx1, gy0, gy1 = pairs_ref.rectangle(sc.grid)
    xs = (gx0, (gx0 + gx1) / 2.0 + 0.123, np.nextafter(gx1, -INF))
    ys = (gy0, (gy0 + gy1) / 2.0 + 0.321, np.nextafter(gy1, -INF))
    spots = [(x, y) for i, x in enumerate(xs) for j, y in enumerate(ys) if (i, j) != (1, 1)]
    inward = (0.3 * sc.cell, 0.2 * sc.cell, -0.3 * sc.cell)  # a partner for each, 0.3 to 0.43 cell further in
    spots += [(x + inward[i], y + inward[j]) for i, x in enumerate(xs) for j, y in enumerate(ys) if (i, j) != (1, 1)]
    spots += [(gx0 - 0.3 * sc.cell, ys[1]), (xs[1], gy1 + 0.1)][:outsiders]
    part = _sorted(rec[pairs_ref.takes_part(rec, sc.grid)])
    w = part[np.linspace(5, len(part) - 6, len(spots)).astype(np.int64)].copy()
    w["x"], w["y"] = [p[0] for p in spots], [p[1] for p in spots]
    return w, w["id"][:8].copy()


def check_edges(sc, rec, w, ids, outsiders):
    """By the restatement alone: the edge agents and their partners are where they were written, to the f32 offset that
    holds them; at least four of the eight take part (one whose offset rounds up to the cell size is reported ON the high
    edge, outside) and are in a pair within one cell; the outsiders are held and take no part; the f64 rebuild matters."""
    at = {int(i): j for j, i in enumerate(rec["id"])}
    rows = rec[[at[int(i)] for i in w["id"]]]  # (a cell and an f32 offset hold them: not the written bits)
    # an f32 offset of at most one cell: 2^-24 of it, and the rounding of the f64 sum; an outsider's offset is measured from
    # the cell it is clamped or aliased into and may be as long as the grid
    tol = np.where(np.arange(len(w)) < 16, 1e-6 * sc.cell, 2.0 ** -23 * max(sc.grid["width"], sc.grid["height"]))
    assert (np.abs(rows["x"] - w["x"]) <= tol).all() and (np.abs(rows["y"] - w["y"]) <= tol).all()
    part = pairs_ref.takes_part(rows, sc.grid)
    want, _ = pairs_ref.pairs(rec, sc.grid, sc.cell)
    paired = int(np.isin(ids.astype(np.uint64), want).sum())
    print(f"{sc.name}: {int(part[:8].sum())} of the 8 edge agents take part, {paired} of them in a pair within one cell; "
          f"{int(part[16:].sum())} of {outsiders} outsiders take part")
    assert part[:8].sum() >= 4 and paired >= 4 and part[8:16].all() and not part[16:].any() and len(part) == 16 + outsiders
    ox, oy = sc.grid["offset"]
    took = rec[pairs_ref.takes_part(rec, sc.grid)]
    through_f32 = sum(int((took[c] != o + (took[c] - o).astype(np.float32).astype(np.float64)).sum())
                      for c, o in (("x", ox), ("y", oy)))
    print(f"{sc.name}: {through_f32} coordinates of participants differ from offset + (float32)(coordinate - offset)")
    assert through_f32 >= 1


def edge_legs(sc, rec, w):
    """Legs made for the agents edge_agents wrote, from where `rec` holds them: for each of the eight edge agents and
    each outsider a wait of 1.5 s 0.1 cell beside it, on the side away from the grid's middle (outside the rectangle for
    an agent on a low edge), then for each a leg of 3 s that starts 3 cells outside the grid from it and is where the
    agent will be after 2 s.  Nobody is ignored.  -> (legs, the number of waits)"""
    at = {int(i): j for j, i in enumerate(rec["id"])}
    who = rec[[at[int(i)] for i in np.concatenate([w["id"][:8], w["id"][16:]])]]
    gx0, gx1, gy0, gy1 = pairs_ref.rectangle(sc.grid)

    def away(p, lo, hi):  # -1 by the low edge (or below it), +1 by the high edge, 0 in the middle
        return np.where(p < lo + 0.25 * (hi - lo), -1.0, np.where(p > hi - 0.25 * (hi - lo), 1.0, 0.0))

    out = np.column_stack([away(who["x"], gx0, gx1), away(who["y"], gy0, gy1)])
    assert (np.abs(out).sum(axis=1) >= 1).all()
    p = np.column_stack([who["x"], who["y"]])
    v = np.column_stack([who["vx"].astype(np.float32).astype(np.float64), who["vy"].astype(np.float32).astype(np.float64)])
    waits = legs_ref.legs_array(p + 0.1 * sc.cell * out, (0.0, 0.0), 0.0, 1.5)
    start = p + 3.0 * sc.cell * out
    inward = legs_ref.legs_array(start, ((p + 2.0 * v) - start) / 2.0, 0.0, 3.0)
    return np.concatenate([waits, inward]), len(waits)


def check_edge_legs(sc, rec, w, ids, legs):
    """By the restatement alone, at the first interval query: at least four of the eight edge agents are rows of the edge
    legs, the outsiders are rows of no leg.  -> (rows, counts)"""
    distance, speed_max = interval_queries(sc, rec)[0]
    rows, counts = intervals_ref.intervals(rec, sc.grid, legs, distance, speed_max)
    listed = int(np.isin(ids.astype(np.uint64), rows["id"]).sum())
    print(f"{sc.name}: restatement alone: {len(rows)} rows of the {len(legs)} edge legs; {listed} of the 8 edge agents are "
          f"rows, {int(np.isin(rows['id'], w['id'][16:].astype(np.uint64)).sum())} rows are outsiders")
    assert listed >= 4 and not np.isin(rows["id"], w["id"][16:].astype(np.uint64)).any()
    return rows, counts


def ask_legs_wider_than_the_grid(sim, sc, rec, w, waits, name):
    """Both leg calls on the waits of edge_legs, each ignoring the agent it stands beside, at speed_max = +inf and a
    distance of twice the grid's width and of +inf: every participant but the ignored one is a row of every leg, from 0 to
    T; the first of them by id is the conflict."""
    part = pairs_ref.takes_part(rec, sc.grid)
    waits = waits.copy()
    waits["ignore"] = np.concatenate([w["id"][:8], w["id"][16:]]).astype(np.uint64)
    less = np.isin(waits["ignore"], rec["id"][part].astype(np.uint64)).astype(np.uint64)
    for distance in (2.0 * sc.grid["width"], INF):
        rows, counts = intervals_ref.agree(sim, rec, sc.grid, waits, distance, INF,
                                           name=f"{name}, intervals wider than the grid: {distance}")
        assert 0 < less.sum() < len(waits) and (counts == np.uint64(part.sum()) - less).all()
        assert (rows["s_in"] == 0.0).all() and (rows["s_out"] == 1.5).all()
        hits = legs_ref.agree(sim, rec, sc.grid, waits, distance, INF, name=f"{name}, legs wider than the grid: {distance}")
        assert (hits["id"] != legs_ref.NO_HIT).all() and (hits["s"] == 0.0).all()


def ask_python_surface_of_the_legs(sim, sc, rec, name, crowd, distance=0.3):
    """Simulation.free_intervals on 50 spots 0.3 m beside agents of `crowd` (records of `rec`: the lattice, without the
    agents written onto the edges) against the complement of the restatement's rows, and Simulation.path_conflict on one
    path through the crowd against the first conflict of its legs by the restatement."""
    from rmf_crowdsim_amd.simulation import free_spans, merge_leg_intervals, paths_legs
    speed_max = 2.0
    part = _sorted(crowd[pairs_ref.takes_part(crowd, sc.grid)])
    who = part[np.linspace(0, len(part) - 1, 50).astype(np.int64)]
    spots = np.column_stack([who["x"] + 0.3, who["y"]])
    waits = legs_ref.legs_array(spots, (0.0, 0.0), 0.5, 4.0)
    rows, _ = intervals_ref.intervals(rec, sc.grid, waits, distance, speed_max)
    want = free_spans(*merge_leg_intervals(rows, len(waits)), waits["t0"], waits["t1"])
    kinds = [len(f) for f in want]
    print(f"{name}, free_intervals: restatement alone: {len(rows)} rows; {kinds.count(0)} of 50 spots never free, "
          f"{sum(f == [(0.5, 4.0)] for f in want)} always")
    assert len(rows) >= 50 and sum(0 < len(f) and f != [(0.5, 4.0)] for f in want) >= 10  # (free for a part of the time)
    assert sim.free_intervals(spots, 0.5, 4.0, distance, speed_max) == want, name
    lo, hi = np.array([part["x"].min(), part["y"].min()]), np.array([part["x"].max(), part["y"].max()])
    mid = lo + np.array([0.31, 0.43]) * (hi - lo)
    path = (np.array([lo - 3.0, mid, mid, hi + 3.0]), np.array([0.0, 4.0, 5.0, 12.0]))  # (the second leg is a wait)
    legs, _ = paths_legs([path])
    hits = legs_ref.conflicts(rec, sc.grid, legs, distance, speed_max)
    first = np.nonzero(hits["id"] != legs_ref.NO_HIT)[0]
    print(f"{name}, path_conflict: restatement alone: legs {first.tolist()} of {len(legs)} conflict")
    assert len(legs) == 3 and len(first) >= 1
    k = int(first[0])
    l, s = legs[k], float(hits["s"][k])
    want = (int(hits["id"][k]), float(l["t0"]) + s, k, (float(l["x0"]) + float(l["vx"]) * s, float(l["y0"]) + float(l["vy"]) * s))
    assert sim.path_conflict(*path, distance, speed_max) == want, name


# ---- meshes -----------------------------------------------------------------------------------------------------------
def cuts_of(rects):
    """(rows, columns) at which a tile of a mesh begins, other than 0, from its tile_rects()"""
    r = np.asarray(rects, dtype=np.int64)
    return sorted(set(r[:, 0].tolist()) - {0}), sorted(set(r[:, 2].tolist()) - {0})


def astride_cuts(sc, rec, rects, apart=False):
    """Records of four agents with new positions astride every cut: 0.3 and 0.1 cell either side of it, in the middle of
    the grid's other axis.  apart: for a crowd that is stepped afterwards: a quarter of a cell either side, two and two
    0.6 cell apart along the cut, 3 cells from the middle of the other axis (the agents astride a row cut and a column cut
    that cross in the middle of the grid do not meet); no two are closer than 0.5 cell, 0.35 m where a cell is 0.7 m, and
    the walking speeds of a scene differ by 0.08 m/s: they stay outside the model's collision distance of 0.2 m for 15
    steps.  (They keep their velocities: a few standers would be all that the speed filters of the scenes admit.)"""
    cut_rows, cut_cols = cuts_of(rects)
    ox, oy = sc.grid["offset"]
    spots = []
    places = [(-0.25, 3.0), (0.25, 3.0), (-0.25, 3.6), (0.25, 3.6)] if apart else \
        [(f, 0.05 * j) for j, f in enumerate((-0.3, -0.1, 0.1, 0.3))]
    for f, along in places:
        spots += [(ox + (c + f) * sc.cell, oy + (sc.cols // 2 + 0.4 + along) * sc.cell) for c in cut_rows]
        spots += [(ox + (sc.rows // 2 + 0.4 + along) * sc.cell, oy + (c + f) * sc.cell) for c in cut_cols]
    part = _sorted(rec[pairs_ref.takes_part(rec, sc.grid)])
    w = part[np.linspace(3, len(part) - 4, len(spots)).astype(np.int64)].copy()
    w["x"], w["y"] = [p[0] for p in spots], [p[1] for p in spots]
    return w


def cut_floor(sc, rec, rects, distance):
    """By the restatement alone: pairs within `distance` whose agents stand on either side of a cut, every cut"""
    want, _ = pairs_ref.pairs(rec, sc.grid, distance)
    row, col = sc.cells_of(rec)
    at = {int(i): j for j, i in enumerate(rec["id"])}
    p, q = [at[v] for v in want[:, 0].tolist()], [at[v] for v in want[:, 1].tolist()]
    cut_rows, cut_cols = cuts_of(rects)
    across = [int(((row[p] < c) != (row[q] < c)).sum()) for c in cut_rows] + \
             [int(((col[p] < c) != (col[q] < c)).sum()) for c in cut_cols]
    print(f"{sc.name}: cuts at rows {cut_rows} and columns {cut_cols}: of {len(want)} pairs within {distance} m, "
          f"{across} across them")
    assert len(across) > 0 and all(n > 0 for n in across)


# ---- cuts placed at will, cuts of the crowd, and the floors of the scenes made for them ---------------------------------
def placed_cut_weights(sc, shape, rows=(), cols=(), halo=1):
    """Weight points (for NativeTileMesh(weights=) / TileLayout(weights=)) that put the interior edges of a
    shape[0] x shape[1] mesh at the rows `rows` and the columns `cols`.  _weighted_edges / mesh_weighted_edges put edge k
    at the first index whose cumulative weight reaches k parts of the total: all the weight of part k in the single row
    r puts that edge at r + 1, so part k stands in row rows[k] - 1 (the last part in the last row).  A point weighs on
    both axes, hence one point for every pair (part along x, part along y); the sums are whole numbers, exact in f64.
    The edges asked for lie at least two halo rings apart (closer ones are pushed apart, and these would not be met)."""
    assert len(rows) == shape[0] - 1 and len(cols) == shape[1] - 1
    for edges, n in ((list(rows), sc.rows), (list(cols), sc.cols)):
        e = [0] + edges + [n]
        assert all(b - a >= 2 * halo for a, b in zip(e, e[1:])), (e, halo)
    ox, oy = sc.grid["offset"]
    in_rows, in_cols = [r - 1 for r in rows] + [sc.rows - 1], [c - 1 for c in cols] + [sc.cols - 1]
    return np.array([(ox + (r + 0.5) * sc.cell, oy + (c + 0.5) * sc.cell) for r in in_rows for c in in_cols])


def rects_of(edges_x, edges_y):
    """tile_rects() of an in-process mesh with these edges: (x0, x1, y0, y1) per tile, tile tx * tiles_y + ty"""
    return np.array([(edges_x[i], edges_x[i + 1], edges_y[j], edges_y[j + 1])
                     for i in range(len(edges_x) - 1) for j in range(len(edges_y) - 1)], dtype=np.uint32)


def layout(sc, shape, halo=1, points=None, rec=None):
    """tiles.TileLayout of the scene's grid, on the CPU: even cuts, the cuts of weights= `points`, or (rec) the cuts
    cs_mesh_recut makes: the quantiles of numpy histograms of the records' rows and columns (cells_of; agents inside
    the grid), no tile thinner than two halo rings."""
    from rmf_crowdsim_amd import LocationHash2D
    from rmf_crowdsim_amd.tiles import TileLayout
    index = LocationHash2D(**sc.grid)
    if rec is not None:
        row, col = sc.cells_of(rec)
        assert (row >= 0).all() and (row < sc.rows).all() and (col >= 0).all() and (col < sc.cols).all()
        hist = (np.bincount(row, minlength=sc.rows), np.bincount(col, minlength=sc.cols))
        return TileLayout(index, shape[0], shape[1], min_cells=2 * halo, histograms=hist)
    return TileLayout(index, shape[0], shape[1], weights=points, min_cells=2 * halo)


def owners(rects, sc, rec):
    """the tile (an index into rects) that owns every record"""
    row, col = sc.cells_of(rec)
    r = np.asarray(rects, dtype=np.int64)
    inside = (row[:, None] >= r[:, 0]) & (row[:, None] < r[:, 1]) & (col[:, None] >= r[:, 2]) & (col[:, None] < r[:, 3])
    assert (inside.sum(axis=1) == 1).all()
    return inside.argmax(axis=1)


def recut_floors(sc, rec, shape=(2, 2), halo=1, empty_before=1, empty_after=0, least=100, moved=8):
    """The floors of a scene made for a re-cut, by TileLayout and numpy alone (no GPU): with even cuts `empty_before` tiles
    hold nobody; after the cuts of the crowd `empty_after` do and every other tile holds at least `least` agents; every
    interior edge moves by at least `moved` cells; no tile is square, before or after.  rec: records, or points (n x 2).
    -> (rects with even cuts, rects after the re-cut, agents per tile after it)"""
    if rec.dtype.names is None:
        pts, rec = rec, np.zeros(len(rec), dtype=[("x", "f8"), ("y", "f8")])
        rec["x"], rec["y"] = pts[:, 0], pts[:, 1]
    even, cut = layout(sc, shape, halo), layout(sc, shape, halo, rec=rec)
    before, after = rects_of(even.x_edges, even.y_edges), rects_of(cut.x_edges, cut.y_edges)
    n_before = np.bincount(owners(before, sc, rec), minlength=len(before))
    n_after = np.bincount(owners(after, sc, rec), minlength=len(after))
    shifts = [abs(a - b) for a, b in zip(even.x_edges[1:-1] + even.y_edges[1:-1], cut.x_edges[1:-1] + cut.y_edges[1:-1])]
    print(f"{sc.name}: even cuts {even.x_edges} x {even.y_edges} hold {n_before.tolist()}, the crowd's cuts {cut.x_edges} x "
          f"{cut.y_edges} hold {n_after.tolist()}; the edges move by {shifts} cells")
    assert int((n_before == 0).sum()) == empty_before and int((n_after == 0).sum()) == empty_after
    assert (n_after[n_after > 0] >= least).all() and n_after.sum() == len(rec)
    assert len(shifts) > 0 and min(shifts) >= moved
    for r in np.concatenate([before, after]).astype(np.int64):
        assert r[1] - r[0] != r[3] - r[2], r
    return before, after, n_after


def thin_tile_floors(sc, rec, rects, k, halo):
    """Tile k of `rects` is exactly two halo rings thick between two neighbours: it owns at least 30 agents, pairs within
    halo * cell exist across BOTH its cuts (cut_floor), and at least one of its agents stands in a cell that the band test
    of the distance queries at that distance (reach = halo + 1 cells from an edge) puts into the bands of both neighbours.
    (No agent can be in a PAIR across both cuts: its partners would be 2 * halo cells apart and each closer than halo.)"""
    r = np.asarray(rects, dtype=np.int64)[k]
    axis = 0 if r[1] - r[0] == 2 * halo else 1
    lo, hi = int(r[2 * axis]), int(r[2 * axis + 1])
    assert hi - lo == 2 * halo and lo > 0 and hi < (sc.rows, sc.cols)[axis]
    own = owners(rects, sc, rec) == k
    at = sc.cells_of(rec)[axis][own]
    both = int(((at < lo + halo + 1) & (at + halo + 1 >= hi)).sum())
    print(f"{sc.name}: the thin tile {r.tolist()} owns {int(own.sum())} agents, {both} of them in the bands of both neighbours")
    assert own.sum() >= 30 and both >= 1
    cut_floor(sc, rec, rects, halo * sc.cell)


# ---- one body for "mesh == engine == restatement" -------------------------------------------------------------------------
FAMILIES = ("select", "field", "near", "encounters", "rays", "legs", "intervals")


def ask_mesh_as_engine(mesh, single, sc, rec, what, halo, scale, monkeypatch, longest=INF, cells=None, by_id=None,
                       removal=True, families=FAMILIES, roles=True):
    """Every between-step call on a mesh and on its single-engine twin, which hold the records `rec`: each answer is the
    restatement's on `rec`, which runs once (whoever is asked second is asked with want=).  Selections, rasters and the
    distance queries at `cells` (None: those of CELLS up to the halo, where a mesh sees across a cut), encounters at a
    range of halo * cell, the rays, both leg calls; nothing asked has changed a record; then the agents `by_id` are read
    by id, and (removal) the agents of the high quadrant leave both.  families: a subset, where a test asks less.  One
    of mesh and single may be None (the ranks of a distributed mesh and their parent hold one each)."""
    twins = [(t, who) for t, who in ((single, "engine"), (mesh, "mesh")) if t is not None]
    for t, _ in twins:
        assert rec.tobytes() == t.read_agents().tobytes(), what
    limit = halo * sc.cell
    cells = [c for c in CELLS if c <= halo] if cells is None else list(cells)
    assert 1.0 in cells  # (one distance IS the limit where the halo is one cell)
    lhs = {}
    for t, who in twins:
        if "select" in families:
            ask_selections(t, sc, rec, f"{what} ({who})")
        if "field" in families:
            ask_fields(t, sc, rec, f"{what} ({who})", monkeypatch)
        if "near" in families:
            ask_distance_queries(t, sc, rec, f"{what} ({who})", cells=cells, roles=roles, cache=lhs)
    rows = cast = hits = spans = None
    for t, who in twins:
        if "encounters" in families:
            rows = ask_encounters(t, sc, rec, f"{what} ({who})", scale, range_=limit, want=rows)
        if "rays" in families:
            cast = ask_rays(t, sc, rec, f"{what} ({who})", scale, longest, floors=cast is None,
                            want=None if cast is None else [h for _, h in cast], rays=None if cast is None else [r for r, _ in cast])
        # the two leg calls: a tile walks only the cells it owns, from its own origin; the legs stay in world coordinates
        if "legs" in families:
            hits = ask_legs(t, sc, rec, f"{what} ({who})", want=hits)
        if "intervals" in families:
            spans = ask_intervals(t, sc, rec, f"{what} ({who})", want=spans)
    for t, who in twins:
        assert rec.tobytes() == t.read_agents().tobytes(), what
    for t, who in twins:  # (last: the agents of the high quadrant leave both)
        if by_id is not None:
            ask_by_id(t, rec, by_id, f"{what} ({who})")
        if removal:
            ask_removal(t, sc, rec, f"{what} ({who})")
    assert len({t.read_agents().tobytes() for t, _ in twins}) == 1, what


# ---- tile engines that hold ghosts: between a halo unpack and the step (tests/test_gpu_queries_ghost_tiles.py) -------------
def populate_kept(sc, sim):
    """Scene.populate that keeps what a selection by owner needs -> [(high-level planner, the ids of its agents)]"""
    out = []
    for pts, vel in sc.parts:
        hlp = StubHighLevelPlan(vel)
        out.append((hlp, np.asarray(sim.add_agents(np.asarray(pts), hlp, LP, sc.eyesight), dtype=np.uint64)))
    return out


def ghost_twins(sc, shape, halo, weights=None, phases=1, flags=0, steps=STEPS, meshes=1):
    """`meshes` LocalTileMesh (the Python mesh, whose exchange a test can make by hand) and a single engine, populated
    and stepped alike -> ([mesh, ...], single, [(planner, ids)] of the first mesh)"""
    from rmf_crowdsim_amd import LocationHash2D, Simulation
    from rmf_crowdsim_amd.tiles import LocalTileMesh
    twins = [LocalTileMesh(LocationHash2D(**sc.grid), shape, halo, weights=weights, phases=phases, flags=flags)
             for _ in range(meshes)] + [Simulation(LocationHash2D(**sc.grid), flags=flags)]
    kept = [populate_kept(sc, t) for t in twins]
    for _ in range(steps):
        for t in twins:
            t.step(DT)
    return twins[:-1], twins[-1], kept[0]


def unpack_ghosts(mesh):
    """The first half of LocalTileMesh.step: pack, move the buffers, unpack.  Every engine holds its ghost ring."""
    if mesh.phases == 2:
        mesh._exchange(0)
        mesh._exchange(1)
    else:
        mesh._exchange_all()


def finish_step(mesh, dt=DT, report=False):
    """The second half of LocalTileMesh.step for a mesh without source-sinks"""
    for e in mesh.engines:
        e.step(dt, report=report)


def mesh_rects(mesh):
    return rects_of(mesh.layout.x_edges, mesh.layout.y_edges)


def held_by_tiles(sc, rects, rec, halo):
    """By numpy alone, per tile of `rects`: (the records it owns, the records its ghost ring holds after an unpack: those
    whose cell lies in its rectangle grown by `halo` cells, clipped to the grid, but not in the rectangle)"""
    row, col = sc.cells_of(rec)
    own = owners(rects, sc, rec)
    out = []
    for k, (x0, x1, y0, y1) in enumerate(np.asarray(rects, dtype=np.int64).tolist()):
        grown = (row >= x0 - halo) & (row < x1 + halo) & (col >= y0 - halo) & (col < y1 + halo)
        out.append((rec[own == k], rec[grown & (own != k)]))
    return out


def _join(own, ghosts):
    return _sorted(np.concatenate([own, ghosts]))


def _differs(a, b):
    """do two answers of a restatement differ (arrays, or tuples of arrays)"""
    a, b = (a if isinstance(a, (tuple, list)) else (a,)), (b if isinstance(b, (tuple, list)) else (b,))
    return any(np.asarray(p).tobytes() != np.asarray(q).tobytes() for p, q in zip(a, b))


def cut_sides(sc, rect):
    """The sides of a tile's rectangle that are cuts (a neighbour and a ring lie beyond): (axis, the owned row or column
    next to the cut, the ring row or column next to that)"""
    x0, x1, y0, y1 = (int(v) for v in rect)
    sides = []
    if x0 > 0:
        sides.append((0, x0, x0 - 1))
    if x1 < sc.rows:
        sides.append((0, x1 - 1, x1))
    if y0 > 0:
        sides.append((1, y0, y0 - 1))
    if y1 < sc.cols:
        sides.append((1, y1 - 1, y1))
    return sides


def ghost_floors(sc, rects, held, halo, distance, least=20, loose=()):
    """By numpy alone, before any engine is asked: every tile holds at least `least` ghosts; at every side of a tile that
    is a cut an owned agent stands in the owned row (column) next to it and a ghost in the ring row (column) beyond,
    the two closer than `distance` (an off-by-one clip of a walk by own_* then changes an answer); on at least one tile
    own_x0, own_x1, own_y0, own_y1 of the local grid are four different numbers.  loose: the tiles whose sides are only
    printed (a tile that owns nobody, a tile whose crowd stands far from its cuts)."""
    four = 0
    for k, ((own, ghosts), rect) in enumerate(zip(held, np.asarray(rects, dtype=np.int64).tolist())):
        x0, x1, y0, y1 = rect
        lx0, ly0 = max(x0 - halo, 0), max(y0 - halo, 0)
        local = (x0 - lx0, x1 - lx0, y0 - ly0, y1 - ly0)  # own_x0, own_x1, own_y0, own_y1 (cs_engine::set_geometry)
        four += len(set(local)) == 4
        sides = []
        for axis, inner, outer in cut_sides(sc, rect):
            a = own[sc.cells_of(own)[axis] == inner]
            g = ghosts[sc.cells_of(ghosts)[axis] == outer]
            near = 0
            if len(a) and len(g):
                d2 = (a["x"][:, None] - g["x"][None, :]) ** 2 + (a["y"][:, None] - g["y"][None, :]) ** 2
                near = int((d2 < distance * distance).sum())
            sides.append((("row", "column")[axis], inner, len(a), len(g), near))
        print(f"{sc.name}: tile {k} {rect} (own_* {local}) owns {len(own)} agents and holds {len(ghosts)} ghosts; "
              f"(axis, owned line, agents in it, ghosts beyond, pairs within {distance:.2f} m): {sides}")
        assert len(ghosts) >= least, (k, len(ghosts))
        assert k in loose or all(s[2] > 0 and s[3] > 0 and s[4] > 0 for s in sides), (k, sides)
    assert four >= 1
    return held


def ghost_selections(sc, rect, own, ghosts, halo, handle_of):
    """Selections that straddle the cuts of a tile: its rectangle grown by halo + 1 cells; a box of 6 x 6 cells round a
    ghost; a circle of 2.5 cells round another; the speeds of the half of the crowd (slower or faster) a ghost belongs
    to; the planner of a ghost.  handle_of(agent id) -> the handle of its high-level planner."""
    ox, oy = sc.grid["offset"]
    cell = sc.cell
    x0, x1, y0, y1 = (int(v) for v in rect)
    g, h = ghosts[0], ghosts[len(ghosts) // 2]
    both = _join(own, ghosts)
    mid = _speeds(both)[1]
    slow = float(np.hypot(g["vx"], g["vy"])) < mid
    return [("the tile and two cells round it", selection(_abi.CS_SEL_RECT, x0=ox + (x0 - halo - 1) * cell, y0=oy + (y0 - halo - 1) * cell,
                                                          x1=ox + (x1 + halo + 1) * cell, y1=oy + (y1 + halo + 1) * cell)),
            ("a box round a ghost", selection(_abi.CS_SEL_RECT, x0=float(g["x"]) - 3 * cell, y0=float(g["y"]) - 3 * cell,
                                              x1=float(g["x"]) + 3 * cell, y1=float(g["y"]) + 3 * cell)),
            ("a circle round a ghost", selection(_abi.CS_SEL_CIRCLE, cx=float(h["x"]), cy=float(h["y"]), r=2.5 * cell)),
            ("the speed of a ghost", selection(_abi.CS_SEL_SPEED, speed_lo=0.0 if slow else mid, speed_hi=mid if slow else INF)),
            ("the planner of a ghost", selection(_abi.CS_SEL_HLP, hlp=int(handle_of(int(g["id"])))))]


def ghost_rays(sc, rect, own, ghosts, halo):
    """Rays for a tile that holds ghosts: from 32 ghosts (origins in the ring; without `ignore` each starts inside its
    ghost) towards the middle of the tile and on to the ring beyond; along the first and the last owned row and column
    from 3 cells outside the grown rectangle, through ring, tile and ring; the fans and random rays of ray_sets about the
    tile's own and ghost records."""
    ox, oy = sc.grid["offset"]
    cell = sc.cell
    x0, x1, y0, y1 = (int(v) for v in rect)
    mid = np.array([ox + 0.5 * (x0 + x1) * cell, oy + 0.5 * (y0 + y1) * cell])
    g = ghosts[np.linspace(0, len(ghosts) - 1, min(32, len(ghosts))).astype(np.int64)]
    o = np.column_stack([g["x"], g["y"]])
    u = mid[None, :] - o
    u /= np.hypot(u[:, 0], u[:, 1])[:, None]
    through = rays_ref.rays_array(o, u)
    lines_o, lines_u = [], []
    for r in (x0, x1 - 1):
        for f in (0.25, 0.75):
            lines_o.append((ox + (r + f) * cell, oy + (y0 - halo - 3) * cell))
            lines_u.append((0.0, 1.0))
    for c in (y0, y1 - 1):
        for f in (0.25, 0.75):
            lines_o.append((ox + (x0 - halo - 3) * cell, oy + (c + f) * cell))
            lines_u.append((1.0, 0.0))
    lines = rays_ref.rays_array(np.array(lines_o), np.array(lines_u))
    return np.concatenate([through, lines, ray_sets(_join(own, ghosts), sc.grid, 30.0, beams=45, segments=150)])


def ghost_legs(sc, rect, own, ghosts, halo, intervals=False):
    """Legs for a tile that holds ghosts: waits of 1.5 s 0.1 cell beside 32 ghosts; legs of 4 s along the first and the
    last owned row and column from 2 cells outside the grown rectangle to 2 cells beyond it; the leg sets of the leg
    tests about the tile's own and ghost records."""
    ox, oy = sc.grid["offset"]
    cell = sc.cell
    x0, x1, y0, y1 = (int(v) for v in rect)
    g = ghosts[np.linspace(0, len(ghosts) - 1, min(32, len(ghosts))).astype(np.int64)]
    waits = legs_ref.legs_array(np.column_stack([g["x"] + 0.1 * cell, g["y"]]), (0.0, 0.0), 0.0, 1.5)
    starts, vels = [], []
    for r in (x0, x1 - 1):
        starts.append((ox + (r + 0.5) * cell, oy + (y0 - halo - 2) * cell))
        vels.append((0.0, (y1 - y0 + 2 * halo + 4) * cell / 4.0))
    for c in (y0, y1 - 1):
        starts.append((ox + (x0 - halo - 2) * cell, oy + (c + 0.5) * cell))
        vels.append(((x1 - x0 + 2 * halo + 4) * cell / 4.0, 0.0))
    lines = np.concatenate([legs_ref.legs_array(np.array([s]), v, 0.0, 4.0) for s, v in zip(starts, vels)])
    both = _join(own, ghosts)
    rest = interval_legs(both, sc.grid, segments=150) if intervals else leg_sets(both, sc.grid, segments=150)
    return np.concatenate([waits, lines, rest])


def ghost_raster(sc, rect, halo):
    """the tile's rectangle grown by halo + 1 cells, cell by cell: a raster window across every cut of the tile"""
    ox, oy = sc.grid["offset"]
    x0, x1, y0, y1 = (int(v) for v in rect)
    return field_ref.desc(ox + (x0 - halo - 1) * sc.cell, oy + (y0 - halo - 1) * sc.cell, sc.cell, sc.cell,
                          x1 - x0 + 2 * halo + 2, y1 - y0 + 2 * halo + 2)


def ask_tile_with_ghosts(engine, sc, rect, own, ghosts, elsewhere, halo, name, monkeypatch, handle_of):
    """Every between-step read on ONE tile engine whose arrays hold ghosts: each answer is the restatement's on `own`, the
    records the tile owns, byte for byte (the raster's sums within field_reference.tolerance).  Before each call the
    floor that lets it fail, by the restatement alone: its answer on the owned records and the ghosts together differs
    from its answer on the owned records.  elsewhere: records the tile does not hold at all.  engine None: the floors
    alone, as tests/test_ghost_tile_floors.py evaluates them without a GPU.  -> the names of the floors met"""
    grid, cell = sc.grid, sc.cell
    both = _join(own, ghosts)
    met = []

    def floor(what, a, b, differ=None):
        assert _differs(a, b) if differ is None else differ, f"{name}, {what}: the ghosts do not change the restatement's answer"
        met.append(what)
        return engine is not None

    # the count and the list
    if floor("len and read_agents", own, both):
        assert len(engine) == len(own), name
        assert engine.read_agents().tobytes() == own.tobytes(), name
    # selections and counts
    sels = ghost_selections(sc, rect, own, ghosts, halo, handle_of)
    hlp_of = lambda rec: np.array([handle_of(int(i)) for i in rec["id"]], dtype=np.uint64)  # noqa: E731
    wants = []
    for what, sel in sels:
        want = own["id"][pred(sel, own, None, hlp_of(own), None)]
        wants.append(len(want))
        if not floor(f"select {what}", want, both["id"][pred(sel, both, None, hlp_of(both), None)]):
            continue
        n, got = select(engine, sel, cap=len(both) + 3)
        print(f"{name}, select {what}: restatement {len(want)} of {len(own)} owned, engine {n}")
        assert n == len(want) and got.tolist() == want.tolist(), (name, what)
        if len(want) > 3:
            n, few = select(engine, sel, cap=len(want) // 2)
            assert n == len(want) and few.tolist() == want[:len(want) // 2].tolist(), (name, what)
    if engine is not None:
        rc, counts = count(engine, [s for _, s in sels])
        assert rc == 0 and counts.tolist() == wants, name
        s = sels[0][1]
        assert engine.select_agents(rect=(s.x0, s.y0, s.x1, s.y1)).tolist() == own["id"].tolist(), name
        assert engine.count_agents([dict(rect=(s.x0, s.y0, s.x1, s.y1))]).tolist() == [len(own)], name
    # the raster, in the form cs_agent_field picks and in the global form
    d = ghost_raster(sc, rect, halo)
    want = field_ref.raster(d, own)
    if floor("agent_field", want[0], field_ref.raster(d, both)[0]):
        for limit in (None, "0"):
            if limit is None:
                monkeypatch.delenv("CS_FIELD_LDS_BYTES", raising=False)
            else:
                monkeypatch.setenv("CS_FIELD_LDS_BYTES", limit)
            for form in ("count", "both"):
                rc, cnt, sums = field_ref.field(engine, d, None, want=form)
                assert rc == 0, (name, field_ref.last_error(engine))
                field_ref.check(f"{name}, raster, {form}, LDS limit {limit}", cnt, sums, want)
        monkeypatch.delenv("CS_FIELD_LDS_BYTES", raising=False)
    # the distance queries, at 0.6 cell and at the halo; once with roles
    lhs_own, lhs_both = {}, {}
    half, slow = sels[1][1], sels[0][1]  # the roles: the box round a ghost, which lies across a cut, and the tile and its rings
    for c in (0.6, float(halo)):
        dist = c * cell
        if floor(f"close_pairs {c}", pairs_ref.pairs(own, grid, dist, cache=lhs_own), pairs_ref.pairs(both, grid, dist, cache=lhs_both)):
            pairs_ref.agree(engine, own, grid, dist, name=f"{name}, pairs, {c} cells", cache=lhs_own)
        # (where an owned agent stands within the distance of a ghost, the rows of the OWNED subjects must change: a ghost
        # is somebody's neighbour; elsewhere the ghosts' own rows are the difference)
        with_ghosts = neighbours_ref.neighbours(both, grid, dist, cache=lhs_both)
        across, _ = pairs_ref.pairs(both, grid, dist, np.isin(both["id"], own["id"]), np.isin(both["id"], ghosts["id"]),
                                    cache=lhs_both)
        if floor(f"agent_neighbours {c}", neighbours_ref.neighbours(own, grid, dist, cache=lhs_own),
                 with_ghosts[np.isin(with_ghosts["id"], own["id"])] if len(across) else with_ghosts):
            neighbours_ref.agree(engine, own, grid, dist, name=f"{name}, neighbours, {c} cells", cache=lhs_own, min_counts=(0, 2))
        if floor(f"agent_clusters {c}", clusters_ref.clusters(own, grid, dist, cache=lhs_own)[:3],
                 clusters_ref.clusters(both, grid, dist, cache=lhs_both)[:3]):
            clusters_ref.agree(engine, own, grid, dist, name=f"{name}, clusters, {c} cells", cache=lhs_own)
    dist = halo * cell
    if floor("close_pairs, two roles", pairs_ref.pairs(own, grid, dist, *pairs_ref.roles(half, slow, own), cache=lhs_own),
             pairs_ref.pairs(both, grid, dist, *pairs_ref.roles(half, slow, both), cache=lhs_both)):
        pairs_ref.agree(engine, own, grid, dist, half, slow, name=f"{name}, pairs, two roles", cache=lhs_own)
        neighbours_ref.agree(engine, own, grid, dist, half, slow, name=f"{name}, neighbours, two roles", cache=lhs_own)
        clusters_ref.agree(engine, own, grid, dist, half, min_size=2, name=f"{name}, clusters of one role", cache=lhs_own)
    # encounters
    args = (0.5, 3.0, halo * cell)
    want = encounters_ref.encounters(own, grid, *args)
    if floor("encounters", want, encounters_ref.encounters(both, grid, *args)):
        encounters_ref.agree(engine, own, grid, *args, name=f"{name}, encounters", want=want)
    # rays
    rays = ghost_rays(sc, rect, own, ghosts, halo)
    for radius in (0.2, 0.4):
        want = rays_ref.cast(own, grid, rays, radius)
        if floor(f"cast_rays {radius}", want, rays_ref.cast(both, grid, rays, radius)):
            rays_ref.agree(engine, own, grid, rays, radius, name=f"{name}, rays {radius}", want=want)
    # leg conflicts and leg intervals: everybody slower than 2 m/s within 0.4 cell; the walk without a reach within 0.8 cell
    for what, ref, restate, legs in (("leg_conflicts", legs_ref, legs_ref.conflicts, ghost_legs(sc, rect, own, ghosts, halo)),
                                     ("leg_intervals", intervals_ref, intervals_ref.intervals,
                                      ghost_legs(sc, rect, own, ghosts, halo, intervals=True))):
        for dist, speed_max in ((0.4 * cell, 2.0), (0.8 * cell, INF)):
            want = restate(own, grid, legs, dist, speed_max)
            if floor(f"{what} {speed_max}", want, restate(both, grid, legs, dist, speed_max)):
                ref.agree(engine, own, grid, legs, dist, speed_max, name=f"{name}, {what} {(dist, speed_max)}", want=want)
    # the Python surface of the two leg calls: waits beside ghosts, and a path from ring to ring through the tile
    from rmf_crowdsim_amd.simulation import free_spans, merge_leg_intervals, paths_legs
    g = ghosts[np.linspace(0, len(ghosts) - 1, min(24, len(ghosts))).astype(np.int64)]
    spots = np.column_stack([g["x"] + 0.3, g["y"]])
    waits = legs_ref.legs_array(spots, (0.0, 0.0), 0.5, 4.0)

    def spans(rec):
        rows, _ = intervals_ref.intervals(rec, grid, waits, 0.3, 2.0)
        return free_spans(*merge_leg_intervals(rows, len(waits)), waits["t0"], waits["t1"])
    want = spans(own)
    if floor("free_intervals", None, None, differ=want != spans(both)):
        assert engine.free_intervals(spots, 0.5, 4.0, 0.3, 2.0) == want, name
    # (from the ghost that stands farthest from every owned agent, 5 cm beside it: with ghosts it is the conflict, at once)
    if len(own):
        apart = ((ghosts["x"][:, None] - own["x"][None, :]) ** 2 + (ghosts["y"][:, None] - own["y"][None, :]) ** 2).min(axis=1)
        lone = ghosts[int(np.argmax(apart))]
    else:
        lone = ghosts[0]
    start = np.array([float(lone["x"]) + 0.05, float(lone["y"])])
    mid = np.array([np.median(both["x"]), np.median(both["y"])])
    far = np.array([g["x"].max(), g["y"].max()]) + 0.5
    path = (np.array([start, mid, mid, far]), np.array([0.0, 4.0, 5.0, 9.0]))  # (the second leg is a wait)
    legs, _ = paths_legs([path])

    def first(rec):
        hits = legs_ref.conflicts(rec, grid, legs, 0.3, 2.0)
        at = np.nonzero(hits["id"] != legs_ref.NO_HIT)[0]
        if not len(at):
            return None
        k = int(at[0])
        l, s = legs[k], float(hits["s"][k])
        return (int(hits["id"][k]), float(l["t0"]) + s, k, (float(l["x0"]) + float(l["vx"]) * s, float(l["y0"]) + float(l["vy"]) * s))
    want = first(own)
    if floor("path_conflict", None, None, differ=want != first(both)):
        assert engine.path_conflict(*path, 0.3, 2.0) == want, name
    # reads by id: owned agents, ghosts of this tile, agents the tile does not hold at all
    some = [r[np.linspace(0, len(r) - 1, min(16, len(r))).astype(np.int64)] for r in (own, ghosts, elsewhere)]
    ids = np.concatenate([r["id"] for r in some])[::-1].copy()
    mine = np.isin(ids, own["id"])
    assert len(some[2]) > 0 or len(elsewhere) == 0
    if floor("read_agents_by_id", mine, np.isin(ids, both["id"])):
        out, found = engine.read_agents_by_id(ids, missing_ok=True)
        assert np.asarray(found, dtype=bool).tolist() == mine.tolist(), name
        at = {int(i): j for j, i in enumerate(own["id"])}
        assert out[mine].tobytes() == own[[at[int(i)] for i in ids[mine]]].tobytes(), name
        blank = np.zeros(int((~mine).sum()), dtype=out.dtype)
        blank["id"] = ids[~mine]
        assert out[~mine].tobytes() == blank.tobytes(), name
        # asking has changed no record and nobody's ownership
        assert len(engine) == len(own) and engine.read_agents().tobytes() == own.tobytes(), name
    return met


# (scene, shape, halo, phases of the exchange, the rows and the columns of the placed cuts; None: the weights are the
# crowd's own points, whose cuts pass through the largest lattice of the lopsided crowd).  Row and column 24 pass through
# that lattice too; the middle tile of the (3, 1) and (1, 3) meshes is two halo rings thick, with a ring on both sides.
# "diagonal": the row cut through the first lattice, the column cut right behind it: the tile of rows 0-23 beyond column 29
# owns nobody and holds the last two columns of the lattice as ghosts.  "odd-far": cells of 2.3 m, the cuts through the
# lattice in the high corner of 700 x 900 cells.
GHOST_CASES = [("lopsided", (2, 2), 1, 1, None), ("lopsided", (2, 2), 2, 2, None), ("lopsided", (3, 1), 1, 2, ((24, 26), ())),
               ("lopsided", (3, 1), 2, 1, ((24, 28), ())), ("lopsided", (1, 3), 1, 1, ((), (24, 26))),
               ("lopsided", (1, 3), 2, 2, ((), (24, 28))), ("diagonal", (2, 2), 2, 1, ((24,), (29,))),
               ("odd-far", (2, 2), 1, 2, ((693,), (894,)))]
GHOST_IDS = [f"{s}-{a}x{b}-halo{h}-phases{p}" for s, (a, b), h, p, _ in GHOST_CASES]
# tiles exempt from the floor of the sides (ghost_floors): on the diagonal scene the column cut lies BEHIND the lattice, so
# that tile 1 owns nobody: nobody stands beyond it for tiles 0 and 2 (their row sides meet the floor), and tile 3 owns the
# second lattice, 80 cells from its cuts (its ghosts are a corner of the first).  The floor holds on every tile of every
# other case.
GHOST_LOOSE = {"diagonal": (0, 1, 2, 3)}


def ghost_case_weights(sc, shape, halo, placed):
    if placed is None:
        return np.concatenate([p for p, _ in sc.parts])
    return placed_cut_weights(sc, shape, placed[0], placed[1], halo)


def ghost_case_floors(case, rec):
    """By TileLayout and numpy alone, for the records `rec` of the scene's crowd after the steps: the rectangles, what every
    tile owns and holds as ghosts, the floors of ghost_floors -> (sc, rects, held)"""
    name, shape, halo, _, placed = case
    sc = scene(name)
    lay = layout(sc, shape, halo, points=ghost_case_weights(sc, shape, halo, placed))
    rects = rects_of(lay.x_edges, lay.y_edges)
    if placed is not None:
        assert rects.tolist() == rects_of([0, *placed[0], sc.rows], [0, *placed[1], sc.cols]).tolist()
    assert all(int(r[1]) - int(r[0]) != int(r[3]) - int(r[2]) for r in rects)  # (no tile is square)
    held = held_by_tiles(sc, rects, rec, halo)
    ownerless = [k for k, (own, _) in enumerate(held) if len(own) == 0]
    assert len(ownerless) == (1 if name == "diagonal" else 0)
    ghost_floors(sc, rects, held, halo, halo * sc.cell, loose=tuple(ownerless) + GHOST_LOOSE.get(name, ()))
    return sc, rects, held


def ghost_state(case, meshes=1, flags=0):
    """-> (sc, meshes, single, rec, rects, held, handle_of): the twins of a case stepped, the floors of ghost_case_floors
    asserted on the single engine's records before any tile is asked, the ghosts of every mesh unpacked"""
    name, shape, halo, phases, placed = case
    sc = scene(name)
    tiles, single, kept = ghost_twins(sc, shape, halo, ghost_case_weights(sc, shape, halo, placed), phases, flags, meshes=meshes)
    rec = single.read_agents()
    _, rects, held = ghost_case_floors(case, rec)
    table = {}
    for hlp, ids in kept:
        handles = {e._planner_handles[id(hlp)] for e in tiles[0].engines}
        assert len(handles) == 1  # (every engine numbers the planners alike)
        table.update((int(i), min(handles)) for i in ids.tolist())
    for mesh in tiles:
        assert mesh_rects(mesh).tolist() == rects.tolist()
        assert mesh.read_agents().tobytes() == rec.tobytes()
        unpack_ghosts(mesh)
        # (before the exchange a tile still holds the agents that walked across a cut in the last step: only now does
        # every tile hold the agents that stand in its cells)
        assert [len(e) for e in mesh.engines] == [len(own) for own, _ in held]
    return sc, tiles, single, rec, rects, held, table.__getitem__


RECUT_FROM = ((24,), (24,))  # the cuts a mesh is made with before test_a_recut_of_tiles_that_hold_ghosts moves them


def ghost_recut_floors(sc, rec, before, halo=1, shape=(2, 2)):
    """By TileLayout and numpy alone: what a re-cut of the mesh with the rectangles `before` must give for the records
    `rec`, and that it can be got wrong: the rings hold at least 20 ghosts each, every edge moves, and histograms that
    counted the ghosts as well would put an edge elsewhere.  -> (rects after the re-cut, agents per tile after it)"""
    held = held_by_tiles(sc, before, rec, halo)
    cut = layout(sc, shape, halo, rec=rec)
    after = rects_of(cut.x_edges, cut.y_edges)
    n_after = np.bincount(owners(after, sc, rec), minlength=len(after))
    twice = layout(sc, shape, halo, rec=np.concatenate([rec] + [g for _, g in held]))
    print(f"{sc.name}: cuts {cuts_of(before)} -> {cuts_of(after)}, tiles hold {n_after.tolist()}; the rings hold "
          f"{[len(g) for _, g in held]} ghosts; histograms with the ghosts would cut at {cuts_of(rects_of(twice.x_edges, twice.y_edges))}")
    assert min(len(g) for _, g in held) >= 20
    assert all(a != b for a, b in zip(sum(cuts_of(before), []), sum(cuts_of(after), [])))
    assert (twice.x_edges, twice.y_edges) != (cut.x_edges, cut.y_edges)
    return after, n_after
