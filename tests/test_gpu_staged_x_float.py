"""The tiled step kernel stages x as an exact float where a window stages at most four rows (k_step_tiled, XF: h = 1 with
one- or two-row bands) and keeps the integer form everywhere else.  Either form must give the bits of the gather kernel
(flags = 1), which forms every relative position with the canonical integer arithmetic (fix_rel).  The cases sit where
the float form could go wrong: staged x at exactly -2^24 and +2^24 (offsets 0 and the largest f32 below the cell, in
the first and last staged row of a window), equal x (+0), cells whose fixed-point size is below 2^23, the grid's first
and last row (three staged rows), a record beyond the exact range (the window must leave the LDS path and be counted),
and the instantiation that source-sink crowds run.  The rule itself: tests/test_staged_x_exact.py.  Needs an MI355X."""
import numpy as np
import pytest

from rmf_crowdsim_amd import (LocationHash2D, MonotonicCrowd, Simulation, SourceSink, StubHighLevelPlan, Zanlungo, _abi,
                              scenes)

pytestmark = pytest.mark.gpu

LP = scenes.METRIC_ZANLUNGO
N = 4096
TOUCH = 0.45  # nobody is moved to within this of anybody: beyond 2 R = 0.4 m, so no pair overlaps (t_i = 0, NaN forces)


def snap_to_row_edges(pts, cell, seed, reach=0.3):
    """Moves a seeded subset of the agents within `reach` of a cell edge in x (x runs across the grid's rows) onto the
    range's extremes: offset exactly 0, or the largest f32 below the cell size.  Returns (points, kind per agent:
    0 untouched, 1 offset 0, 2 largest offset)."""
    rng = np.random.default_rng(seed)
    top = float(np.nextafter(np.float32(cell), np.float32(0.0)))
    out, kind = pts.copy(), np.zeros(len(pts), dtype=int)
    for i in rng.permutation(len(pts)):
        row = np.floor(out[i, 0] / cell)
        off = out[i, 0] - row * cell
        if off < reach:
            x, k = row * cell, 1
        elif off > cell - reach:
            x, k = row * cell + top, 2
        else:
            continue
        if rng.random() < 0.25:
            continue
        d = np.hypot(out[:, 0] - x, out[:, 1] - out[i, 1])
        d[i] = np.inf
        if d.min() >= TOUCH:
            out[i, 0], kind[i] = x, k
    return out, kind


def edge_crowd(cell, border):
    """The creep scene's crowd (4,096 agents, 2.5 / m^2) with a seeded subset on the cell edges in x.  border: the
    grid ends where the crowd ends, so that its first and last row (windows of three staged rows) hold agents."""
    pts, grid, _, group = scenes.uniform_crowd(N, seed=5, cell_size=cell, margin=0.2 if border else 10.0)
    lattice = pts
    pts, kind = snap_to_row_edges(pts, cell, seed=31)
    if border:
        # (nobody a float's spacing below the grid's upper end: the first force would push such an agent off the grid)
        row = np.floor(pts[:, 0] / cell)
        back = (kind == 2) & (row == row.max())
        pts[back, 0], kind[back] = lattice[back, 0], 0
        # (the reference bounds the x index by height / cell and the y index by width / cell: location_hash_2d.rs:54-66;
        # half a cell more, so that the quotient's floor does not hang on its last bit)
        rows, cols = (int(pts[:, a].max() // cell) + 1 for a in (0, 1))
        grid = dict(width=(cols + 0.5) * cell, height=(rows + 0.5) * cell, cell_size=cell, offset=(0.0, 0.0))
    return pts, grid, group, kind


def run(flags, pts, grid, group, eyesight, steps=5, extra=()):
    sim = Simulation(LocationHash2D(**grid), flags=flags)
    scenes.add_counterflow(sim, pts, group, scenes.CREEP_SPEED, Zanlungo(*LP), eyesight)
    for p in extra:
        sim.add_agents([p], StubHighLevelPlan((0.0, scenes.CREEP_SPEED)), Zanlungo(*LP), eyesight)
    for _ in range(steps):
        sim.step(0.05)
    assert sim.last_report["n_nonfinite"] == 0
    return sim


def stats(sim):
    return (sim.kernel_stat(_abi.CS_STAT_WINDOWS_OFF_LDS), sim.kernel_stat(_abi.CS_STAT_STEPS_ON_KEPT_WINDOWS))


@pytest.fixture(scope="module")
def extremes():
    """cell 2.0 m (cs_fix = 2^23) and its gather result, computed once for both window forms"""
    pts, grid, group, kind = edge_crowd(2.0, border=False)
    gather = run(1, pts, grid, group, 2.0).read_agents()
    return pts, grid, group, kind, gather


@pytest.mark.parametrize("keep", ["0", None], ids=["plain-windows", "kept-windows"])
def test_range_extremes_equal_gather_bitwise(extremes, monkeypatch, keep):
    """Offsets exactly 0 and the largest f32 below 2.0 m: staged x = -2^24 in a window's first staged row (the row above a
    two-row band: an odd row) and +2^24 in its last (the row below: an even row); pairs at equal x within sight (+0)."""
    pts, grid, group, kind, gather = extremes
    row = np.floor(pts[:, 0] / 2.0).astype(int)
    assert ((kind == 1) & (row % 2 == 1)).sum() >= 8 and ((kind == 2) & (row % 2 == 0)).sum() >= 8
    # the engine's offsets are the extremes, to the bit
    off = (pts[:, 0] - row * 2.0).astype(np.float32)
    assert (off[kind == 1] == 0.0).all() and (off[kind == 2] == np.nextafter(np.float32(2.0), np.float32(0.0))).all()
    s = np.nonzero(kind)[0]
    same_x = (pts[s, None, 0] == pts[None, s, 0]) & (np.abs(pts[s, None, 1] - pts[None, s, 1]) < 2.0)
    assert (same_x.sum() - len(s)) // 2 >= 8
    if keep is None:
        monkeypatch.delenv("CS_WINDOWS_KEEP", raising=False)
    else:
        monkeypatch.setenv("CS_WINDOWS_KEEP", keep)
    sim = run(2, pts, grid, group, 2.0)
    off_lds, kept = stats(sim)
    print(f"keep {keep}: {int((kind == 1).sum())} agents at offset 0, {int((kind == 2).sum())} at the largest offset, "
          f"{(same_x.sum() - len(s)) // 2} pairs at equal x in sight; windows off LDS {off_lds}, steps on kept windows {kept}")
    assert sim.read_agents().tobytes() == gather.tobytes()
    assert off_lds == 0  # every staged x is within the exact range: nobody leaves the LDS path
    assert (kept > 0) == (keep is None)  # the instantiation with builder workgroups / the plain one


@pytest.mark.parametrize("cell", [1.5, 2.3])
def test_other_cells_and_the_grid_edge_equal_gather_bitwise(cell):
    """Eyesight = cell (h = 1), cs_fix below 2^23, the crowd reaching the grid's first and last row."""
    pts, grid, group, kind = edge_crowd(cell, border=True)
    row = np.floor(pts[:, 0] / cell).astype(int)
    n_rows = int(grid["height"] / cell)
    assert (row == 0).sum() >= 32 and (row == n_rows - 1).sum() >= 32 and (kind != 0).sum() >= 64
    outs = [run(flags, pts, grid, group, cell) for flags in (2, 1)]
    assert stats(outs[0])[0] == 0
    assert outs[0].read_agents().tobytes() == outs[1].read_agents().tobytes()


def test_integer_form_equals_gather_bitwise():
    """cell 1.0 m, eyesight 2.0 m: h = 2, six staged rows: the windows keep the integer form."""
    pts, grid, group, _ = edge_crowd(1.0, border=False)
    outs = [run(flags, pts, grid, group, 2.0) for flags in (2, 1)]
    assert stats(outs[0])[0] == 0
    assert outs[0].read_agents().tobytes() == outs[1].read_agents().tobytes()


def test_a_record_beyond_the_exact_range_sends_its_window_to_the_gather_path():
    """An agent clamped below the grid in x is a member of a cell of row 0 and keeps its negative offset.  In a border
    window (rows 0 .. 2 staged, row 0 at -1 cell) its staged x is -cs_fix + fix_coord(offset): beyond -2^24 once the
    offset is below -2.0 m (cs_fix = 2^23).  Two such agents, in different windows:
      * at x = -0.5 m: within sight of row 0's agents and within the exact range: the LDS path takes it;
      * at x = -2.5 m: beyond the range (and, with the eyesight of at most one cell that h = 1 means, beyond everybody's
        sight: the range cannot be left nearer than that): its window must take the gather path for the step, and be counted.
    Tiled == gather bit for bit with both, and a scene without the second leaves the counter at 0."""
    pts, grid, group, _ = edge_crowd(2.0, border=True)
    ys = np.sort(pts[np.floor(pts[:, 0] / 2.0) == 0, 1])
    near, far = (-0.5, float(ys[len(ys) // 4]) + 0.3), (-2.5, float(ys[3 * len(ys) // 4]) + 0.3)
    # the first one really has neighbours in sight
    assert (np.hypot(pts[:, 0] - near[0], pts[:, 1] - near[1]) < 2.0).sum() >= 2
    with_far = [run(flags, pts, grid, group, 2.0, extra=(near, far)) for flags in (2, 1)]
    assert with_far[0].last_report["n_clamped"] == with_far[1].last_report["n_clamped"]
    a, g = with_far[0].read_agents(), with_far[1].read_agents()
    assert len(a) == N + 2 and a["x"].min() < -2.0
    assert a.tobytes() == g.tobytes()
    print(f"windows off LDS with the record beyond the range: {stats(with_far[0])[0]}")
    assert stats(with_far[0])[0] >= 1
    without = [run(flags, pts, grid, group, 2.0, extra=(near,)) for flags in (2, 1)]
    assert without[0].read_agents().tobytes() == without[1].read_agents().tobytes()
    assert stats(without[0])[0] == 0


def test_source_sink_crowd_equals_gather_bitwise():
    """~2,048 walkers fed by source-sinks (the instantiations that keep the epilogue's context in registers): the lanes
    fill, then ten steps are compared one by one."""
    lanes, grid, fill_steps = scenes.stream_lanes(2048, cell_size=2.0)
    lp = Zanlungo(*LP)
    runs = []
    for flags in (2, 1):
        sim = Simulation(LocationHash2D(**grid), flags=flags)
        plans = {}
        for src, dst, vel in lanes:
            sim.add_source_sink(SourceSink(src, 0.5, MonotonicCrowd(1000.0), plans.setdefault(vel, StubHighLevelPlan(vel)),
                                           lp, [dst], False, 2.0))
        for _ in range(fill_steps):
            sim.step(0.05)
        snaps = []
        for _ in range(10):
            sim.step(0.05)
            snaps.append(sim.read_agents())
        runs.append((snaps, stats(sim)[0]))
    (a, off_lds), (g, _) = runs
    assert len(a[-1]) >= 1500 and off_lds == 0
    for x, y in zip(a, g):
        assert x.tobytes() == y.tobytes()
