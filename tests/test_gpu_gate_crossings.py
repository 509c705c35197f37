"""Who crosses a line on one engine (include/crowdstep_state.h, Simulation.gate_crossings / count_gate_crossings): the
engine against the numpy restatement of the rule (tests/gates_reference.py) applied to its OWN read_agents().  Equality is
exact: the gate, dir, the id and the bits of s and u of every row, the counts per gate and direction and the returned
count; there is no tolerance anywhere ("Who crosses a line")."""
import numpy as np
import pytest

from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, LocationHash2D,
                              NoLocalPlan, Selection, Simulation, StubHighLevelPlan, _abi)
from close_pairs_reference import rectangle, roles, takes_part
from gates_reference import GATE_CROSSING_DTYPE, SIZE_MAX, agree, call, crossings, gates_array, last_error, path_gates
from select_reference import drain, selection
from test_gpu_agent_write import _steps
from test_gpu_encounters import _advance, _scene

pytestmark = pytest.mark.gpu
INF = float("inf")
GRID = dict(width=32.0, height=32.0, cell_size=2.0, offset=(-4.0, 3.0))  # 16 x 16 cells: x in [-4, 28), y in [3, 35)
CROWDED = ((3, 3, 65), (8, 11, 128), (12, 5, 129))  # (row of x, column of y, agents): the 64-slot stepping of a run


def randomize(a, seed, top=2.5):
    """write every agent a random f32 velocity of up to `top` m/s (a tenth stand still) -> the records afterwards"""
    rng = np.random.default_rng(seed)
    w = a.read_agents()
    n = len(w)
    phi, speed = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(0.0, top, n)
    speed[rng.uniform(size=n) < 0.1] = 0.0
    w["vx"], w["vy"] = (speed * np.cos(phi)).astype(np.float32), (speed * np.sin(phi)).astype(np.float32)
    a.write_agents(w, fields=("velocity",))
    return a.read_agents()


def walkers(grid=GRID, n=3000, seed=5, flags=0, crowded=CROWDED):
    """n agents standing anywhere on the grid, then written random velocities (randomize); the cells of `crowded` hold
    exactly the numbers named there -> (engine, its records)"""
    rng = np.random.default_rng(seed)
    gx0, gx1, gy0, gy1 = rectangle(grid)
    cell = float(grid["cell_size"])
    pts = np.column_stack([rng.uniform(gx0 + 0.01, gx1 - 0.01, n), rng.uniform(gy0 + 0.01, gy1 - 0.01, n)])
    row, col = np.floor((pts[:, 0] - gx0) / cell), np.floor((pts[:, 1] - gy0) / cell)
    k = 0
    for r, c, m in crowded:
        pts[(row == r) & (col == c), 0] += cell  # (the cells of `crowded` are not neighbours)
    for r, c, m in crowded:
        pts[k:k + m] = np.column_stack([gx0 + (r + rng.uniform(0.05, 0.95, m)) * cell, gy0 + (c + rng.uniform(0.05, 0.95, m)) * cell])
        k += m
    a = Simulation(LocationHash2D(**grid), flags=flags)
    a.add_agents(pts, StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 2.0)
    a.step(0.05)
    rec = randomize(a, seed + 1)
    assert len(rec) == n and takes_part(rec, grid).all()
    row, col = np.floor((rec["x"] - gx0) / cell), np.floor((rec["y"] - gy0) / cell)
    for r, c, m in crowded:
        assert int(((row == r) & (col == c)).sum()) == m
    return a, rec


def crowd_gates(rec, grid, seed=7, each=40, t1=2.0):
    """Gates made for a crowd: `each` random doors of 2 m (along x, along y, oblique), gates through cell corners, along
    cell boundaries and along the grid's edges, partly and wholly outside the grid and longer than it, gates with A == B,
    windows that open later, windows so short that the reach stays below a cell, and gates laid through reported agent
    positions (from one, and level with one): their agents are on the line when the window opens."""
    rng = np.random.default_rng(seed)
    part = rec[takes_part(rec, grid)]
    gx0, gx1, gy0, gy1 = rectangle(grid)
    cell = float(grid["cell_size"])
    lo_x, hi_x, lo_y, hi_y = part["x"].min(), part["x"].max(), part["y"].min(), part["y"].max()
    seg, t0s, t1s = [], [], []

    def add(ax, ay, bx, by, t0=0.0, t1_=None):
        seg.append((float(ax), float(ay), float(bx), float(by)))
        t0s.append(t0)
        t1s.append(t0 + t1 if t1_ is None else t1_)

    for k in range(each):  # doors
        cx, cy = rng.uniform(lo_x, hi_x), rng.uniform(lo_y, hi_y)
        phi = (0.0, 0.5 * np.pi, rng.uniform(0.0, 2.0 * np.pi))[k % 3]
        dx, dy = np.cos(phi), np.sin(phi)
        if k % 3 == 0:
            dx, dy = (1.0, 0.0) if k % 2 else (-1.0, 0.0)
        if k % 3 == 1:
            dx, dy = (0.0, 1.0) if k % 2 else (0.0, -1.0)
        add(cx - dx, cy - dy, cx + dx, cy + dy, t0=(0.0, 0.5, 1.5)[k % 3] if k >= each // 2 else 0.0)
    mid_r, mid_c = int((0.5 * (lo_x + hi_x) - gx0) // cell), int((0.5 * (lo_y + hi_y) - gy0) // cell)
    for d in range(-2, 3):  # through cell corners, both diagonals; along cell boundaries, both senses
        x, y = gx0 + (mid_r + d) * cell, gy0 + (mid_c - d) * cell
        add(x - 3 * cell, y - 3 * cell, x + 2 * cell, y + 2 * cell)
        add(x - 2 * cell, y + 2 * cell, x + 3 * cell, y - 3 * cell, t0=0.5)
        add(x, y - 4 * cell, x, y + 3 * cell)
        add(x + 5 * cell, y, x - 2 * cell, y)
    for ax, ay, bx, by in ((gx0, gy0, gx0, gy1), (gx1, gy1, gx1, gy0), (gx0, gy0, gx1, gy0), (gx1, gy1, gx0, gy1)):
        add(ax, ay, bx, by)  # the grid's edges
    mx, my = float(np.median(part["x"])), float(np.median(part["y"]))
    add(mx, my, gx1 + 10.0, my + 1.0)  # partly outside
    add(mx, gy0 - 7.0, mx + 0.5, my)
    add(gx1 + 1.0, gy0, gx1 + 1.0, gy1)  # wholly outside, within reach of the edge
    add(gx0, gy0 - 30.0, gx1, gy0 - 30.0)  # wholly outside, beyond any reach
    add(1e9, 1e9, 1e9 + 5.0, 1e9 + 5.0)
    add(gx0 - 50.0, my, gx1 + 50.0, my)  # longer than the grid
    add(mx, gy1 + 80.0, mx + 1.0, gy0 - 80.0)
    add(gx0 - 20.0, gy0 - 25.0, gx1 + 30.0, gy1 + 20.0, t0=1.0)
    add(gx1 + 1e6, my, gx0 - 1e6, my + 0.25)
    add(mx, my, mx, my)  # A == B, on nobody and (below) on somebody
    for k in range(each // 2):  # a reach below one cell: 0.1 s at up to 2.5 m/s
        cx, cy = rng.uniform(lo_x, hi_x), rng.uniform(lo_y, hi_y)
        add(cx - 1.5, cy - 0.5 * (k % 3), cx + 1.5, cy + 0.5 * (k % 2), t1_=0.1)
    moving = part[(part["vx"] != 0) | (part["vy"] != 0)]
    moving = moving[np.argsort(moving["id"])]
    for k, p in enumerate(moving[:: max(len(moving) // each, 1)][:each]):  # through reported positions
        add(p["x"], p["y"], p["x"] + (1.5 if k % 2 else -1.5), p["y"] + 0.75)  # from the agent: u == 0
        add(p["x"] - 1.0, p["y"], p["x"] + 1.25, p["y"])  # level with it: c0 == 0
        if k == 0:
            add(p["x"], p["y"], p["x"], p["y"])
    return gates_array(seg, np.array(t0s), np.array(t1s))


def check_crowd(sim, rec, grid, speed_max, name, sel=None, cols=(None, None, None), gates=None, floors=True, seed=7):
    """One query on crowd_gates: the class counts by the restatement ALONE (printed, then asserted non-zero), then the
    engine against it -> (gates, rows, counts)"""
    gates = crowd_gates(rec, grid, seed) if gates is None else gates
    mask = None if sel is None else roles(sel, None, rec, *cols)[0]
    stats = {}
    want = crossings(rec, grid, gates, speed_max, mask, stats=stats)
    print(f"  {name}: restatement alone: {len(gates)} gates, {len(want[0])} rows, {stats}")
    if floors:
        assert min(stats.values()) > 0, stats
    agree(sim, rec, grid, gates, speed_max, sel, cols, name, want=want)
    return gates, want[0], want[1]


@pytest.fixture(scope="module")
def crowd():
    """the walkers of this module, shared by the tests that only ask (each asserts that it left them as they were)"""
    a, rec = walkers()
    yield a, rec
    assert a.read_agents().tobytes() == rec.tobytes()


def test_the_walkers_equal_the_restatement(crowd):
    a, rec = crowd
    for speed_max in (INF, 1.5, 0.0):
        gates, rows, counts = check_crowd(a, rec, GRID, speed_max, f"speed_max {speed_max}", floors=speed_max > 0.0)
        if speed_max == 0.0:
            assert len(rows) == 0
        if speed_max == 1.5:  # (it excludes some agents, by the restatement alone)
            fast = rec["id"][np.hypot(rec["vx"].astype(np.float64), rec["vy"].astype(np.float64)) >= 1.5]
            assert len(fast) > 500 and not np.isin(rows["id"], fast).any() and len(rows) < len(everyone)
        if speed_max == INF:
            everyone = rows
            T = (gates["t1"] - gates["t0"])[rows["gate"].astype(np.int64)]
            assert (rows["s"] < T).all() and not np.signbit(rows["s"]).any() and (rows["u"] >= 0).all() and (rows["u"] < 1).all()
            per_gate = counts.sum(axis=1)
            assert per_gate.max() > 64  # (a gate whose rows take more than one ballot)
            same = (gates["ax"] == gates["bx"]) & (gates["ay"] == gates["by"])
            assert same.sum() == 2 and not per_gate[same].any()  # (A == B: nobody)
            # cap below the count: the prefix and nothing beyond it; out_counts sums to the returned count whatever cap is
            for cap in (1, len(rows) // 2, len(rows) - 1):
                got, per, out = call(a, gates, INF, cap=cap)
                assert got == len(rows) == int(per.sum()) and per.tobytes() == counts.tobytes()
                assert out[:cap].tobytes() == rows[:cap].tobytes() and (out[cap:].view(np.uint8) == 0xAB).all()
            # the Python surface
            got, per = a.gate_crossings(gates, INF)
            assert got.dtype == GATE_CROSSING_DTYPE and got.tobytes() == rows.tobytes()
            assert per.dtype == np.uint64 and per.shape == (len(gates), 2) and per.tobytes() == counts.tobytes()
            got, per = a.gate_crossings(gates, INF, limit=7)
            assert got.tobytes() == rows[:7].tobytes() and per.tobytes() == counts.tobytes()
            assert a.count_gate_crossings(gates, INF).tobytes() == counts.tobytes()
            got, per = a.gate_crossings(gates[:0], 2.0)
            assert got.shape == (0,) and per.shape == (0, 2) and a.count_gate_crossings(gates[:0], 2.0).shape == (0, 2)


@pytest.mark.parametrize("n", [1, 4, 5, 2000])
def test_numbers_of_gates_that_fill_and_do_not_fill_a_workgroup(crowd, n):
    a, rec = crowd
    rng = np.random.default_rng(n)
    c = np.column_stack([rng.uniform(-4.0, 28.0, n), rng.uniform(3.0, 35.0, n)])
    d = rng.uniform(-3.0, 3.0, (n, 2))
    gates = gates_array(np.column_stack([c - d, c + d]), rng.choice([0.0, 0.5], n), 2.5)
    if n <= 5:
        gates[-1] = (-10.0, 19.0, 40.0, 19.5, 0.0, 3.0)  # (the last gate of a workgroup that is not full: a busy one)
    rows, counts = agree(a, rec, GRID, gates, INF, name=f"{n} gates")
    assert counts[-1].sum() > 0 and (n < 2000 or (int(rows["gate"].max()) >= 1990 and len(rows) > 5 * n))


def test_the_crowded_cells_in_steps_of_64_slots(crowd):
    """Doors inside the cells that hold 65, 128 and 129 agents, and lanes through them, with windows long enough for
    everybody who heads that way: the rows of one gate come from two and three 64-slot steps of one run."""
    a, rec = crowd
    seg = []
    for r, c, m in CROWDED:
        x0, y0 = -4.0 + 2.0 * r, 3.0 + 2.0 * c
        seg += [(x0, y0 + 1.0, x0 + 2.0, y0 + 1.0), (x0 + 1.0, y0 + 2.0, x0 + 1.0, y0), (x0, y0, x0 + 2.0, y0 + 2.0),
                (x0 - 6.0, y0 + 0.5, x0 + 8.0, y0 + 1.5)]
    gates = gates_array(seg, 0.0, 4.0)
    rows, counts = agree(a, rec, GRID, gates, INF, name="crowded cells")
    per_gate = counts.sum(axis=1).reshape(3, 4)
    print(f"  rows per gate of the crowded cells: {per_gate.tolist()}")
    assert (per_gate[:, :3] >= 10).all() and per_gate[1:, 3].min() > 64 and (counts > 0).all()
    agree(a, rec, GRID, gates, 1.0, name="crowded cells, the slow")


def test_the_whole_grid_path_and_reaches_of_every_size(crowd):
    """speed_max = +inf with a large t1 (no clip at all), a finite reach that covers the grid, one below a cell, ends
    beyond 2^32 cells, and windows with T == 0."""
    a, rec = crowd
    base = crowd_gates(rec, GRID, seed=9)
    for t1, speed_max in ((1e6, INF), (1e3, 2.0), (40.0, INF), (0.05, 3.0), (1e300, 1e300)):
        gates = base.copy()
        gates["t0"] = np.where(np.arange(len(gates)) % 4 == 0, min(0.5, t1 / 2.0), 0.0)
        gates["t1"] = t1
        stats = {}
        rows, counts = agree(a, rec, GRID, gates, speed_max, stats=stats, name=f"t1 {t1}, speed_max {speed_max}")
        print(f"    {stats}")
        assert stats["left"] > 0 and stats["right"] > 0
    far = gates_array([(-1e13, 10.0, 1e13, 30.0), (12.0, 1e300, 12.5, -1e300), (1e14, 1e14, -1e14, -1e14 + 1.0),
                       (-1.7e308, 20.0, 1.7e308, 20.0), (5.0, -1.7e308, 5.0, 1.7e308)], 0.0, 3.0)
    rows, counts = agree(a, rec, GRID, far, 2.0, name="ends beyond 2^32 cells")
    assert (counts[:2].sum(axis=1) > 20).all()
    still = base.copy()
    still["t1"] = still["t0"]
    assert len(agree(a, rec, GRID, still, INF, name="T == 0")[0]) == 0


def test_agents_written_onto_lines_and_gate_ends_with_dyadic_coordinates():
    """Agents on a 1/8 lattice written with dyadic velocities: everything the rule computes is exact.  Agents on the
    line move off it at s == +0.0 either way, agents at a gate's A are in (u == 0), at its B out, and a chain of gates
    through shared vertices lists a walker once: its rows are those of the one long gate."""
    grid = dict(width=32.0, height=32.0, cell_size=2.0, offset=(-16.0, -16.0))
    xs, ys = np.meshgrid(np.arange(-6.0, 6.0 + 0.125, 0.125), np.arange(-1.0, 1.0 + 0.125, 0.25))
    pts = np.column_stack([xs.ravel(), ys.ravel()])
    a = Simulation(LocationHash2D(**grid))
    a.add_agents(pts, StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 2.0)
    a.step(0.05)
    w = a.read_agents()
    w["x"], w["y"] = pts[:, 0], pts[:, 1]
    vel = np.array([(0.0, 1.0), (0.0, -0.5), (0.25, 0.5), (-0.5, -0.25), (1.0, 0.0), (0.0, 0.0)])[np.arange(len(w)) % 6]
    w["vx"], w["vy"] = vel[:, 0], vel[:, 1]
    a.write_agents(w, fields=("position", "velocity"))
    rec = a.read_agents()
    assert np.array_equal(rec["x"], pts[:, 0]) and np.array_equal(rec["y"], pts[:, 1]) and takes_part(rec, grid).all()
    vertices = [-4.0, -2.5, -2.0, 0.25, 1.0, 4.0]
    chain = path_gates([(v, 0.0) for v in vertices], 0.0, 8.0)
    whole = gates_array([(-4.0, 0.0, 4.0, 0.0)], 0.0, 8.0)
    c_rows, c_counts = agree(a, rec, grid, chain, INF, name="the chain")
    w_rows, w_counts = agree(a, rec, grid, whole, INF, name="the whole gate")
    assert len(np.unique(c_rows["id"])) == len(c_rows) == len(w_rows) > 100  # (no walker twice, nobody lost)
    by_id = c_rows[np.argsort(c_rows["id"], kind="stable")]
    assert (by_id["id"] == w_rows["id"]).all() and (by_id["dir"] == w_rows["dir"]).all()
    assert by_id["s"].tobytes() == w_rows["s"].tobytes() and c_counts.sum(axis=0).tolist() == w_counts.sum(axis=0).tolist()
    on_line = rec["id"][(rec["y"] == 0.0) & (rec["x"] >= -4.0) & (rec["x"] < 4.0) & (rec["vy"] != 0.0)]
    at_zero = w_rows[w_rows["s"] == 0.0]
    assert len(on_line) > 20 and sorted(at_zero["id"].tolist()) == sorted(on_line.tolist())
    assert not at_zero["s"].view(np.uint64).any() and set(at_zero["dir"].tolist()) == {1, -1}  # (+0.0, never -0.0)
    heading = (rec["vx"] == 0.0) & (rec["vy"] != 0.0) & (rec["y"] * rec["vy"] <= 0.0)  # (straight at the line, or on it)
    at_a, at_b = rec["id"][(rec["x"] == -4.0) & heading], rec["id"][(rec["x"] == 4.0) & heading]
    assert len(at_a) > 0 and np.isin(at_a, w_rows["id"]).all() and (w_rows["u"][np.isin(w_rows["id"], at_a)] == 0.0).all()
    assert len(at_b) > 0 and not np.isin(at_b, w_rows["id"]).any()
    # the other winding, windows that open later, and vertical gates on a cell boundary (x == 2) and between two
    more = gates_array([(4.0, 0.0, -4.0, 0.0), (2.0, -1.0, 2.0, 1.0), (2.0, 1.0, 2.0, -1.0), (2.125, -1.0, 2.125, 0.5),
                        (-5.0, -0.5, 5.0, -0.5), (-6.0, -1.0, 6.0, 1.0)], [0.0, 0.0, 0.5, 0.25, 1.0, 0.0], 8.0)
    rows, counts = agree(a, rec, grid, more, INF, name="windings, later windows, a cell boundary")
    assert (counts.sum(axis=1) > 0).all()
    # the other winding swaps the sides, keeps s, and is half-open at the other end: the walkers through x == -4 are the
    # first winding's alone (u == 0 there, u == 1 here), those through x == 4 this one's alone
    back = rows[rows["gate"] == 0]
    both = np.intersect1d(back["id"], w_rows["id"])
    b, f = back[np.isin(back["id"], both)], w_rows[np.isin(w_rows["id"], both)]
    assert len(both) > 100 and (b["dir"] == -f["dir"]).all() and b["s"].tobytes() == f["s"].tobytes()
    only_f, only_b = w_rows[~np.isin(w_rows["id"], both)], back[~np.isin(back["id"], both)]
    assert len(only_f) > 0 and (only_f["u"] == 0.0).all() and len(only_b) > 0 and (only_b["u"] == 0.0).all()
    assert np.isin(at_a, only_f["id"]).all() and np.isin(at_b, only_b["id"]).all()
    agree(a, rec, grid, np.concatenate([chain, whole, more]), 0.75, name="the slower ones")


def test_filters_by_rect_planner_and_speed():
    a, led, sinks, grid = _scene(sinks=True)
    _advance(a, led, 40)
    rec = a.read_agents()
    cols = led.columns(rec)
    speed = np.hypot(rec["vx"].astype(np.float64), rec["vy"].astype(np.float64))
    sels = [("a rectangle", selection(_abi.CS_SEL_RECT, x0=-INF, y0=-INF, x1=float(np.median(rec["x"])), y1=INF)),
            ("a planner", selection(_abi.CS_SEL_HLP, hlp=int(np.bincount(np.asarray(cols[1]).astype(np.int64)).argmax()))),
            ("the slower half", selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=float(np.median(speed)))),
            ("nobody", selection(_abi.CS_SEL_LP, lp=12345))]
    gates, everyone, _ = check_crowd(a, rec, grid, 2.0, "no filter", floors=False)
    keys = set(zip(everyone["gate"].tolist(), everyone["id"].tolist()))
    for name, sel in sels:
        _, rows, counts = check_crowd(a, rec, grid, 2.0, name, sel=sel, cols=cols, gates=gates, floors=False)
        allowed = rec["id"][roles(sel, None, rec, *cols)[0]]
        assert np.isin(rows["id"], allowed).all() and set(zip(rows["gate"].tolist(), rows["id"].tolist())) <= keys
        assert (len(rows) == 0 and not counts.any()) if name == "nobody" else 0 < len(rows) < len(everyone)
    x1 = float(np.median(rec["x"]))
    want = crossings(rec, grid, gates, 2.0, roles(sels[0][1], None, rec, *cols)[0])
    got, per = a.gate_crossings(gates, 2.0, filter=dict(rect=(-INF, -INF, x1, INF)))
    assert got.tobytes() == want[0].tobytes() and per.tobytes() == want[1].tobytes()
    assert a.count_gate_crossings(gates, 2.0, Selection(rect=(-INF, -INF, x1, INF))).tobytes() == want[1].tobytes()
    assert a.read_agents().tobytes() == rec.tobytes()


@pytest.mark.parametrize("flags", [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER])
def test_between_steps_after_a_step_and_after_removals(flags):
    a, led, _, grid = _scene(flags, 1024)
    _advance(a, led, 30)
    rec = a.read_agents()
    gates, rows, _ = check_crowd(a, rec, grid, 2.0, f"flags {flags}, 30 steps in")
    _advance(a, led, 1)
    check_crowd(a, a.read_agents(), grid, INF, f"flags {flags}, a step later")  # (gates through the new positions)
    a.remove_agents_by_id(rec["id"][::3].tolist())
    left = a.read_agents()
    assert len(left) == len(rec) - len(rec[::3])
    _, rows, _ = check_crowd(a, left, grid, 2.0, f"flags {flags}, a third removed", gates=gates, floors=False)
    assert len(rows) >= 100 and not np.isin(rows["id"], rec["id"][::3]).any()
    _advance(a, led, 5)
    check_crowd(a, a.read_agents(), grid, 2.0, f"flags {flags}, five steps later", gates=gates, floors=False)


def test_refusals(crowd):
    a, rec = crowd
    good = gates_array([(-10.0, 19.0, 40.0, 19.5)] * 6, 0.0, 3.0)
    usable, counts = agree(a, rec, GRID, good, 2.0, name="six busy gates")
    assert len(usable) > 60
    cap = len(usable)
    nan = float("nan")

    def bad(field, value, k=3):
        gates = good.copy()
        gates[field][k] = value
        return gates

    bad_terms = selection(1 << 9)
    nan_rect = selection(_abi.CS_SEL_RECT, x0=nan, y0=0.0, x1=1.0, y1=1.0)
    cases = [("NaN speed_max", good, dict(speed_max=nan), "speed_max is NaN or negative"),
             ("negative speed_max", good, dict(speed_max=-1e-300), "speed_max is NaN or negative"),
             ("too many gates", good, dict(n=_abi.CS_GATES_MAX + 1), "more gates than CS_GATES_MAX"),
             ("null gates", good, dict(null_gates=True), "null gates"),
             ("unknown terms", good, dict(sel=bad_terms), "gate_crossings"), ("a NaN in the filter", good, dict(sel=nan_rect), "gate_crossings")]
    for field in ("ax", "ay", "bx", "by"):
        cases += [(f"{field} {v}", bad(field, v), {}, "gate 3: its ends are not finite") for v in (nan, INF, -INF)]
    for field in ("t0", "t1"):
        cases += [(f"{field} {v}", bad(field, v), {}, "gate 3: its times are not finite") for v in (nan, INF, -INF)]
    cases += [("negative t0", bad("t0", -1e-300), {}, "gate 3: its t0 is negative"),
              ("t1 before t0", bad("t0", 11.0), {}, "gate 3: its t1 is before its t0")]
    for name, gates, kw, text in cases:
        kw = dict(kw)
        speed_max = kw.pop("speed_max", 2.0)
        for c in (cap, 0):
            got, per, out = call(a, gates, speed_max, cap=c, **kw)
            assert got == SIZE_MAX and last_error(a).startswith("gate_crossings") and text in last_error(a), (name, last_error(a))
            assert (out.view(np.uint8) == 0xAB).all() and (per.view(np.uint8) == 0xAB).all(), name  # (nothing written)
        assert a.read_agents().tobytes() == rec.tobytes(), name
        assert call(a, good, 2.0, cap=cap)[2][:cap].tobytes() == usable.tobytes(), name
    two = bad("bx", nan, 5)
    two["t1"][2] = -1.0
    assert call(a, two, 2.0, cap=12)[0] == SIZE_MAX and "gate 2" in last_error(a)  # (the first bad gate)
    assert a._lib.cs_gate_crossings(a._engine, None, 0, 2.0, None, None, None, 0) == 0  # no gates: nothing to do
    agree(a, rec, GRID, bad("t1", 0.0), 2.0, name="t1 == t0 == 0 is admitted")
    agree(a, rec, GRID, bad("bx", -10.0), INF, name="a gate that is nearly A == B, and +inf, are admitted")
    with pytest.raises(CrowdSimError, match="gate_crossings: gate 0"):
        a.gate_crossings(gates_array([(1.0, 4.0, 2.0, 4.0)], 2.0, 1.0), 2.0)
    with pytest.raises(CrowdSimError, match="gate_crossings"):
        a.count_gate_crossings(good, 2.0, filter=dict(circle=(0.0, 0.0, -2.0)))
    with pytest.raises(CrowdSimError, match="gate_crossings"):
        a.gate_crossings(good, -1.0)
    assert a.gate_crossings(good, 2.0)[0].tobytes() == usable.tobytes()


def test_a_total_beyond_the_list_limit_is_counted_and_not_listed(crowd):
    """2^20 copies of a lane that more than 64 walkers cross: more than CS_PAIRS_MAX rows.  The count-only form gives
    them exactly; a listing is refused, writes nothing and leaves the engine usable."""
    a, rec = crowd
    lane = gates_array([(-10.0, 19.0, 40.0, 19.5)], 0.0, 3.0)
    one = int(a.count_gate_crossings(lane, 3.0).sum())
    assert one > 64
    gates = np.repeat(lane, _abi.CS_GATES_MAX)
    got, per, none = call(a, gates, 3.0, rows=False)
    assert got == one * 2 ** 20 > _abi.CS_PAIRS_MAX and none is None and (per.sum(axis=1) == one).all()
    got, per, out = call(a, gates, 3.0, cap=3)
    assert got == SIZE_MAX and "too many crossings to list" in last_error(a)
    assert (out.view(np.uint8) == 0xAB).all() and (per.view(np.uint8) == 0xAB).all()
    with pytest.raises(CrowdSimError, match="too many crossings to list"):
        a.gate_crossings(gates, 3.0)
    check_crowd(a, rec, GRID, 2.0, "after the refusal")


def test_wide_ids_by_external_id(monkeypatch):
    """Ids above 2^32 come back in ascending order, before and after a renumbering."""
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(2 ** 40 + 1))
    monkeypatch.setenv("CS_DEVICE_ID_LIMIT", "4096")
    a, rec = walkers(n=600, crowded=(), flags=CS_CFG_WIDE_IDS)
    monkeypatch.delenv("CS_DEVICE_ID_LIMIT")
    monkeypatch.delenv("CS_FIRST_AGENT_ID")
    assert int(rec["id"].min()) > 2 ** 40
    spot = np.array([[20.0, 30.0]])
    still, nolp = StubHighLevelPlan((0.0, 0.0)), NoLocalPlan()
    for r in range(6):
        more = a.add_agents(np.repeat(spot, 600, axis=0) + np.arange(600)[:, None] * 0.001, still, nolp, 1.0)
        a.step(0.05)  # (everybody stands again: the plan says so)
        if r in (0, 5):
            n_before = a.kernel_stat(_abi.CS_STAT_RENUMBERINGS)
            rec = randomize(a, 40 + r)
            _, rows, _ = check_crowd(a, rec, GRID, 2.0, f"round {r}, {n_before} renumberings")
            assert len(rows) >= 100 and int(rows["id"].min()) > 2 ** 32
            assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) == n_before
        a.remove_agents_by_id(more[:-1])
    assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) >= 1
    check_crowd(a, randomize(a, 50), GRID, 2.0, "at the end")


def test_an_odd_cell_grid():
    """the 0.7 m cells of tests/odd_grids.py, whose origin is no multiple of the cell"""
    import odd_grids as og
    sc = og.scene("odd-cell")
    a = og.stepped(sc, lambda g: Simulation(LocationHash2D(**g)))
    rec = a.read_agents()
    for speed_max, t1 in ((INF, 2.0), (1.0, 6.0)):
        _, rows, _ = check_crowd(a, rec, sc.grid, speed_max, f"odd-cell, speed_max {speed_max}", floors=False,
                                 gates=crowd_gates(rec, sc.grid, t1=t1))
        assert len(rows) >= 100 and {1, -1} <= set(rows["dir"].tolist()) and (rows["s"] == 0.0).any()
    assert a.read_agents().tobytes() == rec.tobytes()


@pytest.mark.parametrize("flags", [0, CS_CFG_FORCE_TILED])
def test_twins_one_of_which_asks_between_steps(flags):
    """One twin asks after every step from 20 to 30, the other never does: the same bytes, events and report."""
    twins = [_scene(flags, 4096, sinks=True) for _ in range(2)]
    (a, led_a, _, grid), (b, led_b, _, _) = twins
    for s, led, _, _ in twins:
        _advance(s, led, 20)
    rec = a.read_agents()
    assert rec.tobytes() == b.read_agents().tobytes()
    gates = crowd_gates(rec, grid)
    for _ in range(10):
        assert 0 < int(a.count_gate_crossings(gates, 2.0).sum())
        assert len(a.gate_crossings(gates, INF, filter=dict(source_sink=0), limit=50)[0]) <= 50
        assert len(a.gate_crossings(gates, INF, limit=50)[0]) == 50
        _steps((a, b), 1)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert drain(a) == drain(b)
    assert a.last_report == b.last_report


def test_a_tile_that_holds_ghosts_answers_for_the_agents_it_owns():
    """The engines of a 2 x 2 mesh whose ghost rings are unpacked (tests/odd_grids.py): each is asked gates along and
    across its owned edges; it answers for the agents it owns, and the rows of the four together are the single
    engine's."""
    import odd_grids as og
    case = og.GHOST_CASES[0]
    sc, (mesh,), single, rec, rects, held, _ = og.ghost_state(case)
    with og.released(single, *mesh.engines):
        cell = sc.cell
        ox, oy = sc.grid["offset"]
        gates = [crowd_gates(rec, sc.grid, each=25, t1=3.0)]
        for x0, x1, y0, y1 in np.asarray(rects, dtype=np.int64).tolist():
            for axis, inner, outer in og.cut_sides(sc, (x0, x1, y0, y1)):
                edge = max(inner, outer)
                if axis == 0:
                    seg = [(ox + edge * cell, oy + y0 * cell, ox + edge * cell, oy + y1 * cell),  # along the cut
                           (ox + (edge + 0.5) * cell, oy + y1 * cell, ox + (edge + 0.5) * cell, oy + y0 * cell),
                           (ox + (edge - 0.5) * cell, oy + y0 * cell, ox + (edge - 0.5) * cell, oy + y1 * cell)]
                else:
                    seg = [(ox + x0 * cell, oy + edge * cell, ox + x1 * cell, oy + edge * cell),
                           (ox + x1 * cell, oy + (edge + 0.5) * cell, ox + x0 * cell, oy + (edge + 0.5) * cell),
                           (ox + x0 * cell, oy + (edge - 0.5) * cell, ox + x1 * cell, oy + (edge - 0.5) * cell)]
                gates.append(gates_array(seg, 0.0, 3.0))
        gates = np.concatenate(gates)
        whole, whole_counts = agree(single, rec, sc.grid, gates, INF, name="the single engine")
        parts, total, with_ghosts = [], np.zeros((len(gates), 2), dtype=np.uint64), 0
        for k, (engine, (own, ghosts)) in enumerate(zip(mesh.engines, held)):
            rows, per = agree(engine, own, sc.grid, gates, INF, name=f"tile {k}: {len(own)} owned, {len(ghosts)} ghosts")
            both = crossings(og._join(own, ghosts), sc.grid, gates, INF)[0]  # what an engine that listed its ghosts would say
            with_ghosts += len(both) - len(rows)
            assert len(both) > len(rows) and not np.isin(rows["id"], ghosts["id"]).any()
            parts.append(rows)
            total += per
        print(f"{with_ghosts} rows would be ghosts'")
        merged = np.concatenate(parts)
        merged = merged[np.lexsort((merged["id"], merged["gate"]))]
        assert merged.tobytes() == whole.tobytes() and total.tobytes() == whole_counts.tobytes()
