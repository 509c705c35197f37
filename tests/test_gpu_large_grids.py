"""Large, sparse and one-sided grids against the f64 oracle, up to the 31-bit cell limit.  Needs an MI355X.

Every other oracle comparison runs on a grid a margin wider than a dense crowd: the one-launch cell scan
(`k_scan_onepass`, at most 1,024 scan tiles of 1,024 cells), band windows within the builder's LDS column prefix,
coordinates of a few hundred metres.  Here a few thousand agents stand in clusters on grids of up to 16.8M cells (the
oracle keeps a std::set per cell: that is its ceiling), and on grids one cell wide or one cell high; beyond that the
engine is compared with itself, by whole-cell translation into the top corner of a grid just under 2^31 cells.

Scenes are laid out in cells of 1 m.  The engine's (and the reference's) flat cell index is x_row * nx + y_col with
nx = width / cell (location_hash_2d.rs:54-66): x runs over the grid's ny rows, y over one row's nx cells.  The clusters
sit on the first and the last cell of the grid and across scan-tile boundaries (flat indices k * 1,024 - 1 | k * 1,024),
and walk along y, i.e. along the flat index, through those boundaries.  A cell_start that is off in one such tile, a
dropped partial tile or a window cut or sized wrongly changes whom some agent sees, and the step's result.

Tolerances are the project's: ids, reports, errors and neighbour lists exact; positions within 1e-4 of L, with L = 10 m,
the extent of one cluster (the grid's extent would allow metres); engine runs of different kernels, scans or grids
bitwise equal.
"""
import numpy as np
import pytest

from oracle_sim import OracleSimulation
from rmf_crowdsim_amd import (CrowdSimError, LocationHash2D, NoHighLevelPlan, NoLocalPlan, Simulation,
                              StubHighLevelPlan, Zanlungo, _abi)
from test_gpu_parity import max_rel_err

pytestmark = pytest.mark.gpu

LP = Zanlungo(0.05, 1.0, 0.0, 0.4, 2.0, 0.2)  # (the batch-query test's model: forces act, nobody is thrown)
SCAN_TILE = 1024
L = 10.0
DT, STEPS = 0.1, 30
WALK = 0.4  # m/s along y: 1.2 m in STEPS steps, across a cell boundary for everybody


def _grid(nx, ny, offset=(0.0, 0.0)):
    return dict(width=float(nx), height=float(ny), cell_size=1.0, offset=offset)


def _cluster(cx, cy, nx, ny, rows, cols, spacing, seed, margin=0.0):
    """rows x cols jittered lattice centred on (cx, cy) (x: the grid's rows, y: a row's cells; spacing (sx, sy)); points
    outside the grid (or closer than `margin` to its high edges, for walkers) dropped.  Positions are multiples of
    2^-16 m: exact in a cell-relative f32 offset, and in f64 after a shift by whole cells.  -> (points, row, column)"""
    sx, sy = spacing
    k = np.arange(rows * cols)
    rng = np.random.default_rng(seed)
    x = cx + ((k // cols) - (rows - 1) / 2.0) * sx + rng.uniform(-0.2, 0.2, k.size) * sx
    y = cy + ((k % cols) - (cols - 1) / 2.0) * sy + rng.uniform(-0.2, 0.2, k.size) * sy
    p = np.round(np.stack([x, y], axis=1) * 65536.0) / 65536.0
    keep = (p[:, 0] > 0.05) & (p[:, 0] < ny - 0.05 - margin) & (p[:, 1] > 0.05) & (p[:, 1] < nx - 0.05 - margin)
    return p[keep], (k // cols)[keep], (k % cols)[keep]


def _centre(flat, nx):
    return flat // nx + 0.5, flat % nx + 0.5


def tile_crowd(nx, ny, tiles=(), seed=3):
    """Walkers in 10 x 10 clusters across the given scan-tile boundaries and at the middle of the grid (n_slots >= 2048,
    the tiled kernel's condition), standing clusters on the first and the last cell.  A cluster is a set of lanes
    along y, 0.7 m apart, of walkers 1 m apart; fast and slow walkers alternate in a lane, so that the fast ones catch up
    and the model turns them aside (their paths come within the 0.2 m collision distance).
    -> ((fast, slow walkers), standers)."""
    ncells = nx * ny
    n_tiles = -(-ncells // SCAN_TILE)
    ks = sorted(set(int(k) for k in tiles if 0 < k < n_tiles) | {1, 2, 3, n_tiles - 1, n_tiles // 2})
    anchors = [_centre(k * SCAN_TILE, nx) for k in ks] + [_centre(ncells // 2, nx)]
    anchors += [_centre(ncells // 3 + 40 * j, nx) for j in range(40)]  # (a row of clusters: enough agents)
    fast, slow, taken = [], [], []
    for j, (cx, cy) in enumerate(anchors):
        if any(abs(cx - ax) < 7.0 and abs(cy - ay) < 10.0 for ax, ay in taken):
            continue  # the cluster that is there covers it
        taken.append((cx, cy))
        p, a, b = _cluster(cx, cy, nx, ny, 10, 8, (0.7, 1.0), seed + j, margin=2.0)
        clear = (p[:, 0] > 1.6) | (p[:, 1] > 2.2)  # (nobody inside, or walking into, the standers of the first cell)
        p, a, b = p[clear], a[clear], b[clear]
        fast.append(p[(a + b) % 2 == 0])
        slow.append(p[(a + b) % 2 == 1])
    standers = [_cluster(0.5, 0.5, nx, ny, 4, 4, (0.6, 0.6), seed + 100)[0],
                _cluster(ny - 0.5, nx - 0.5, nx, ny, 4, 4, (0.6, 0.6), seed + 101)[0]]
    return (np.concatenate(fast), np.concatenate(slow)), np.concatenate(standers)


def _populate(sim, walkers, standers, shift=0.0):
    sim.add_agents(walkers[0] + shift, StubHighLevelPlan((0.0, WALK)), LP, 1.0)
    sim.add_agents(walkers[1] + shift, StubHighLevelPlan((0.0, 0.8 * WALK)), LP, 1.0)
    sim.add_agents(standers + shift, NoHighLevelPlan(), LP, 1.0)


def _forces_act(agents, walkers):
    """The share of walkers whose velocity is not the one their planner asked for."""
    n0, n1 = len(walkers[0]), len(walkers[1])
    want = np.concatenate([np.full(n0, WALK), np.full(n1, 0.8 * WALK)])
    speed = np.hypot(agents["vx"][: n0 + n1], agents["vy"][: n0 + n1])
    return float((np.abs(speed - want) > 1e-6).mean())


def _run(sim, steps, report=True):
    reports = []
    for _ in range(steps):
        sim.step(DT, report=report)
        reports.append(dict(sim.last_report) if report else None)
    return sim.read_agents(), reports


def _leave_high_edge(sim, nx, ny):
    """A walker in the grid's last cell heading +x: it leaves through the high edge in the 4th step
    (location_hash_2d.rs:61-63); the step fails and commits nothing.  -> (failing step, error, agents after)."""
    sim.add_agents([(ny - 0.375, nx - 0.5)], StubHighLevelPlan((1.0, 0.0)), NoLocalPlan(), 1.0)
    for k in range(10):
        try:
            sim.step(DT)
        except CrowdSimError as e:
            return k, str(e), sim.read_agents()
    return None, None, sim.read_agents()


def _engine(grid, flags, monkeypatch, onepass=None):
    if onepass is None:
        monkeypatch.delenv("CS_SCAN_ONEPASS", raising=False)
    else:
        monkeypatch.setenv("CS_SCAN_ONEPASS", onepass)
    return Simulation(LocationHash2D(**grid), flags=flags)


def _variants(ncells):
    one = [None, "0"] if -(-ncells // SCAN_TILE) <= 1024 else [None]
    return [(f, o) for o in one for f in (_abi.CS_CFG_DEFAULT, _abi.CS_CFG_FORCE_GATHER)]


def _compare_with_oracle(nx, ny, walkers, standers, monkeypatch, failure=True):
    grid = _grid(nx, ny)
    ora = OracleSimulation(LocationHash2D(**grid))
    _populate(ora, walkers, standers)
    want, want_rep = _run(ora, STEPS)
    want_fail = _leave_high_edge(ora, nx, ny) if failure else None
    ora.close()
    assert np.isfinite(want["x"]).all() and np.isfinite(want["y"]).all()
    ref = None
    for flags, onepass in _variants(nx * ny):
        sim = _engine(grid, flags, monkeypatch, onepass)
        _populate(sim, walkers, standers)
        got, got_rep = _run(sim, STEPS)
        assert got_rep == want_rep, (flags, onepass)
        err = max_rel_err(got, want, L)
        assert err <= 1e-4, (flags, onepass, err)
        if ref is None:
            ref = got
        assert got.tobytes() == ref.tobytes(), (flags, onepass)
        if failure:
            k, msg, after = _leave_high_edge(sim, nx, ny)
            assert (k, msg) == want_fail[:2] and k == 3 and "Index out of bounds" in msg
            assert max_rel_err(after, want_fail[2], L) <= 1e-4
        sim.close()
    assert _forces_act(want, walkers) > 0.1 and want_rep[-1]["n_tti_zero"] == 0
    print(f"{nx} x {ny} = {nx * ny:,} cells, {len(want)} agents: |dp|/L = {err:.2e}")


# ---- 1. scan-tile boundaries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [
    (1024, 1024),   # 1,048,576 cells: the last one-launch grid, 1,024 full tiles
    (61681, 17),    # 1,048,577 = 17 * 61,681: the first two-launch grid, one cell in its last tile
    (1023, 1025),   # 1,048,575 = 1,023 (mod 1,024) and 3 (mod 4): one-launch, the last tile one cell short
    (1022, 1023),   # 1,045,506 = 2 (mod 4): the scalar tail of the uint4 path
    (1025, 1025),   # 1,050,625 = 1 (mod 1,024): two launches, a last tile of one cell
    (4097, 4097),   # 16,785,409 cells = 1 (mod 1,024): 16,393 tiles
], ids=["2^20", "2^20+1", "2^20-1", "mod4=2", "mod1024=1", "16.8M"])
def test_scan_tile_boundaries_match_the_oracle(nx, ny, monkeypatch):
    """Both step kernels and, where the one-launch scan applies, both scans, against the oracle: 30 steps of
    walkers crossing scan-tile boundaries, the per-step reports, and the step in which a walker in the last cell
    leaves the grid through its high edge."""
    n_tiles = -(-nx * ny // SCAN_TILE)
    walkers, standers = tile_crowd(nx, ny, tiles=(n_tiles // 3, n_tiles - 2, 1023, 1024, 1025))
    assert len(walkers[0]) + len(walkers[1]) + len(standers) >= 2048
    _compare_with_oracle(nx, ny, walkers, standers, monkeypatch)


# ---- 2. one-sided grids --------------------------------------------------------------------------------------------
def _line_crowd(nx, ny, n_agents, seed):
    """Clusters spread along the long side of a grid only a few cells across, n_agents or more: files 1 m apart along
    the long side, lanes 0.7 m apart across it, fast and slow walkers alternating in a lane (tile_crowd).
    -> ((fast, slow), along_x)"""
    along_x = ny > nx
    length, width = (ny, nx) if along_x else (nx, ny)
    lanes = max(1, int(width / 0.7))
    n_clusters = -(-n_agents // (12 * lanes))
    fast, slow = [], []
    for j in range(n_clusters):
        c = 8.0 + (length - 16.0) * j / max(n_clusters - 1, 1)
        if along_x:
            p, a, b = _cluster(c, width / 2.0, nx, ny, 12, lanes, (1.0, 0.7), seed + j)
        else:
            p, a, b = _cluster(width / 2.0, c, nx, ny, lanes, 12, (0.7, 1.0), seed + j)
        fast.append(p[(a + b) % 2 == 0])
        slow.append(p[(a + b) % 2 == 1])
    return (np.concatenate(fast), np.concatenate(slow)), along_x


def _one_sided(cls, nx, ny, walkers, along_x, flags=0):
    grid = LocationHash2D(**_grid(nx, ny))
    sim = cls(grid) if cls is OracleSimulation else cls(grid, flags=flags)
    for pts, v in zip(walkers, (WALK, 0.8 * WALK)):
        sim.add_agents(pts, StubHighLevelPlan((v, 0.0) if along_x else (0.0, v)), LP, 1.0)
    return sim


def _query_points(pts, seed):
    rng = np.random.default_rng(seed)
    q = pts[rng.choice(len(pts), 60, replace=False)] + rng.uniform(-0.8, 0.8, (60, 2))
    return q, rng.choice([0.3, 1.0, 2.5], 60)


def _radius_queries(sim, q, radii):
    return sim.query_radius_batch(radii, q), [sim.get_neighbours_in_radius(radii[i], q[i]) for i in range(len(q))]


def _knn_ok(got, agents, p, k):
    """The engine's k-NN is exact (nearest first, ties by id: cs_query_knn), where the reference's ring search is not
    (location_hash_2d.rs:151-238 stops as soon as it holds k candidates): compared with the exact answer over the
    oracle's f64 positions.  Agents equally far to f32 rounding may come in either order."""
    d = np.hypot(agents["x"] - p[0], agents["y"] - p[1])
    want = [int(v) for v in agents["id"][np.lexsort((agents["id"], d))[:k]]]
    if got == want:
        return True
    dist = dict(zip(agents["id"].tolist(), d.tolist()))
    return sorted(got) == sorted(want) and np.allclose([dist[v] for v in got], [dist[v] for v in want], rtol=1e-5)


def _check_knn(sim, agents, q, k, singles=None):
    """Batch k-NN of every point and the single query of the first `singles` points (all: None) against _knn_ok."""
    batch = sim.query_knn_batch(k, q)
    for i, p in enumerate(q):
        assert _knn_ok(batch[i], agents, p, k), (i, batch[i])
        if singles is None or i < singles:
            got = sim.get_nearest_neighbours(k, p)
            assert _knn_ok(got, agents, p, k), (i, got)


@pytest.mark.parametrize("nx,ny", [(1, 2_000_003), (2_000_003, 1), (4, 200_000), (5, 200_000)],
                         ids=["corridor", "strip", "nx=4", "nx=5"])
def test_one_sided_grids_match_the_oracle(nx, ny):
    """A corridor one cell wide (2M rows), a strip one cell high (2M cells in its one row: far beyond the builder's
    LDS column prefix, windows cut by the fixed-point column bound), and grids of 4 and 5 cells a row, either side of
    the tiled kernel's nx >= 3h + 2.  Step, radius and batch queries equal the oracle's, k-NN the exact answer.
    (The corridor's single radius query measured distances from a reference row clamped into the first nx rows,
    i.e. from up to 2,000 km away, and listed an agent outside the radius.)"""
    walkers, along_x = _line_crowd(nx, ny, 2100, 11)
    assert len(walkers[0]) + len(walkers[1]) >= 2048
    ora = _one_sided(OracleSimulation, nx, ny, walkers, along_x)
    want, want_rep = _run(ora, STEPS)
    q, radii = _query_points(np.stack([want["x"], want["y"]], axis=1), 5)
    want_q = _radius_queries(ora, q, radii)
    ora.close()
    ref = None
    for flags in (_abi.CS_CFG_DEFAULT, _abi.CS_CFG_FORCE_GATHER):
        sim = _one_sided(Simulation, nx, ny, walkers, along_x, flags)
        got, got_rep = _run(sim, STEPS)
        assert got_rep == want_rep
        assert max_rel_err(got, want, L) <= 1e-4
        got_q = _radius_queries(sim, q, radii)
        assert got_q[0] == want_q[0] and got_q[1] == want_q[1]
        _check_knn(sim, want, q[:30], 6)
        if ref is None:
            ref = got
        assert got.tobytes() == ref.tobytes()
        sim.close()
    assert _forces_act(want, walkers) > 0.1 and want_rep[-1]["n_tti_zero"] == 0


# ---- 3. queries and read-back far from the origin --------------------------------------------------------------------
@pytest.mark.parametrize("offset", [(0.0, 0.0), (-30000.0, 45000.0)], ids=["origin", "offset"])
def test_queries_and_read_back_far_from_the_origin(offset):
    """The 16.8M-cell grid with 4 m cells (16 km a side; with the offset the crowd stands some 50 km from the origin):
    radius and batch queries equal the oracle's lists exactly, in its order; k-NN queries the exact answer, including
    one in empty space that doubles its radius across hundreds of cells towards an isolated agent (k larger than the
    crowd, a search of the whole grid here, is asked on the crowd at the cell limit);
    read_agents and a snapshot frame give the oracle's f64 positions."""
    n = 4097
    cell = 4.0
    grid = dict(width=n * cell, height=n * cell, cell_size=cell, offset=offset)
    walkers, standers = tile_crowd(n, n)
    lone = np.array([[3000.5, 1000.5], [4096.875, 0.125]])  # (cells) one isolated agent, one in the corner cell
    o = np.array(offset)
    pts = np.concatenate([walkers[0], walkers[1], standers, lone]) * cell + o
    sims = {}
    for cls in (OracleSimulation, Simulation):
        sim = cls(LocationHash2D(**grid))
        for part, v in ((walkers[0], WALK), (walkers[1], -WALK), (np.concatenate([standers, lone]), 0.0)):
            sim.add_agents(part * cell + o, StubHighLevelPlan((0.0, v)), LP, cell)
        start = sim.read_agents()
        assert np.array_equal(start["x"], pts[:, 0]) and np.array_equal(start["y"], pts[:, 1])  # dyadic: exact
        _run(sim, 10)
        sims[cls] = sim
    ora, sim = sims[OracleSimulation], sims[Simulation]
    a, b = sim.read_agents(), ora.read_agents()
    assert max_rel_err(a, b, L * cell) <= 1e-4
    sim.request_snapshot()
    frame = np.sort(sim.snapshot(wait=True)[0].copy(), order="id")
    assert (frame["id"] == a["id"]).all() and np.array_equal(frame["x"], a["x"]) and np.array_equal(frame["y"], a["y"])
    far = [np.array(p) * cell + o for p in ((3000.5, 400.5), (2000.0, 1000.0), (10.0, 4000.0), (4096.5, 4096.5),
                                           (-50.0, -50.0), (5000.0, 2000.0))]
    near = [np.array([b["x"][i], b["y"][i]]) + 0.3 for i in range(0, len(b), len(b) // 25)]
    qs = np.array(far + near)
    radii = np.array([3.0, 9.0, 30.0] * (len(qs) // 3 + 1))[: len(qs)]
    assert sim.query_radius_batch(radii, qs) == ora.query_radius_batch(radii, qs)
    for q, r in zip(qs, radii):
        assert sim.get_neighbours_in_radius(r, q) == ora.get_neighbours_in_radius(r, q)
    for k in (1, 3, 17):  # (near the crowd, and from empty space 600 cells from the isolated agent: batch only)
        _check_knn(sim, b, np.array(near + [far[0]]), k, singles=4)
    lone_id = int(b["id"][-2])
    assert ora.get_nearest_neighbours(1, far[0]) == [lone_id]  # (600 cells of empty space to it)
    assert sim.get_nearest_neighbours(1, far[0]) == [lone_id]
    sim.close()
    ora.close()


# ---- 4. at the 31-bit cell limit, by whole-cell translation ---------------------------------------------------------
BIG = 46340  # 46,340^2 = 2,147,395,600 cells: 88,047 under 2^31 - 1


def test_the_31_bit_cell_limit_is_where_cs_create_says():
    """cs_create refuses gnx * gny >= 2^31 - 1 (crowdstep_hip.hip: a flat cell index and the index one past the
    last are 31-bit) and takes one cell fewer.  2^31 - 1 is prime: 1 x (2^31 - 1) is the only grid of that size."""
    with pytest.raises(CrowdSimError, match="grid too large for 32-bit cell indices"):
        Simulation(LocationHash2D(1.0, float(2 ** 31 - 1), 1.0, (0.0, 0.0)))
    sim = Simulation(LocationHash2D(1.0, float(2 ** 31 - 2), 1.0, (0.0, 0.0)))
    sim.add_agents([(0.5, 0.5), (2 ** 31 - 2.5, 0.5)], StubHighLevelPlan((0.5, 0.0)), NoLocalPlan(), 1.0)
    sim.step(0.25)
    a = sim.read_agents()
    assert a["id"].tolist() == [0, 1] and a["x"].tolist() == [0.625, 2 ** 31 - 2.375]
    sim.close()


def test_a_crowd_shifted_into_the_top_corner_of_a_grid_at_the_limit_steps_alike():
    """Cell-relative arithmetic does not depend on which cell an agent stands in: a crowd on a 64 x 64 grid (checked
    against the oracle) and the same crowd shifted by 46,276 whole cells on both axes into the top corner of a
    46,340 x 46,340 grid (high edges coincide) give the same velocities, ids and reports bit for bit and positions
    equal to the shifted ones to the last bit of the f64 read-back, fail in the same step on the same walker, and
    answer the same radius and k-NN queries (one with k larger than the crowd).  Device memory: five (ncells + 1) x 4 B tables, 43 GB.
    Measured on an MI355X: 14 ms a step on the large grid (515 ms before the block offsets of the two-launch scan were
    computed by one linear pass, k_scan_bases)."""
    w = 64
    shift = float(BIG - w)
    p, a, b = _cluster(30.0, 30.0, w, w, 80, 56, (0.7, 1.0), 21, margin=2.0)  # 56 m x 56 m of lanes
    walkers = (p[(a + b) % 2 == 0], p[(a + b) % 2 == 1])
    standers = np.concatenate([_cluster(0.5, 0.5, w, w, 4, 4, (0.6, 0.6), 22)[0],
                               _cluster(w - 0.5, w - 0.5, w, w, 4, 4, (0.6, 0.6), 23)[0]])
    assert len(walkers[0]) + len(walkers[1]) + len(standers) >= 2048
    runs = {}
    for name, cls, n, d in (("oracle", OracleSimulation, w, 0.0), ("small", Simulation, w, 0.0),
                            ("big", Simulation, BIG, shift)):
        sim = cls(LocationHash2D(**_grid(n, n)))
        _populate(sim, walkers, standers, shift=d)
        got, rep = _run(sim, 4)
        q = np.array([[20.3, 30.7], [40.1, 2.2], [63.5, 63.5], [0.2, 10.0]]) + d
        queries = ([sim.get_neighbours_in_radius(r, p) for p in q for r in (0.8, 2.5)],
                   [sim.get_nearest_neighbours(k, p) for p in q for k in (1, 5)],
                   sim.query_knn_batch(len(got) + 10, q[:2]) if cls is Simulation else None)  # (everybody)
        fail = _leave_high_edge(sim, n, n)
        runs[name] = (got, rep, queries, fail)
        sim.close()
    (o, orep, oq, ofail), (s, srep, sq, sfail), (g, grep, gq, gfail) = runs["oracle"], runs["small"], runs["big"]
    assert srep == orep and sq[0] == oq[0] and max_rel_err(s, o, L) <= 1e-4
    assert sfail[:2] == ofail[:2] and sfail[0] == 3
    assert grep == srep and gq == sq and gfail[:2] == sfail[:2]
    q = np.array([[20.3, 30.7], [40.1, 2.2], [63.5, 63.5], [0.2, 10.0]])
    assert all(_knn_ok(sq[1][2 * i + j], o, p, k) for i, p in enumerate(q) for j, k in enumerate((1, 5)))
    assert all(_knn_ok(sq[2][i], o, p, len(o)) for i, p in enumerate(q[:2]))  # (k-NN: the exact answer)
    for a, b in ((g, s), (gfail[2], sfail[2])):
        assert (a["id"] == b["id"]).all()
        assert np.array_equal(a["vx"], b["vx"]) and np.array_equal(a["vy"], b["vy"])
        for c in ("x", "y"):
            ulp = np.spacing(a[c])
            assert (np.abs(a[c] - (b[c] + shift)) <= ulp).all(), c  # (the read-back rounds cell + offset once)


# ---- 5. one mesh case ------------------------------------------------------------------------------------------------
def test_a_2x2_mesh_of_two_launch_tiles_matches_the_single_engine():
    """The 16.8M-cell crowd cut into a 2 x 2 LocalTileMesh: every tile holds some 4.2M cells (two-launch scan) and
    all but one have a non-zero origin.  Bitwise equal to the single engine after the same steps."""
    from rmf_crowdsim_amd.tiles import LocalTileMesh
    n = 4097
    grid = _grid(n, n)
    walkers, standers = tile_crowd(n, n)
    single = Simulation(LocationHash2D(**grid))
    mesh = LocalTileMesh(LocationHash2D(**grid), (2, 2), halo_cells=1)
    for t in (single, mesh):
        _populate(t, walkers, standers)
        for k in range(STEPS):
            t.step(DT, report=(k % 10 == 9))
    counts = mesh.tile_counts()
    assert (counts > 0).sum() >= 2 and counts.sum() == len(walkers[0]) + len(walkers[1]) + len(standers)
    assert single.read_agents().tobytes() == mesh.read_agents().tobytes()
