"""Band windows cut at agent granularity (csrc/cs_kernel_band_builder.hip.inc, BlockDesc::cut): the agents of a band of
one or two rows, in the order (column, row, slot), are dealt out 256 at a time, so every workgroup of the neighbour kernel
but the band's last is full.  A window then owns only SOME members of its first and last cells; the rest of those cells
is staged like any ghost.  Which window steps an agent changes nothing it computes: the tiled kernel must equal the gather
kernel bit for bit and the f64 oracle at the suite's tolerance (max |dp| / L <= 1e-4, integers exact), over steps in which
agents change cells.  Plain windows throughout (CS_WINDOWS_KEEP=0: kept windows own cells, not slots), every list read
back and checked on the host before its launch (CS_CHECK_WINDOWS=1: every owned slot in exactly one window)."""
import math

import numpy as np
import pytest

from oracle_sim import OracleSimulation
from rmf_crowdsim_amd import LocationHash2D, Simulation, StubHighLevelPlan, Zanlungo, _abi, scenes

pytestmark = pytest.mark.gpu
LP = Zanlungo(*scenes.METRIC_ZANLUNGO)
# agents that stand 0.11 m apart (a cell of several hundred): radius 2 cm so that nobody overlaps
LP_SMALL = Zanlungo(1.0, 1.0, 0.0, 0.04, 2.0, 0.02)
TILE = 256
DT = 0.05


def _full_windows(rec, grid, rows_per_band=2):
    """sum over the bands of ceil(agents of the band / 256): what a list of full windows has"""
    row = np.floor((rec["x"] - grid["offset"][0]) / grid["cell_size"]).astype(np.int64)
    per_band = np.bincount(row // rows_per_band)
    return int(sum(math.ceil(c / TILE) for c in per_band if c))


def _tiled_gather_oracle(monkeypatch, grid, populate, steps=4, exact=True):
    """Steps the scene on the tiled kernel, the gather kernel and the oracle.  Returns the tiled run's records, the
    windows listed per step and the count full windows would have (from the positions each step started from)."""
    monkeypatch.setenv("CS_WINDOWS_KEEP", "0")
    monkeypatch.setenv("CS_CHECK_WINDOWS", "1")
    tiled = Simulation(LocationHash2D(**grid), flags=_abi.CS_CFG_FORCE_TILED)
    populate(tiled)
    listed, full = [], []
    for _ in range(steps):
        full.append(_full_windows(tiled.read_agents(), grid))
        tiled.step(DT)
        listed.append(tiled.kernel_stat(_abi.CS_STAT_WINDOWS_LISTED))
    a = tiled.read_agents()
    assert not exact or tiled.kernel_stat(_abi.CS_STAT_WINDOWS_CHUNKED) == 0
    off_lds = tiled.kernel_stat(_abi.CS_STAT_WINDOWS_OFF_LDS)
    tiled.close()
    monkeypatch.delenv("CS_CHECK_WINDOWS")
    gather = Simulation(LocationHash2D(**grid), flags=_abi.CS_CFG_FORCE_GATHER)
    oracle = OracleSimulation(LocationHash2D(**grid))
    for sim in (gather, oracle):
        populate(sim)
        for _ in range(steps):
            sim.step(DT)
    b, o = gather.read_agents(), oracle.read_agents()
    gather.close()
    oracle.close()
    print(f"windows listed {listed}, full windows {full}, off the LDS path {off_lds}")
    assert len(a) == len(o) and a.tobytes() == b.tobytes()
    assert (a["id"] == o["id"]).all() and (a["next_waypoint"] == o["next_waypoint"]).all()
    extent = max(grid["width"], grid["height"])
    err = float(np.hypot(a["x"] - o["x"], a["y"] - o["y"]).max() / extent)
    print(f"max |dp| / L vs the oracle {err:.3e}")
    assert err <= 1e-4
    if exact:
        assert listed == full
    else:
        assert all(l >= f for l, f in zip(listed, full))
    return a, listed, full, off_lds


def _walkers(pts, group, lp=LP, eyesight=2.0, walk=scenes.WALK_SPEED):
    return lambda sim: scenes.add_walking_crowd(sim, pts, group, lp, eyesight, walk=walk)


def test_uniform_crowd_has_exactly_the_full_windows(monkeypatch):
    """6,000 walkers, ~10 per cell, bands of ~190 to ~1,500 agents: the windows listed equal sum ceil(band / 256) in
    every step, so the lanes in use are agents / (256 x windows)."""
    pts, grid, extent, group = scenes.uniform_crowd(6000, seed=3, cell_size=2.0, room=4.0)
    a, listed, full, _ = _tiled_gather_oracle(monkeypatch, grid, _walkers(pts, group), steps=5)
    assert len(a) == 6000
    # (the walkers keep their preferred velocity: whoever stood within 32.5 cm of its row's end has changed cell)
    assert (np.floor(a["x"] / 2.0) != np.floor((a["x"] - 5 * DT * scenes.WALK_SPEED) / 2.0)).sum() > 300
    print(f"lanes in use: {6000 / (TILE * listed[-1]):.3f}")


def test_creeping_counterflow_with_forces_on_agent_cut_windows(monkeypatch):
    """The same crowd as a creeping counter-flow: every agent has a finite time to collision and non-zero forces, summed
    over neighbours that other windows own."""
    pts, grid, extent, group = scenes.uniform_crowd(5000, seed=11, cell_size=2.0)

    def populate(sim):
        scenes.add_counterflow(sim, pts, group, scenes.CREEP_SPEED, LP, 2.0)
    a, _, _, _ = _tiled_gather_oracle(monkeypatch, grid, populate, steps=4)
    assert np.mean(np.hypot(a["vx"], np.abs(a["vy"]) - scenes.CREEP_SPEED) > 0) > 0.9


def _cell_block(n, row, col, cell=2.0, columns=18):
    """n agents 0.11 m apart inside the cell (row, col): x picks the row, y the column"""
    return scenes.jittered_lattice(n, 0.11, (row * cell + 0.01, col * cell + 0.01), 0.2, 17 + row + col, columns=columns)


def test_cells_of_more_than_and_exactly_a_workgroup(monkeypatch):
    """Beside a walking crowd, in bands of their own: a cell of 300 agents with a cell of 256 four columns on (band 1:
    556 agents = 256 of the first cell | its last 44 and 212 of the second | the second's last 44: three windows own
    parts of one cell), and a cell of exactly 256 followed by one of 10 (band 15: the first cut falls behind the last
    agent of a cell and in front of the first agent of the next).  The two bands lie far apart: a window stages its
    band's ghost rows too, and here it may stage 729 agents (95 % of the 768 LDS slots of a window at this mean
    occupancy), so the 556 of band 1 leave no room for another big cell in a ghost row; a band whose full windows
    would stage more keeps the whole-column rule, as the test of the staging bound below shows."""
    pts, grid, extent, group = scenes.uniform_crowd(3000, seed=5, cell_size=2.0, margin=14.0, room=4.0)
    blocks = [_cell_block(300, 2, 6), _cell_block(256, 2, 10), _cell_block(256, 30, 6), _cell_block(10, 30, 9)]
    for b, (r, c) in zip(blocks, ((2, 6), (2, 10), (30, 6), (30, 9))):
        assert (np.floor(b[:, 0] / 2.0) == r).all() and (np.floor(b[:, 1] / 2.0) == c).all()

    def populate(sim):
        scenes.add_walking_crowd(sim, pts, group, LP, 2.0)
        for b in blocks:  # (two creeping streams inside every block: finite times to collision)
            sim.add_agents(b[0::2], StubHighLevelPlan((scenes.WALK_SPEED, scenes.CREEP_SPEED)), LP_SMALL, 0.3)
            sim.add_agents(b[1::2], StubHighLevelPlan((scenes.WALK_SPEED, -scenes.CREEP_SPEED)), LP_SMALL, 0.3)
    a, listed, full, off_lds = _tiled_gather_oracle(monkeypatch, grid, populate, steps=5)
    assert len(a) == 3000 + 822 and off_lds == 0
    assert full[0] == _full_windows(np.rec.fromarrays([pts[:, 0]], names="x"), grid) + 3 + 2


@pytest.mark.parametrize("scene", ["empty first row", "empty second row", "empty columns", "odd rows"])
def test_bands_with_holes(scene, monkeypatch):
    """A band whose first or second row is empty (the crowd is a strip one row wide; walkers cross into the empty row
    during the steps), bands with runs of empty columns in the middle, and a grid of 31 rows whose last band has one row."""
    cell = 2.0
    grid = dict(width=62.0, height=62.0, cell_size=cell, offset=(0.0, 0.0))
    walk = scenes.WALK_SPEED
    if scene in ("empty first row", "empty second row"):
        x0 = 22.0 if scene == "empty first row" else 20.0  # row 11 / row 10 of band 5 (rows 10 and 11)
        k = np.arange(270)
        strip = np.stack([x0 + 0.55 + (k % 3) * 0.6, 3.0 + (k // 3) * 0.6], axis=1)   # the last line crosses the row's end
        pts = np.concatenate([strip, strip + np.array([16.0, 0.3])])                    # a second strip, eight rows on
    elif scene == "empty columns":
        k = np.arange(1500)
        left = np.stack([10.3 + (k // 30) * 0.632, 4.3 + (k % 30) * 0.632], axis=1)
        pts = np.concatenate([left, left + np.array([0.0, 30.0])])   # columns 2-11 and 17-26: five empty ones in every band
    else:
        walk = -scenes.WALK_SPEED  # (towards low x: the crowd starts in the grid's last row, 60 <= x < 62)
        k = np.arange(2400)
        pts = np.stack([61.8 - (k // 60) * 0.632, 6.0 + (k % 60) * 0.632], axis=1)
    group = np.arange(len(pts)) % 2
    a, listed, full, _ = _tiled_gather_oracle(monkeypatch, grid, _walkers(pts, group, walk=walk), steps=5)
    assert len(a) == len(pts)
    if scene == "odd rows":
        assert (np.floor(pts[:, 0] / cell) == 30).sum() > 100


@pytest.mark.parametrize("eyesight", [2.0, 3.0])
def test_eyesight_of_two_and_three_cells(eyesight, monkeypatch):
    """Cells of 1 m: two and three ghost rows and columns around a window; bands of ~350 agents, whose full window spans
    ~50 columns."""
    pts, grid, extent, group = scenes.uniform_crowd(12000, seed=6, cell_size=1.0, margin=6.0, room=2.0)
    # (at three cells a full window stages ~1,180 agents of the 1,277 it may: within the jitter of a band's count of the
    # bound, so only the two-cell case insists on full windows)
    a, listed, full, off_lds = _tiled_gather_oracle(monkeypatch, grid, _walkers(pts, group, eyesight=eyesight), steps=4,
                                                    exact=(eyesight == 2.0))
    assert len(a) == 12000 and off_lds == 0


def test_sparse_band_beside_dense_rows_keeps_the_staging_bound(monkeypatch):
    """Two dense rows (~20 agents per cell) between sparse bands (~1 per cell) on a grid 130 columns wide: 256 agents of a
    sparse band span ~100 columns, whose ghost row holds ~2,000 agents, far more than a window may stage.  Such a band
    is cut by the whole-column rule under the staging bound as before (more windows than full ones), no window leaves
    the LDS path, and the dense band beside it is still dealt out 256 at a time."""
    cell = 2.0
    grid = dict(width=260.0, height=40.0, cell_size=cell, offset=(0.0, 0.0))  # 20 rows x 130 columns
    kd = np.arange(2 * 4 * 520)
    dense = np.stack([16.0 + 0.25 + (kd // 520) * 0.45, 6.0 + (kd % 520) * 0.45 + 0.1], axis=1)   # rows 8, 9 (x in 16 .. 19.6)
    ks = np.arange(4 * 120)
    sparse_lo = np.stack([12.5 + (ks // 120) * 0.9, 8.0 + (ks % 120) * 1.9], axis=1)            # rows 6, 7
    sparse_hi = sparse_lo + np.array([8.0, 0.5])                                                  # rows 10, 11
    pts = np.concatenate([dense, sparse_lo, sparse_hi])
    group = np.arange(len(pts)) % 2
    a, listed, full, off_lds = _tiled_gather_oracle(monkeypatch, grid, _walkers(pts, group), steps=4, exact=False)
    assert len(a) == len(pts) and off_lds == 0
    assert listed[0] > full[0]   # the sparse bands' windows were cut short by what they stage


def test_window_check_reports_a_list_beyond_the_launch(monkeypatch):
    """CS_TILE_WINDOWS_CAP sizes the launch for five windows where the crowd needs ~30: the host-side check of the list
    (the new descriptors included) refuses it before anything is launched, and nothing faults."""
    monkeypatch.setenv("CS_WINDOWS_KEEP", "0")
    monkeypatch.setenv("CS_CHECK_WINDOWS", "1")
    monkeypatch.setenv("CS_TILE_WINDOWS_CAP", "5")
    pts, grid, extent, group = scenes.uniform_crowd(6000, seed=3, cell_size=2.0)
    sim = Simulation(LocationHash2D(**grid), flags=_abi.CS_CFG_FORCE_TILED)
    scenes.add_walking_crowd(sim, pts, group, LP, 2.0)
    with pytest.raises(RuntimeError, match=r"window check: \d+ windows listed, the array holds \d+, the launch 5"):
        sim.step(DT)
    monkeypatch.delenv("CS_TILE_WINDOWS_CAP")
    ok = Simulation(LocationHash2D(**grid), flags=_abi.CS_CFG_FORCE_TILED)  # (the same list passes with its real launch)
    scenes.add_walking_crowd(ok, pts, group, LP, 2.0)
    ok.step(DT)
    assert ok.kernel_stat(_abi.CS_STAT_WINDOWS_LISTED) == _full_windows(np.rec.fromarrays([pts[:, 0]], names="x"), grid)


def test_kept_windows_still_own_cells(monkeypatch):
    """A small crowd steps on windows cut one step earlier (the 125k-agent path, here 6,000 agents): those are cut by
    the whole-column rule with fillers, as before.  The host-side check refuses a slot-owning window in a kept list and
    wants every column of every band covered exactly once; the results equal windows cut every step and the gather
    kernel; the kept lists hold more windows than full ones would be."""
    pts, grid, extent, group = scenes.uniform_crowd(6000, seed=3, cell_size=2.0, room=4.0)
    monkeypatch.setenv("CS_CHECK_WINDOWS", "1")
    runs = {}
    for name, keep, flags in (("kept", "1", 2), ("every", "0", 2), ("gather", "0", 1)):
        monkeypatch.setenv("CS_WINDOWS_KEEP", keep)
        sim = Simulation(LocationHash2D(**grid), flags=flags)
        scenes.add_walking_crowd(sim, pts, group, LP, 2.0)
        listed = []
        for _ in range(6):
            sim.step(DT)
            listed.append(sim.kernel_stat(_abi.CS_STAT_WINDOWS_LISTED))
        runs[name] = (sim.read_agents(), listed, sim.kernel_stat(_abi.CS_STAT_STEPS_ON_KEPT_WINDOWS))
        sim.close()
    assert runs["kept"][0].tobytes() == runs["every"][0].tobytes() == runs["gather"][0].tobytes()
    assert runs["kept"][2] >= 4 and runs["every"][2] == 0
    full = _full_windows(np.rec.fromarrays([pts[:, 0]], names="x"), grid)
    print(f"windows listed: kept {runs['kept'][1]}, cut every step {runs['every'][1]}, full {full}")
    assert runs["every"][1][0] == full and min(runs["kept"][1]) > full and runs["gather"][1] == [0] * 6


# ---- a 2 x 2 mesh, one rank per tile over gloo, border windows cut by the same rule ------------------------------
_MESH_GRID = dict(width=96.0, height=96.0, cell_size=2.0, offset=(0.0, 0.0))


def _mesh_scene(target):
    pts, _, _, group = scenes.uniform_crowd(12000, seed=8, cell_size=2.0, margin=12.0)
    for g, v in enumerate(((1.30, 0.4), (1.28, 0.4))):   # walkers that cross cells and the cuts between tiles
        target.add_agents(pts[group == g], StubHighLevelPlan(v), LP, 2.0)


def _mesh_rank(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import NativeTileMesh, TorchHostTransport
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["CS_TILE_SPLIT"] = "1"   # the border windows as a list and a launch of their own
    os.environ["CS_WINDOWS_KEEP"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mesh = NativeTileMesh(LocationHash2D(**_MESH_GRID), (2, 2), 1, device=0, rank=rank, n_ranks=world,
                              flags=_abi.CS_CFG_TILE_OVERLAP | _abi.CS_CFG_FORCE_TILED,
                              host_transport=TorchHostTransport(dist))
        _mesh_scene(mesh)
        for k in range(5):
            mesh.step(DT, report=(k == 4))
        a = mesh.read_agents()
        counts = [None] * world
        dist.all_gather_object(counts, int(mesh.tile_counts().sum()))
        if rank == 0:
            with open(out_path, "wb") as f:
                pickle.dump((a, counts), f)
    finally:
        dist.destroy_process_group()


def test_two_by_two_mesh_over_gloo_with_border_windows(tmp_path):
    """Four ranks (2 x 2 tiles of ~3,000 agents) over torch.distributed / gloo sharing the GPU, CS_CFG_TILE_OVERLAP with
    the windows along a tile's edges listed and launched apart (they pack the next step's halo records): the border
    and interior lists are both cut at agent granularity, border classification by the span of owned columns.  The
    mesh equals one engine bit for bit."""
    import pickle
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "mesh.pkl")
    procs = [ctx.Process(target=_mesh_rank, args=(r, 4, 29761, out)) for r in range(4)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    with open(out, "rb") as f:
        both, counts = pickle.load(f)
    single = Simulation(LocationHash2D(**_MESH_GRID), flags=_abi.CS_CFG_FORCE_GATHER)
    _mesh_scene(single)
    for _ in range(5):
        single.step(DT, report=False)
    a = single.read_agents()
    assert len(a) == 12000 and a.tobytes() == both.tobytes()
    assert sum(counts) == 12000 and min(counts) > 1000
