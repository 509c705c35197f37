"""The neighbours of each agent on a tile mesh (cs_mesh_agent_neighbours; NativeTileMesh.agent_neighbours /
count_agents_with_neighbours), in process: every tile computes the rows of its own subjects against its own others, the
participants near a cut travel as band records, each tile merges what its band subjects find behind the cuts into their rows
on its device, min_count is applied after that, and the mesh gives the single engine's answer byte for byte, which is also
the restatement's (tests/neighbours_reference.py).  No halo exchange is made for it: the next steps of the mesh are those of
a mesh that never asked."""
import numpy as np
import pytest

from rmf_crowdsim_amd import LocationHash2D, NoLocalPlan, Selection, Simulation, StubHighLevelPlan, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from neighbours_reference import NONE, SIZE_MAX, agent_neighbours, agree, last_error, neighbours
from select_reference import Ledger, selection
from test_gpu_agent_write import _add_crossing, _crossing

pytestmark = pytest.mark.gpu
INF = float("inf")
CELLS = (0.3, 1.0, 2.5)  # the distances of the single-engine test, in cells


def _pair(shape, halo, n=4096, steps=10):
    """A mesh and a single engine with the same crossing crowd after the same steps -> (mesh, single, ledger of the
    single engine, grid)"""
    pts, pref, group, grid, extent = _crossing(n)
    mesh = NativeTileMesh(LocationHash2D(**grid), shape, halo)
    single = Simulation(LocationHash2D(**grid))
    led = Ledger(single).watch()
    for t in (mesh, single):
        _add_crossing(t, pts, group)
        for _ in range(steps):
            t.step(0.05)
    return mesh, single, led, grid


def _same(mesh, single, rec, grid, distance, sel_s=None, sel_o=None, cols=(None, None, None), name="", cache=None):
    """mesh == single engine == restatement, in every form of agree(); and mesh == single engine over another fill"""
    want = agree(single, rec, grid, distance, sel_s, sel_o, cols, name + " (engine)", cache)
    agree(mesh, rec, grid, distance, sel_s, sel_o, cols, name + " (mesh)", cache)
    n_e, r_e = agent_neighbours(single, distance, sel_s, sel_o, 1, cap=len(want) + 1, fill=0xCD)
    n_m, r_m = agent_neighbours(mesh, distance, sel_s, sel_o, 1, cap=len(want) + 1, fill=0xCD)
    assert n_m == n_e == int((want["count"] >= 1).sum()) and r_m.tobytes() == r_e.tobytes(), name
    return want


def _cuts(grid, shape):
    cell = grid["cell_size"]
    rows, cols_ = int(grid["height"] / cell), int(grid["width"] / cell)
    return ([round(k * rows / shape[0]) * cell for k in range(1, shape[0])],
            [round(k * cols_ / shape[1]) * cell for k in range(1, shape[1])])


@pytest.mark.parametrize("shape,halo", [((2, 2), 1), ((2, 2), 2), ((3, 1), 1), ((3, 1), 2)])
def test_a_mesh_gives_the_rows_of_one_engine(shape, halo):
    mesh, single, led, grid = _pair(shape, halo)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    assert int((mesh.tile_counts() > 0).sum()) >= 2
    cell = grid["cell_size"]
    limit = halo * cell
    distances = sorted(set([c * cell for c in CELLS if c * cell <= limit] + [limit]))
    lhs = {}
    for distance in [0.0] + distances:
        want = _same(mesh, single, rec, grid, distance, name=f"{shape}, halo {halo}, distance {distance}", cache=lhs)
        assert len(want) == len(rec)
        assert int(want["count"].sum()) == 2 * mesh.count_close_pairs(distance)
    # subjects whose nearest stands behind a cut are among them
    cuts_x, cuts_y = _cuts(grid, shape)
    want = neighbours(rec, grid, limit, cache=lhs)
    pos = {int(r["id"]): (float(r["x"]), float(r["y"])) for r in rec}
    across = sum(1 for r in want[want["count"] > 0]
                 if any((pos[int(r["id"])][0] < c) != (pos[int(r["nearest"])][0] < c) for c in cuts_x)
                 or any((pos[int(r["id"])][1] < c) != (pos[int(r["nearest"])][1] < c) for c in cuts_y))
    print(f"{shape}: {int((want['count'] > 0).sum())} subjects with a neighbour within {limit} m, the nearest of {across} "
          "behind a cut")
    assert across > 0
    # the Python surface of the mesh
    got = mesh.agent_neighbours(limit)
    assert got.tobytes() == want.tobytes()
    assert mesh.count_agents_with_neighbours(limit, min_count=2) == int((want["count"] >= 2).sum())
    assert mesh.agent_neighbours(limit, min_count=1, limit=3).tobytes() == want[want["count"] >= 1][:3].tobytes()
    assert mesh.read_agents().tobytes() == rec.tobytes()


def test_around_the_cuts_the_distance_limit_twins_and_roles():
    """2 x 2 tiles over the 240 m grid of the crossing crowd: the cuts lie at 120 m."""
    pts, pref, group, grid, extent = _crossing(4096)
    assert grid["width"] == grid["height"] == 240.0
    meshes = [NativeTileMesh(LocationHash2D(**grid), (2, 2), 1) for _ in range(2)]
    single = Simulation(LocationHash2D(**grid))
    led = Ledger(single).watch()
    mesh, twin = meshes
    for t in (mesh, twin, single):
        _add_crossing(t, pts, group)
        for _ in range(10):
            t.step(0.05)
    # twins: the next 10 steps of the mesh that asked (all forms, every step) are those of the mesh that never did
    limit = grid["cell_size"]
    lower_left = selection(_abi.CS_SEL_RECT, x0=0.0, y0=0.0, x1=125.0, y1=125.0)
    for _ in range(10):
        n, _ = agent_neighbours(mesh, limit, cap=100000)
        assert n == len(mesh) and agent_neighbours(mesh, limit)[0] == n
        assert 0 < agent_neighbours(mesh, limit, lower_left, None, 1, cap=16)[0] < n
        assert 0 < agent_neighbours(mesh, limit, None, lower_left, 2)[0] < n
        for t in (mesh, twin, single):
            t.step(0.05)
    assert mesh.read_agents().tobytes() == twin.read_agents().tobytes() == single.read_agents().tobytes()
    rec = single.read_agents()
    # everybody within 3 m of the inner corner moves out of the way (onto a far row), then: a subject 0.1 m from the
    # corner with one other in each of the four tiles, two of them equidistant in different tiles (dx = -0.5 and +0.5
    # exactly, the same dy); two agents straddling each cut, far from the corner
    near = np.flatnonzero(np.hypot(rec["x"] - 120.0, rec["y"] - 120.0) < 3.0)
    rest = np.setdiff1d(np.arange(len(rec)), near)[:9]
    w = rec[np.concatenate([rest, near])].copy()
    w["x"][:5] = [120.0, 119.5, 120.5, 119.5, 120.6]   # the subject, then the tiles (lo, lo), (hi, lo), (lo, hi), (hi, hi)
    w["y"][:5] = [120.1, 119.75, 119.75, 120.6, 120.7]
    w["x"][5:7], w["y"][5:7] = [119.9, 120.1], [61.0, 61.5]   # across the x cut
    w["x"][7:9], w["y"][7:9] = [70.3, 70.6], [119.85, 120.0]  # across the y cut (one of them ON it)
    w["x"][9:], w["y"][9:] = 30.0 + 0.5 * np.arange(len(near)), 20.5
    for t in (mesh, twin, single):
        t.write_agents(w, fields=("position",))
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    assert (mesh.tile_counts() > 0).all()
    ids = [int(i) for i in w["id"]]
    at = {i: (rec["x"][rec["id"] == i][0], rec["y"][rec["id"] == i][0]) for i in ids[:5]}
    assert [(bool(at[i][0] >= 120.0), bool(at[i][1] >= 120.0)) for i in ids[1:5]] == [(False, False), (True, False),
                                                                                      (False, True), (True, True)]

    def d2_of(i):  # (numpy f64 scalars: every operation rounded once)
        dx, dy = at[ids[0]][0] - at[i][0], at[ids[0]][1] - at[i][1]
        return dx * dx + dy * dy
    assert d2_of(ids[1]) == d2_of(ids[2]) < min(d2_of(ids[3]), d2_of(ids[4])) < 1.0
    lhs = {}
    for distance in (1.0, limit):
        want = _same(mesh, single, rec, grid, distance, name=f"around the cuts, distance {distance}", cache=lhs)
        row = want[want["id"] == ids[0]][0]
        assert row["count"] == 4 and row["nearest"] == min(ids[1], ids[2]) and row["nearest_d2"] == d2_of(ids[1])
        for p, q in ((ids[5], ids[6]), (ids[7], ids[8])):  # (each sees the other behind the cut, or somebody closer)
            xp, yp, xq, yq = (rec[k][rec["id"] == i][0] for i in (p, q) for k in ("x", "y"))
            apart = (xp - xq) * (xp - xq) + (yp - yq) * (yp - yq)
            assert apart < 1.0 and all(want[want["id"] == i][0]["nearest_d2"] <= apart for i in (p, q))
    # a distance just above halo_cells * cell_size is refused, in both forms, and the mesh stays usable
    above = float(np.nextafter(limit, INF))
    for cap in (None, 8):
        n, out = agent_neighbours(mesh, above, cap=cap, fill=0xAB)
        assert n == SIZE_MAX and "halo_cells" in last_error(mesh)
        if cap:
            assert (out.view(np.uint8) == 0xAB).all()
    assert agent_neighbours(mesh, INF)[0] == SIZE_MAX
    assert agent_neighbours(mesh, float("nan"), cap=4)[0] == SIZE_MAX and agent_neighbours(mesh, -1.0)[0] == SIZE_MAX
    assert agent_neighbours(single, above)[0] == len(rec)  # (one engine has no such limit)
    _same(mesh, single, rec, grid, limit, name="after the refusals", cache=lhs)
    # roles: robots in different tiles
    nolp, still = NoLocalPlan(), StubHighLevelPlan((0.0, 0.0))
    spots = np.array([[119.5, 118.9], [120.5, 118.8], [119.4, 121.2], [120.6, 121.1], [90.2, 90.1], [150.3, 90.4],
                      [90.3, 150.2], [150.1, 150.4]])
    robots = {}
    for t in (mesh, twin, single):
        robots[t] = t.add_agents(spots, still, nolp, 2.0)
    assert list(robots[mesh]) == list(robots[single])
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    cols = led.columns(rec)
    lp_robots = led._handles(nolp)[0]
    assert mesh._handles[id(nolp)] == lp_robots
    is_robot = selection(_abi.CS_SEL_LP, lp=lp_robots)
    is_crowd = selection(_abi.CS_SEL_LP, lp=int(cols[2][0]))
    disc = selection(_abi.CS_SEL_CIRCLE, cx=120.0, cy=120.0, r=15.0)
    slow = selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=1.2)
    robot_ids = sorted(int(i) for i in robots[single])
    lhs = {}
    for distance in (1.0, limit):
        want = _same(mesh, single, rec, grid, distance, is_robot, None, cols, f"robots x everyone, {distance}", lhs)
        assert want["id"].tolist() == robot_ids
        if distance == limit:  # the four robots around the inner corner stand in four tiles and see one another
            corner = robot_ids[:4]
            assert (want["count"][:4] >= 1).all()
            only = _same(mesh, single, rec, grid, distance, is_robot, is_robot, cols, f"robots x robots, {distance}", lhs)
            assert only["id"].tolist() == robot_ids and (only["count"][:4] >= 1).all() and (only["count"][4:] == 0).all()
            assert np.isin(only["nearest"][:4], corner).all() and (only["nearest"][4:] == NONE).all()
        _same(mesh, single, rec, grid, distance, is_robot, is_crowd, cols, f"robots x crowd, {distance}", lhs)
        _same(mesh, single, rec, grid, distance, is_crowd, is_robot, cols, f"crowd x robots, {distance}", lhs)
        _same(mesh, single, rec, grid, distance, disc, disc, cols, f"subjects == others across the corner, {distance}", lhs)
        _same(mesh, single, rec, grid, distance, is_crowd, disc, cols, f"overlapping roles, {distance}", lhs)
        _same(mesh, single, rec, grid, distance, disc, slow, cols, f"a speed term behind the cuts, {distance}", lhs)
    want = neighbours(rec, grid, limit, np.asarray(cols[2]) == lp_robots, None)
    assert mesh.agent_neighbours(limit, Selection(local_planner=nolp)).tobytes() == want.tobytes()
    assert mesh.count_agents_with_neighbours(limit, dict(local_planner=nolp), None) == int((want["count"] >= 1).sum())


def _two_rank_cases():
    """(distance, subjects, others, min_count): the cut of the 2 x 1 mesh of the two ranks lies at x = 30 m; the limit is
    2 m"""
    box = selection(_abi.CS_SEL_RECT, x0=24.0, y0=22.5, x1=37.25, y1=36.0)  # across the cut
    left = selection(_abi.CS_SEL_RECT, x0=0.0, y0=0.0, x1=30.0, y1=60.0)    # one rank's side
    return [(0.0, None, None, 0), (0.9, None, None, 0), (2.0, None, None, 1), (2.0, box, None, 0), (1.4, left, None, 2),
            (2.0, None, left, 1), (2.0, left, box, 0)]


def _two_rank_answers(t):
    out = []
    for distance, ss, so, min_count in _two_rank_cases():
        count = agent_neighbours(t, distance, ss, so, min_count)[0]
        n, got = agent_neighbours(t, distance, ss, so, min_count, cap=count + 2, fill=0xEE)
        few = agent_neighbours(t, distance, ss, so, min_count, cap=5, fill=0xEE)
        out.append((count, n, got.tobytes(), few[0], few[1].tobytes()))
    return out


def _rank_counts_neighbours(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import TorchHostTransport
    from test_gpu_agent_write_mesh import GRID, _scene
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 1), 1, device=0, rank=rank, n_ranks=world,
                              host_transport=TorchHostTransport(dist))
        _scene(mesh)
        for _ in range(25):
            mesh.step(0.05, report=False)
        notes = {"before": mesh.read_agents(), "answers": _two_rank_answers(mesh)}
        notes["refused"] = (agent_neighbours(mesh, 2.5)[0] == SIZE_MAX
                            and agent_neighbours(mesh, float("nan"), cap=4)[0] == SIZE_MAX)
        notes["python"] = mesh.agent_neighbours(2.0, min_count=1)
        for _ in range(10):
            mesh.agent_neighbours(2.0, limit=8)
            mesh.count_agents_with_neighbours(1.0)
            mesh.step(0.05, report=False)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_give_the_rows_of_one_engine(tmp_path):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU: the band records and the rows travel through
    the host transport's gathers, every rank gets the whole answer, the single engine's, and steps on as it."""
    import pickle
    import torch.multiprocessing as mp
    from test_gpu_agent_write_mesh import GRID, _scene
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "neighbours.pkl")
    procs = [ctx.Process(target=_rank_counts_neighbours, args=(r, 2, 29813, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    notes = []
    for r in range(2):
        with open(f"{out}.{r}", "rb") as f:
            notes.append(pickle.load(f))
    single = Simulation(LocationHash2D(**GRID))
    _scene(single)
    for _ in range(25):
        single.step(0.05, report=False)
    before = single.read_agents()
    want = _two_rank_answers(single)
    rows = neighbours(before, GRID, 2.0, min_count=1)
    x_of = dict(zip(before["id"].tolist(), before["x"].tolist()))
    assert any((x_of[int(r["id"])] < 30.0) != (x_of[int(r["nearest"])] < 30.0) for r in rows)  # (a nearest of the other rank)
    everyone = len(neighbours(before, GRID, 0.0))
    assert [w[0] for w in want][:3] == [everyone, everyone, len(rows)] and len(rows) > 0
    assert sum(1 for w in want if 0 < w[0] < everyone) >= 3  # (the selections and min_count bite)
    listed = single.agent_neighbours(2.0, min_count=1)
    assert listed.tobytes() == rows.tobytes()
    for _ in range(10):
        single.step(0.05, report=False)
    end = single.read_agents()
    for n in notes:
        assert n["before"].tobytes() == before.tobytes()
        assert n["answers"] == want and n["refused"]
        assert n["python"].tobytes() == listed.tobytes()
        assert len(end) > 400 and n["agents"].tobytes() == end.tobytes()
