"""The pairs of agents within a distance on a tile mesh (cs_mesh_close_pairs; NativeTileMesh.close_pairs /
count_close_pairs), in process: every tile lists the pairs among its own agents, the agents near a cut travel as band
records and are paired across tiles, and the mesh gives the single engine's answer byte for byte: pairs, order, count and
the bits of d2, which is also the restatement's (tests/close_pairs_reference.py).  No halo exchange is made for it: the
next steps of the mesh are those of a mesh that never asked."""
import numpy as np
import pytest

from rmf_crowdsim_amd import LocationHash2D, NoLocalPlan, Selection, Simulation, StubHighLevelPlan, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from close_pairs_reference import SIZE_MAX, agree, close_pairs, last_error, pairs
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


def _same(mesh, single, rec, grid, distance, sel_a=None, sel_b=None, cols=(None, None, None), name=""):
    """mesh == single engine == restatement, in the listing form, the count-only form and under a cap"""
    want, want_d2 = agree(single, rec, grid, distance, sel_a, sel_b, cols, name + " (engine)")
    agree(mesh, rec, grid, distance, sel_a, sel_b, cols, name + " (mesh)")
    n_e, p_e, d_e = close_pairs(single, distance, sel_a, sel_b, cap=len(want) + 1, fill=0xCD)
    n_m, p_m, d_m = close_pairs(mesh, distance, sel_a, sel_b, cap=len(want) + 1, fill=0xCD)
    assert n_m == n_e == len(want) and p_m.tobytes() == p_e.tobytes() and d_m.tobytes() == d_e.tobytes(), name
    return want, want_d2


@pytest.mark.parametrize("shape,halo", [((2, 2), 1), ((1, 3), 1), ((3, 1), 3)])
def test_a_mesh_lists_the_pairs_of_one_engine(shape, halo):
    mesh, single, led, grid = _pair(shape, halo)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    assert int((mesh.tile_counts() > 0).sum()) >= 2
    cell = grid["cell_size"]
    limit = halo * cell
    distances = [c * cell for c in CELLS if c * cell <= limit]
    assert len(distances) >= 2 and (halo != 1 or limit in distances)  # (with one halo cell: one distance IS the limit)
    for distance in [0.0] + distances:
        want, _ = _same(mesh, single, rec, grid, distance, name=f"{shape}, distance {distance}")
        assert len(want) > 0 if distance >= cell else distance > 0.0 or len(want) == 0
    # pairs across the cuts are among them: both agents within `limit` of a cut, on either side of it
    rows, cols_ = int(grid["height"] / cell), int(grid["width"] / cell)
    cuts_x = [round(k * rows / shape[0]) * cell for k in range(1, shape[0])]
    cuts_y = [round(k * cols_ / shape[1]) * cell for k in range(1, shape[1])]
    want, _ = pairs(rec, grid, limit)
    pos = {int(r["id"]): (float(r["x"]), float(r["y"])) for r in rec}
    across = sum(1 for p, q in want.tolist()
                 if any((pos[p][0] < c) != (pos[q][0] < c) for c in cuts_x) or any((pos[p][1] < c) != (pos[q][1] < c) for c in cuts_y))
    print(f"{shape}: {len(want)} pairs within {limit} m, {across} of them across a cut")
    assert across > 0
    # the Python surface of the mesh
    got, d2 = mesh.close_pairs(limit, distances=True)
    want, want_d2 = pairs(rec, grid, limit)
    assert got.tolist() == want.tolist() and d2.tobytes() == want_d2.tobytes()
    assert mesh.count_close_pairs(limit) == len(want) and mesh.close_pairs(limit, limit=3).tolist() == want[:3].tolist()
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
        n, _, _ = close_pairs(mesh, limit, cap=100000)
        assert 0 < n < 100000 and close_pairs(mesh, limit)[0] == n
        assert 0 < close_pairs(mesh, limit, lower_left, None, cap=16)[0] < n
        for t in (mesh, twin, single):
            t.step(0.05)
    assert mesh.read_agents().tobytes() == twin.read_agents().tobytes() == single.read_agents().tobytes()
    rec = single.read_agents()
    # four agents around the inner corner, two straddling each cut, far from the corner
    w = rec[[10, 11, 12, 13, 20, 21, 30, 31]].copy()
    w["x"][:4] = [119.7, 120.3, 119.75, 120.25]
    w["y"][:4] = [119.8, 119.7, 120.2, 120.35]
    w["x"][4:6], w["y"][4:6] = [119.9, 120.1], [61.0, 61.5]   # across the x cut
    w["x"][6:8], w["y"][6:8] = [70.3, 70.6], [119.85, 120.0]  # across the y cut (one of them ON it)
    for t in (mesh, twin, single):
        t.write_agents(w, fields=("position",))
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    assert (mesh.tile_counts() > 0).all()
    ids = [int(i) for i in w["id"]]
    expected = [sorted((ids[i], ids[j])) for i in range(4) for j in range(i + 1, 4)] + [sorted(ids[4:6]), sorted(ids[6:8])]
    for distance in (1.0, limit):
        want, _ = _same(mesh, single, rec, grid, distance, name=f"around the cuts, distance {distance}")
        listed = want.tolist()
        assert all(p in listed for p in expected), distance
    # a distance just above halo_cells * cell_size is refused, in both forms, and the mesh stays usable
    above = float(np.nextafter(limit, INF))
    for cap in (None, 8):
        n, out, d2 = close_pairs(mesh, above, cap=cap, fill=0xAB)
        assert n == SIZE_MAX and "halo_cells" in last_error(mesh)
        if cap:
            assert (out.view(np.uint8) == 0xAB).all() and (d2.view(np.uint8) == 0xAB).all()
    assert close_pairs(mesh, INF)[0] == SIZE_MAX
    assert close_pairs(single, above)[0] == pairs(rec, grid, above, count_only=True)  # (one engine has no such limit)
    _same(mesh, single, rec, grid, limit, name="after the refusals")
    # roles: robots in different tiles
    nolp, still = NoLocalPlan(), StubHighLevelPlan((0.0, 0.0))
    spots = np.array([[119.5, 119.5], [120.5, 119.4], [119.4, 120.6], [120.6, 120.5], [90.2, 90.1], [150.3, 90.4],
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
    robot_ids = set(int(i) for i in robots[single])
    for distance in (1.0, limit):
        want, _ = _same(mesh, single, rec, grid, distance, is_robot, None, cols, f"robots x everyone, {distance}")
        assert all(p in robot_ids or q in robot_ids for p, q in want.tolist())
        if distance == limit:  # the four robots around the inner corner stand in four tiles and pair with one another
            corner = sorted(robot_ids)[:4]
            assert all([p, q] in want.tolist() for i, p in enumerate(corner) for q in corner[i + 1:])
        _same(mesh, single, rec, grid, distance, is_robot, is_crowd, cols, f"robots x crowd, {distance}")
        _same(mesh, single, rec, grid, distance, disc, disc, cols, f"A == B across the corner, {distance}")
        _same(mesh, single, rec, grid, distance, is_crowd, disc, cols, f"overlapping roles, {distance}")
    want, _ = pairs(rec, grid, limit, np.asarray(cols[2]) == lp_robots, None)
    assert mesh.close_pairs(limit, Selection(local_planner=nolp)).tolist() == want.tolist()
    assert mesh.count_close_pairs(limit, None, dict(local_planner=nolp)) == len(want)


def _two_rank_cases():
    """(distance, role A): the cut of the 2 x 1 mesh of the two ranks lies at x = 30 m; the limit is 2 m"""
    box = selection(_abi.CS_SEL_RECT, x0=24.0, y0=22.5, x1=37.25, y1=36.0)  # across the cut
    left = selection(_abi.CS_SEL_RECT, x0=0.0, y0=0.0, x1=30.0, y1=60.0)    # one rank's side
    return [(0.0, None), (0.9, None), (2.0, None), (2.0, box), (1.4, left)]


def _two_rank_answers(t):
    out = []
    for distance, sel in _two_rank_cases():
        count = close_pairs(t, distance, sel, None)[0]
        n, got, d2 = close_pairs(t, distance, sel, None, cap=count + 2, fill=0xEE)
        few = close_pairs(t, distance, sel, None, cap=5, want_d2=False)
        out.append((count, n, got.tobytes(), d2.tobytes(), few[0], few[1].tobytes()))
    return out


def _rank_lists_pairs(rank, world, port, out_path):
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
        notes["refused"] = close_pairs(mesh, 2.5)[0] == SIZE_MAX and close_pairs(mesh, float("nan"), cap=4)[0] == SIZE_MAX
        notes["python"] = mesh.close_pairs(2.0, distances=True)
        for _ in range(10):
            mesh.close_pairs(2.0, limit=8)
            mesh.step(0.05, report=False)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_list_the_pairs_of_one_engine(tmp_path):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU: the band records and the pair lists travel
    through the host transport's gathers, every rank gets the whole answer, the single engine's, and steps on as it."""
    import pickle
    import torch.multiprocessing as mp
    from test_gpu_agent_write_mesh import GRID, _scene
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "pairs.pkl")
    procs = [ctx.Process(target=_rank_lists_pairs, args=(r, 2, 29789, out)) for r in range(2)]
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
    across, _ = pairs(before, GRID, 2.0)
    x_of = dict(zip(before["id"].tolist(), before["x"].tolist()))
    assert any((x_of[p] < 30.0) != (x_of[q] < 30.0) for p, q in across.tolist())  # (pairs of agents of both ranks)
    assert [w[0] for w in want][:3] == [0, len(pairs(before, GRID, 0.9)[0]), len(across)] and want[1][0] > 0
    listed = single.close_pairs(2.0, distances=True)
    for _ in range(10):
        single.step(0.05, report=False)
    end = single.read_agents()
    for n in notes:
        assert n["before"].tobytes() == before.tobytes()
        assert n["answers"] == want and n["refused"]
        assert n["python"][0].tobytes() == listed[0].tobytes() and n["python"][1].tobytes() == listed[1].tobytes()
        assert len(end) > 400 and n["agents"].tobytes() == end.tobytes()
