"""Encounters on a tile mesh (cs_mesh_encounters; NativeTileMesh.encounters / count_encounters), in process: every tile lists
the encounters among its own agents, the agents near a cut travel as band records with their velocity and are tested across
tiles, and the mesh gives the single engine's answer byte for byte: rows, order, count and the bits of t and d2, which is
also the restatement's (tests/encounters_reference.py).  No halo exchange is made for it: the next steps of the mesh are
those of a mesh that never asked."""
import numpy as np
import pytest

from rmf_crowdsim_amd import LocationHash2D, NoLocalPlan, Selection, Simulation, StubHighLevelPlan, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from close_pairs_reference import SIZE_MAX, last_error
from encounters_reference import agree, call, encounters
from select_reference import Ledger, selection
from test_gpu_agent_write import _add_crossing, _crossing

pytestmark = pytest.mark.gpu
INF = float("inf")
RANGES = (0.3, 1.0, 2.5, 3.0)  # in cells
N = 2048


def _crowd():
    """The crossing crowd of 2048 agents on a grid of 108 x 108 cells, which 2 and 3 tiles divide evenly: the cuts of two
    tiles lie at 108 m, those of three at 72 m and 144 m, and the crowd (40 m to 127 m) stands astride them."""
    pts, pref, group, grid, extent = _crossing(N)
    assert grid["width"] == grid["height"] <= 216.0 and grid["cell_size"] == 2.0
    return pts, group, dict(grid, width=216.0, height=216.0)
NUMBERS = ((0.8, 2.0), (1.5, 1.0), (0.4, INF))  # (distance, horizon)


def _same(mesh, single, rec, grid, numbers, sel_a=None, sel_b=None, cols=(None, None, None), name="", stats=None):
    """mesh == single engine == restatement, in the listing form, the count-only form and under a cap"""
    want = agree(single, rec, grid, *numbers, sel_a, sel_b, cols, name + " (engine)", stats=stats)
    agree(mesh, rec, grid, *numbers, sel_a, sel_b, cols, name + " (mesh)", want=want)
    n_e, r_e = call(single, *numbers, sel_a, sel_b, cap=len(want) + 1, fill=0xCD)
    n_m, r_m = call(mesh, *numbers, sel_a, sel_b, cap=len(want) + 1, fill=0xCD)
    assert n_m == n_e == len(want) and r_m.tobytes() == r_e.tobytes(), name
    return want


def _crosses(rows, rec, cuts_x, cuts_y):
    """how many rows hold two agents on different sides of a cut"""
    pos = {int(r["id"]): (float(r["x"]), float(r["y"])) for r in rec}
    return sum(1 for r in rows
               if any((pos[int(r["a"])][0] < c) != (pos[int(r["b"])][0] < c) for c in cuts_x)
               or any((pos[int(r["a"])][1] < c) != (pos[int(r["b"])][1] < c) for c in cuts_y))


@pytest.mark.parametrize("shape,halo", [((2, 2), 1), ((1, 3), 1), ((3, 1), 3)])
def test_a_mesh_lists_the_encounters_of_one_engine(shape, halo):
    pts, group, grid = _crowd()
    mesh = NativeTileMesh(LocationHash2D(**grid), shape, halo)
    single = Simulation(LocationHash2D(**grid))
    for t in (mesh, single):
        _add_crossing(t, pts, group)
        for _ in range(40):
            t.step(0.05)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    assert int((mesh.tile_counts() > 0).sum()) >= 2
    cell = grid["cell_size"]
    limit = halo * cell
    ranges = [c * cell for c in RANGES if c * cell <= limit]
    assert limit in ranges  # (one range IS the limit)
    for k, range_ in enumerate(ranges):
        distance, horizon = NUMBERS[k % len(NUMBERS)]
        stats = {}
        want = _same(mesh, single, rec, grid, (distance, horizon, range_), name=f"{shape}, {(distance, horizon, range_)}",
                     stats=stats)
        assert range_ < cell or 0 < len(want) < stats["in_range"]
    _same(mesh, single, rec, grid, (0.8, 2.0, 0.0), name=f"{shape}, range 0")
    # encounters across the cuts are among them
    rows_, cols_ = int(grid["height"] / cell), int(grid["width"] / cell)
    cuts_x = [round(k * rows_ / shape[0]) * cell for k in range(1, shape[0])]
    cuts_y = [round(k * cols_ / shape[1]) * cell for k in range(1, shape[1])]
    want = _same(mesh, single, rec, grid, (1.5, 2.0, limit), name=f"{shape}, at the limit")
    across = _crosses(want, rec, cuts_x, cuts_y)
    moving = int(((want["t"] > 0.0) & (want["t"] < 2.0)).sum())
    print(f"{shape}: {len(want)} encounters within {limit} m, {across} of them across a cut, {moving} with 0 < t < horizon")
    assert across > 0 and moving > 0
    # a range just above halo_cells * cell_size is refused, in both forms, as is +inf; the mesh stays usable
    above = float(np.nextafter(limit, INF))
    for range_ in (above, INF):
        for cap in (None, 8):
            n, out = call(mesh, 1.5, 2.0, range_, cap=cap, fill=0xAB)
            assert n == SIZE_MAX and "halo_cells" in last_error(mesh)
            if cap:
                assert (out.view(np.uint8) == 0xAB).all()
    assert call(single, 1.5, 2.0, above)[0] == encounters(rec, grid, 1.5, 2.0, above, count_only=True)  # (one engine: no limit)
    assert call(mesh, INF, INF, limit)[0] == call(single, INF, INF, limit)[0] > 0  # (only the range is limited)
    # the Python surface of the mesh
    got = mesh.encounters(1.5, 2.0, limit)
    assert got.tobytes() == want.tobytes()
    assert mesh.count_encounters(1.5, 2.0, limit) == len(want) and mesh.encounters(1.5, 2.0, limit, limit=3).tobytes() == want[:3].tobytes()
    assert mesh.read_agents().tobytes() == rec.tobytes()


def test_around_the_cuts_twins_and_roles():
    """2 x 2 tiles over the 216 m grid of the crossing crowd: the cuts lie at 108 m."""
    pts, group, grid = _crowd()
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
    lower_left = selection(_abi.CS_SEL_RECT, x0=0.0, y0=0.0, x1=112.0, y1=112.0)
    for _ in range(10):
        n, _ = call(mesh, 1.5, 2.0, limit, cap=100000)
        assert 0 < n < 100000 and call(mesh, 1.5, 2.0, limit)[0] == n
        assert 0 < call(mesh, 1.5, 2.0, limit, lower_left, None, cap=16)[0] < n
        for t in (mesh, twin, single):
            t.step(0.05)
    assert mesh.read_agents().tobytes() == twin.read_agents().tobytes() == single.read_agents().tobytes()
    rec = single.read_agents()
    # agents astride the cuts with closing velocities: four around the inner corner, all heading for it; two across the x
    # cut and two across the y cut (one of them ON it), far from the corner, each pair closing at 1 m/s
    w = rec[[10, 11, 12, 13, 20, 21, 30, 31]].copy()
    w["x"][:4] = [107.0, 109.0, 107.0, 109.0]
    w["y"][:4] = [107.0, 107.0, 109.0, 109.0]
    w["vx"][:4], w["vy"][:4] = [0.5, -0.5, 0.5, -0.5], [0.5, 0.5, -0.5, -0.5]
    w["x"][4:6], w["y"][4:6] = [107.25, 108.75], [61.0, 61.0]     # across the x cut
    w["vx"][4:6], w["vy"][4:6] = [0.5, -0.5], [0.0, 0.0]
    w["x"][6:8], w["y"][6:8] = [70.5, 70.5], [106.5, 108.0]       # across the y cut
    w["vx"][6:8], w["vy"][6:8] = [0.0, 0.0], [0.75, -0.25]
    for t in (mesh, twin, single):
        t.write_agents(w, fields=("position", "velocity"))
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    assert (mesh.tile_counts() > 0).all()
    ids = [int(i) for i in w["id"]]
    sides = [(0, 1), (0, 2), (1, 3), (2, 3)]  # 2 m apart, closing at 1 m/s: they meet after 2 s
    diagonals = [(0, 3), (1, 2)]              # 2.83 m apart: out of range
    want = _same(mesh, single, rec, grid, (0.5, 3.0, limit), name="around the cuts")
    got = {(int(r["a"]), int(r["b"])): (float(r["t"]), float(r["d2"])) for r in want}
    key = lambda i, j: tuple(sorted((ids[i], ids[j])))  # noqa: E731
    assert all(key(i, j) not in got for i, j in sides + diagonals)  # (d2 == range^2, and beyond it: not in range)
    assert got[key(4, 5)] == (1.5, 0.0) and got[key(6, 7)] == (1.5, 0.0)
    want = _same(mesh, single, rec, grid, (1.25, 1.0, limit), name="around the cuts, clamped")
    got = {(int(r["a"]), int(r["b"])): (float(r["t"]), float(r["d2"])) for r in want}
    assert got[key(4, 5)] == (1.0, 0.25) and got[key(6, 7)] == (1.0, 0.25)
    inner = w[:4].copy()  # the four a quarter of a metre further in: 1.5 m apart along the sides
    inner["x"], inner["y"] = [107.25, 108.75, 107.25, 108.75], [107.25, 107.25, 108.75, 108.75]
    for t in (mesh, twin, single):
        t.write_agents(inner, fields=("position",))
    rec = single.read_agents()
    want = _same(mesh, single, rec, grid, (0.5, 3.0, limit), name="around the corner")
    got = {(int(r["a"]), int(r["b"])): (float(r["t"]), float(r["d2"])) for r in want}
    assert all(got[key(i, j)] == (1.5, 0.0) for i, j in sides) and all(key(i, j) not in got for i, j in diagonals)
    # roles: robots in different tiles
    nolp, still = NoLocalPlan(), StubHighLevelPlan((0.0, 0.0))
    spots = np.array([[107.5, 107.5], [108.5, 107.4], [107.4, 108.6], [108.6, 108.5], [80.2, 80.1], [130.3, 80.4],
                      [80.3, 130.2], [130.1, 130.4]])
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
    disc = selection(_abi.CS_SEL_CIRCLE, cx=108.0, cy=108.0, r=15.0)
    robot_ids = set(int(i) for i in robots[single])
    for numbers in ((0.5, 3.0, 1.0), (1.8, 1.0, limit)):
        want = _same(mesh, single, rec, grid, numbers, is_robot, None, cols, f"robots x everyone, {numbers}")
        assert all(int(r["a"]) in robot_ids or int(r["b"]) in robot_ids for r in want)
        if numbers[2] == limit:  # the four robots around the inner corner stand in four tiles and meet one another (still)
            corner = sorted(robot_ids)[:4]
            listed = list(zip(want["a"].tolist(), want["b"].tolist()))
            assert all((p, q) in listed for i, p in enumerate(corner) for q in corner[i + 1:])
        _same(mesh, single, rec, grid, numbers, is_robot, is_crowd, cols, f"robots x crowd, {numbers}")
        _same(mesh, single, rec, grid, numbers, disc, disc, cols, f"A == B across the corner, {numbers}")
        _same(mesh, single, rec, grid, numbers, is_crowd, disc, cols, f"overlapping roles, {numbers}")
    want = encounters(rec, grid, 1.8, 1.0, limit, np.asarray(cols[2]) == lp_robots, None)
    assert mesh.encounters(1.8, 1.0, limit, Selection(local_planner=nolp)).tobytes() == want.tobytes()
    assert mesh.count_encounters(1.8, 1.0, limit, None, dict(local_planner=nolp)) == len(want) > 0
