"""Every agent that enters a timed leg on a tile mesh (cs_mesh_leg_intervals; NativeTileMesh.leg_intervals /
count_leg_intervals / free_intervals): every tile runs all legs against the agents it owns, its walk clipped to its owned
cells; the per-leg counts add and the rows are merged by (leg, id); the mesh gives the single engine's answer byte for
byte, which is also the restatement's (tests/leg_intervals_reference.py), whatever distance, speed_max and t1 are.  No halo
exchange is made for it: the next steps of the mesh are those of a mesh that never asked."""
import numpy as np
import pytest

from rmf_crowdsim_amd import LocationHash2D, Simulation, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from leg_intervals_reference import SIZE_MAX, agree, call, intervals, last_error, legs_array
from select_reference import selection
from test_gpu_agent_write import _add_crossing
from test_gpu_encounters_mesh import _crowd
from test_gpu_leg_conflicts_mesh import _cut_legs
from test_gpu_leg_intervals import check_long_listing, interval_legs, long_listing_alone, many_legs, thin

pytestmark = pytest.mark.gpu
INF = float("inf")


def _same(mesh, single, rec, grid, legs, distance, speed_max, sel=None, name=""):
    """mesh == single engine == restatement, listing and counting; `sel` is a rectangle (no ledger needed)"""
    want = agree(single, rec, grid, legs, distance, speed_max, sel, name=name + " (engine)")
    agree(mesh, rec, grid, legs, distance, speed_max, sel, name=name + " (mesh)", want=want)
    return want


def test_a_mesh_lists_the_intervals_as_one_engine():
    shape = (2, 2)
    pts, group, grid = _crowd()
    mesh = NativeTileMesh(LocationHash2D(**grid), shape, 1)
    twin = NativeTileMesh(LocationHash2D(**grid), shape, 1)
    single = Simulation(LocationHash2D(**grid))
    for t in (mesh, twin, single):
        _add_crossing(t, pts, group)
        for _ in range(40):
            t.step(0.05)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes() and (mesh.tile_counts() > 0).sum() == 4
    cell = grid["cell_size"]
    cuts_x = [round(int(grid["height"] / cell) / 2) * cell]
    cuts_y = [round(int(grid["width"] / cell) / 2) * cell]
    pace = float(np.median(np.hypot(rec["vx"].astype(np.float64), rec["vy"].astype(np.float64))))
    legs = interval_legs(rec, grid)
    for distance, speed_max in ((0.5, INF), (1.0, pace), (3.0, 2.0), (0.2, INF)):  # (3 m: wider than a halo of one cell)
        _same(mesh, single, rec, grid, legs, distance, speed_max, name=f"the legs, {(distance, speed_max)}")
    # legs along, across and on the cuts: rows of one leg come from agents on both sides of a cut
    legs = _cut_legs(cuts_x, cuts_y)
    pos = {int(r["id"]): (float(r["x"]), float(r["y"])) for r in rec}
    rows, counts = _same(mesh, single, rec, grid, legs, 0.5, 2.0, name="legs at the cuts")
    both = 0
    for k in np.nonzero(counts >= 2)[0]:
        xs = [pos[int(i)] for i in rows["id"][rows["leg"] == k]]
        both += len({x < cuts_x[0] for x, _ in xs}) == 2 or len({y < cuts_y[0] for _, y in xs}) == 2
    print(f"{both} legs at the cuts with rows from both sides of a cut")
    assert both >= 20  # (no tile alone gives their rows)
    # a prefix: cap below the count, nothing written beyond it, the counts whole
    for cap in (1, len(rows) // 2):
        got, per_leg, out = call(mesh, legs, 0.5, 2.0, cap=cap)
        assert got == len(rows) and per_leg.tobytes() == counts.tobytes()
        assert out[:cap].tobytes() == rows[:cap].tobytes() and (out[cap:].view(np.uint8) == 0xAB).all()
    # targets two tiles away, +inf
    far = selection(_abi.CS_SEL_RECT, x0=float(np.median(rec["x"])), y0=float(np.median(rec["y"])), x1=INF, y1=INF)
    _same(mesh, single, rec, grid, legs[::5], INF, INF, far, name="+inf, the far quarter")
    # refusals leave the mesh usable and write nothing
    bad = legs.copy()
    bad["vy"][5] = float("nan")
    for legs_, distance in ((bad, 0.2), (legs, -1.0)):
        n, per_leg, out = call(mesh, legs_, distance, 2.0, cap=8)
        assert n == SIZE_MAX and "leg_intervals" in last_error(mesh)
        assert (out.view(np.uint8) == 0xAB).all() and (per_leg.view(np.uint8) == 0xAB).all()
    assert "leg 5" in (call(mesh, bad, 0.2, 2.0), last_error(mesh))[1]
    # the Python surface of the mesh
    assert mesh.leg_intervals(legs, 0.5, 2.0).tobytes() == rows.tobytes()
    assert mesh.leg_intervals(legs, 0.5, 2.0, limit=9).tobytes() == rows[:9].tobytes()
    assert mesh.count_leg_intervals(legs, 0.5, 2.0).tobytes() == counts.tobytes()
    assert mesh.leg_intervals(legs[:0], 0.5, 2.0).shape == (0,)
    spots = np.column_stack([rec["x"][::101] + 0.4, rec["y"][::101]])
    assert mesh.free_intervals(spots, 0.5, 4.0, 0.5, 2.0) == single.free_intervals(spots, 0.5, 4.0, 0.5, 2.0)
    assert mesh.read_agents().tobytes() == rec.tobytes()
    # the next steps are those of a mesh that never asked
    for t in (mesh, twin):
        for _ in range(5):
            t.step(0.05)
    assert mesh.read_agents().tobytes() == twin.read_agents().tobytes()


def test_a_mesh_lists_two_to_the_17_legs_as_one_engine():
    """The long listing of tests/test_gpu_leg_intervals.py on 2 x 2 tiles: every tile sorts its own rows by keys whose
    leg half has 18 bits, and the four runs are merged by the same keys."""
    pts, group, grid = _crowd()
    mesh = NativeTileMesh(LocationHash2D(**grid), (2, 2), 1)
    single = Simulation(LocationHash2D(**grid))
    for t in (mesh, single):
        _add_crossing(t, pts, group)
        for _ in range(40):
            t.step(0.05)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    legs = many_legs(rec, grid)
    left = thin(single, rec, 7)
    assert thin(mesh, rec, 7).tobytes() == left.tobytes() and 250 <= len(left) <= 350
    counts = mesh.tile_counts().reshape(-1)
    assert (counts > 0).all() and int(counts.sum()) == len(left)
    want = long_listing_alone(left, grid, legs, 0.5, 2.0, "2 x 2 tiles")
    check_long_listing(single, left, grid, legs, 0.5, 2.0, "the engine", want)
    check_long_listing(mesh, left, grid, legs, 0.5, 2.0, "2 x 2 tiles", want)
    assert mesh.read_agents().tobytes() == left.tobytes()


def _two_rank_legs(rec, grid):
    legs = interval_legs(rec, grid)
    comb = np.linspace(5.0, 55.0, 26)
    across = legs_array(np.column_stack([np.full_like(comb, 20.0), comb]), (2.5, 0.0), 0.0, 8.0)  # over the cut at 30 m
    on_cut = legs_array(np.column_stack([np.full_like(comb, 30.0), comb]), (0.0, 0.0), 0.0, 6.0)
    return np.concatenate([legs, across, on_cut])


def _two_rank_answers(t, rec, grid):
    """per query: (the count listing everything, the rows' bytes, the counts' bytes, the count of a prefix, its bytes, the
    count and the counts of the count-only form)"""
    legs = _two_rank_legs(rec, grid)
    left = selection(_abi.CS_SEL_RECT, x0=0.0, y0=0.0, x1=30.0, y1=60.0)  # one rank's side
    out = []
    for distance, speed_max, sel in ((0.5, 2.0, None), (0.2, INF, None), (0.5, 2.0, left), (0.0, 2.0, None)):
        total = call(t, legs, distance, speed_max, sel, cap=0, rows=False)[0]
        n, per_leg, rows = call(t, legs, distance, speed_max, sel, cap=total, fill=0xEE)
        m, _, head = call(t, legs, distance, speed_max, sel, cap=total // 3, fill=0xEE)
        k, only, _ = call(t, legs, distance, speed_max, sel, cap=0, rows=False)
        out.append((n, rows.tobytes(), per_leg.tobytes(), m, head.tobytes(), k, only.tobytes()))
    return out


def _rank_lists_intervals(rank, world, port, out_path):
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
        before = mesh.read_agents()
        notes = {"before": before, "answers": _two_rank_answers(mesh, before, GRID)}
        legs = _two_rank_legs(before, GRID)
        notes["refused"] = call(mesh, legs, float("nan"), 2.0, cap=4)[0] == SIZE_MAX
        notes["python"] = mesh.leg_intervals(legs, 0.5, 2.0)
        for _ in range(10):
            mesh.count_leg_intervals(legs, 0.5, 2.0)
            mesh.step(0.05, report=False)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_give_the_rows_of_one_engine(tmp_path):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU: the counts and the rows travel through the
    host transport's gathers, every rank gets the whole answer, the single engine's, and steps on as it."""
    import pickle
    import torch.multiprocessing as mp
    from test_gpu_agent_write_mesh import GRID, _scene
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "intervals.pkl")
    procs = [ctx.Process(target=_rank_lists_intervals, args=(r, 2, 29823, out)) for r in range(2)]
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
    want = _two_rank_answers(single, before, GRID)
    legs = _two_rank_legs(before, GRID)
    rows, counts = intervals(before, GRID, legs, 0.5, 2.0)
    assert want[0][0] == len(rows) > 100 and want[0][1][:rows.nbytes] == rows.tobytes() and want[3][0] == 0
    assert want[0][2] == counts.tobytes() == want[0][6] and want[0][3] == want[0][5] == len(rows)
    x_of = dict(zip(before["id"].tolist(), before["x"].tolist()))
    sides = {(int(r["leg"]), x_of[int(r["id"])] < 30.0) for r in rows}
    assert sum((k, True) in sides and (k, False) in sides for k in range(len(legs))) >= 5  # (rows of both ranks in one leg)
    for _ in range(10):
        single.step(0.05, report=False)
    end = single.read_agents()
    for n in notes:
        assert n["before"].tobytes() == before.tobytes()
        assert n["answers"] == want and n["refused"]
        assert n["python"].tobytes() == rows.tobytes()
        assert len(end) > 400 and n["agents"].tobytes() == end.tobytes()
