"""Sending agents to goals by id in batches on a tile mesh (cs_mesh_set_targets, NativeTileMesh.set_targets): the
positions of all entries are gathered, every tile runs the book part for the whole batch in batch order, so that every
tile's route book numbers routes alike, and assigns to the agents it owns.  The mesh stays equal to one engine, bit for
bit, in process and over two ranks of a host transport."""
import numpy as np
import pytest

from rmf_crowdsim_amd import (CrowdSimError, HighLevelPlanner, LocationHash2D, NoLocalPlan,
                              RouteFollower, Simulation, _abi)
from rmf_crowdsim_amd.tiles import NativeTileMesh
from set_targets_scenes import EXITS, Host, lattice, run_dispatch
from test_oracle_reference_kats import DoglegRoutes

pytestmark = pytest.mark.gpu
CS_CFG_TILE_OVERLAP = _abi.CS_CFG_TILE_OVERLAP
BOOKED, PLANNED, FORWARDED = 1, 2, 4


def _mesh(tiles=(2, 2), flags=0):
    return lambda index, **kw: NativeTileMesh(index, tiles, 1, flags=flags, **kw)


_single = {}


def _single_dispatch():
    if "run" not in _single:
        _single["run"] = run_dispatch(Simulation, False)
    return _single["run"]


@pytest.mark.parametrize("flags", [0, CS_CFG_TILE_OVERLAP])
def test_the_dispatch_on_a_mesh_equals_one_engine(flags):
    """The NoLocalPlan dispatch scene on a 2 x 2 mesh: statuses equal, the crowd bitwise equal after 180 steps, every
    tile plans what the single engine plans, in its order (the one Python planner is registered with all four tiles:
    its log of a batch is the single engine's log of that batch, once per tile), agents that cross a cut afterwards
    keep their route."""
    one = _single_dispatch()
    mesh = run_dispatch(_mesh(flags=flags), False)
    assert mesh.statuses == one.statuses
    assert mesh.statuses.count(PLANNED) > 1000 and mesh.statuses.count(BOOKED) > 1000
    lo_m = lo_1 = 0
    for hi_m, hi_1 in zip(mesh.marks, one.marks):
        assert hi_1 > lo_1 and mesh.routes.calls[lo_m:hi_m] == 4 * one.routes.calls[lo_1:hi_1]
        lo_m, lo_1 = hi_m, hi_1
    a, b = mesh.sim.read_agents(), one.sim.read_agents()
    assert len(a) == 1600 and a.tobytes() == b.tobytes()
    start = lattice(40, 40, 1.6, (40.0, 40.0), 0.15, 5)
    crossed = ((start[:, 0] < 80.0) != (a["x"] < 80.0)) | ((start[:, 1] < 80.0) != (a["y"] < 80.0))
    print(f"mesh dispatch (flags {flags}): {int(crossed.sum())} agents crossed a cut, tiles hold "
          f"{mesh.sim.tile_counts().tolist()}")
    assert crossed.sum() > 100
    # (an in-process mesh makes no exchange ahead: what set_targets does to one is
    # test_set_targets_voids_an_exchange_made_ahead)


# ---- CS_CFG_TILE_OVERLAP: an exchange made ahead is void after the call -------------------------------------------
def _middle_tile_runs(out_path):
    """The set-up of test_gpu_tiles.py's middle tile: one tile engine in the middle of the grid whose XLO / XHI peers are
    this rank itself, stepped with cs_tile_step_rccl, which under CS_CFG_TILE_OVERLAP makes the next step's exchange
    ahead on the second stream.  The crowd keeps clear of the bands along those edges (straight routes along y), so the
    buffers travel empty and the overlapped schedule must give the plain one's bits."""
    import pickle
    import torch
    from rmf_crowdsim_amd import Zanlungo, scenes
    from rmf_crowdsim_amd.tiles import RECORD, XHI, XLO
    torch.cuda.set_device(0)
    side = torch.cuda.Stream()
    grid = dict(width=60.0, height=60.0, cell_size=2.0, offset=(0.0, 0.0))
    pts = scenes.jittered_lattice(900, 0.63, (25.0, 6.0), 0.2, 3, columns=16)

    def run(flags, resend):
        with torch.cuda.stream(side):
            sim = Simulation(LocationHash2D(**grid), device=0, stream=side.cuda_stream, tile=(10, 20, 0, 30), halo_cells=1,
                             flags=flags)
            cap = 1024
            keep = {d: (torch.zeros((cap + 1) * RECORD, dtype=torch.uint8, device="cuda"),
                        torch.zeros((cap + 1) * RECORD, dtype=torch.uint8, device="cuda")) for d in (XLO, XHI)}
            for d, (s_, r_) in keep.items():
                sim.halo_set_buffers(d, s_.data_ptr(), r_.data_ptr(), cap)
            sim.rccl_comm_init(1, 0, sim.rccl_unique_id())
            sim.halo_set_peers([0, 0, -1, -1, -1, -1, -1, -1])
            calls = []

            def straight(start, goal):
                calls.append((start, goal))
                return [start, goal]
            # (hash cells of 5 cm: every agent plans a route of its own and walks straight along y, nobody converges)
            hlp = RouteFollower(straight, scale=0.05, arrive=0.1, speed=0.3)
            ids = sim.add_agents(pts, hlp, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
            statuses = [sim.set_targets(ids, pts + (0.0, 12.0)).tolist()]  # (before the first step: nothing made ahead yet)
            for k in range(60):
                sim.tile_step_rccl(0.05)
                if resend and k == 30:
                    statuses.append(sim.set_targets(ids[::2], pts[::2] + (0.0, -6.0)).tolist())
            side.synchronize()
            out = sim.read_agents()
            stats = (sim.kernel_stat(_abi.CS_STAT_EXCHANGES_AHEAD), sim.kernel_stat(_abi.CS_STAT_EXCHANGES_AHEAD_USED))
            del sim
        return out, stats, statuses, len(calls)
    runs = {(flags, resend): run(flags, resend) for flags in (0, CS_CFG_TILE_OVERLAP) for resend in (False, True)}
    with open(out_path, "wb") as f:
        pickle.dump(runs, f)


def test_set_targets_voids_an_exchange_made_ahead(tmp_path):
    """Route state travels in halo records, so a batch between two steps voids the exchange that the step before made
    ahead (CS_CFG_TILE_OVERLAP): it is repeated on the engine's stream.  Against the same run without that batch, one
    exchange more was made ahead and not used; the result has the bits of the plain schedule."""
    import pickle
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "middle.pkl")
    p = ctx.Process(target=_middle_tile_runs, args=(out,))  # (a fresh process: its own RCCL communicator)
    p.start()
    p.join(240)
    if p.is_alive():
        p.terminate()
        p.join(10)
    assert p.exitcode == 0
    with open(out, "rb") as f:
        runs = pickle.load(f)
    (plain, plain_stats, plain_st, _), (ahead, ahead_stats, ahead_st, _) = runs[(0, True)], runs[(CS_CFG_TILE_OVERLAP, True)]
    (still, still_stats, _, _), (quiet, quiet_stats, _, _) = runs[(0, False)], runs[(CS_CFG_TILE_OVERLAP, False)]
    print(f"exchanges ahead (made, used): with the batch {ahead_stats}, without {quiet_stats}; plain {plain_stats}")
    assert plain_stats == (0, 0) and still_stats == (0, 0)
    assert quiet_stats[0] >= 50 and ahead_stats[0] >= 50
    assert (ahead_stats[0] - ahead_stats[1]) == (quiet_stats[0] - quiet_stats[1]) + 1
    assert len(plain) == 900 and plain.tobytes() == ahead.tobytes() and still.tobytes() == quiet.tobytes()
    assert plain_st == ahead_st and len(plain_st) == 2 and set(plain_st[1]) <= {BOOKED, PLANNED}
    assert plain.tobytes() != still.tobytes()  # (the batch turned half the crowd round)
    assert plain["x"].min() > 24.0 and plain["x"].max() < 36.0  # (clear of the bands along the x edges)


class Listening(HighLevelPlanner):
    def __init__(self):
        self.targets = []

    def get_desired_velocity(self, agent, time):
        return (0.0, 0.25)

    def set_target(self, agent, point, tolerance):
        self.targets.append((agent.agent_id, tuple(agent.position), tuple(point), tuple(tolerance)))


def test_refused_batches_and_host_planners_on_a_mesh():
    def build(cls):
        h = Host(cls, False, scale=4.0)
        h.heard = Listening()
        h.ids = h.sim.add_agents(lattice(16, 16, 1.6, (68.0, 68.0), 0.15, 3), h.hlp, NoLocalPlan(), 2.0)
        h.led = h.sim.add_agents(lattice(4, 4, 1.6, (77.0, 77.0), 0.0, 0), h.heard, NoLocalPlan(), 2.0)  # on all four tiles
        h.sim.step(0.1)
        return h
    mesh, one = build(_mesh()), build(Simulation)
    batch = mesh.led[::-1] + mesh.ids[::2]
    goals = np.array([EXITS[k % 4] for k in range(len(batch))], dtype=np.float64)
    for bad_ids, bad_goals, why in ((batch + [10 ** 9], np.vstack([goals, goals[:1]]), "unknown agent id"),
                                    (batch, np.vstack([goals[:-1], [[np.nan, 0.0]]]), "not finite")):
        with pytest.raises(CrowdSimError, match=why):
            mesh.sim.set_targets(bad_ids, bad_goals)
    assert mesh.routes.calls == [] and mesh.heard.targets == []
    sm = [int(s) for s in mesh.sim.set_targets(batch, goals, tolerance=(0.5, 0.25))]
    so = [int(s) for s in one.sim.set_targets(batch, goals, tolerance=(0.5, 0.25))]
    assert sm == so and sm[:16] == [FORWARDED] * 16 and PLANNED in sm and BOOKED in sm
    assert mesh.routes.calls == 4 * one.routes.calls
    # the host planner hears every one of its agents once, from the tile that owns it, in batch order
    assert mesh.heard.targets == one.heard.targets and len(one.heard.targets) == 16
    for _ in range(40):
        mesh.sim.step(0.1)
        one.sim.step(0.1)
    assert mesh.sim.read_agents().tobytes() == one.sim.read_agents().tobytes()
    assert len(mesh.sim.set_targets([], np.zeros((0, 2)))) == 0


def test_route_follower_set_target_forwards_to_the_mesh():
    mesh = Host(_mesh(), False, scale=4.0)
    ids = mesh.sim.add_agents([(79.0, 79.0), (81.0, 81.0)], mesh.hlp, NoLocalPlan(), 2.0)
    agents = mesh.sim.agents
    assert mesh.hlp.set_target(agents[ids[0]], EXITS[2], (0.0, 0.0)) == PLANNED
    assert mesh.hlp.set_target(agents[ids[1]], EXITS[2], (0.0, 0.0)) == BOOKED
    assert mesh.routes.calls == 4 * [((79.0, 79.0), EXITS[2])]


# ---- two ranks over a host transport --------------------------------------------------------------------------------
def _two_rank_scene(t):
    routes = DoglegRoutes()
    hlp = RouteFollower(routes, scale=4.0, arrive=0.1, speed=1.2)
    ids = t.add_agents(lattice(24, 24, 1.6, (61.0, 61.0), 0.15, 5), hlp, NoLocalPlan(), 2.0)
    return routes, ids


def _two_rank_batches(ids):
    rng = np.random.default_rng(31)
    first = (list(ids), [EXITS[i % 4] for i in ids])
    some = rng.choice(ids, len(ids) // 2, replace=False).tolist()
    return first, (some, [EXITS[(i + 1) % 4] for i in some])


def _rank_sends(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import TorchHostTransport
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mesh = NativeTileMesh(LocationHash2D(160.0, 160.0, 2.0, (0.0, 0.0)), (2, 1), 1, device=0, rank=rank, n_ranks=world,
                              host_transport=TorchHostTransport(dist))
        routes, ids = _two_rank_scene(mesh)
        first, second = _two_rank_batches(ids)
        notes = {"st": [mesh.set_targets(*first).tolist()]}
        for _ in range(40):
            mesh.step(0.1, report=False)
        bad = np.asarray(second[0] + [10 ** 9], dtype=np.uint64)
        xy = np.ascontiguousarray(np.asarray(second[1] + [EXITS[0]], dtype=np.float64))
        C = mesh._C
        notes["refused_rc"] = int(mesh._lib.cs_mesh_set_targets(
            mesh._mesh, bad.ctypes.data_as(C.POINTER(C.c_uint64)), xy.ctypes.data_as(C.POINTER(C.c_double)), len(bad), 0.0,
            0.0, None))
        notes["refused_calls"] = len(routes.calls)
        notes["st"].append(mesh.set_targets(*second).tolist())
        for _ in range(60):
            mesh.step(0.1, report=False)
        notes["agents"] = mesh.read_agents()
        notes["calls"] = list(routes.calls)
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_a_batch_is_sent_across_two_ranks_over_a_host_transport(tmp_path):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU (the set-up of
    test_gpu_agents_by_id_mesh.py): the batch's agents live on both ranks; both return the same statuses, refuse the
    same batch without planning, plan what one engine plans, and the whole crowd equals one engine's."""
    import pickle
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "sends.pkl")
    procs = [ctx.Process(target=_rank_sends, args=(r, 2, 29781, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)  # (each rank's run under its own time limit)
    stuck = [p for p in procs if p.is_alive()]
    for p in stuck:
        p.terminate()
        p.join(10)
    assert not stuck and [p.exitcode for p in procs] == [0, 0]
    notes = []
    for r in range(2):
        with open(f"{out}.{r}", "rb") as f:
            notes.append(pickle.load(f))
    single = Simulation(LocationHash2D(160.0, 160.0, 2.0, (0.0, 0.0)))
    routes, ids = _two_rank_scene(single)
    first, second = _two_rank_batches(ids)
    st = [single.set_targets(*first).tolist()]
    for _ in range(40):
        single.step(0.1, report=False)
    a = single.read_agents()
    assert (a["x"] < 80.0).any() and (a["x"] >= 80.0).any()
    planned_first = len(routes.calls)
    st.append(single.set_targets(*second).tolist())
    for _ in range(60):
        single.step(0.1, report=False)
    want = single.read_agents()
    assert st[1].count(PLANNED) > 20
    for n in notes:
        assert n["st"] == st and n["refused_rc"] == 2 and n["refused_calls"] == planned_first
        assert n["calls"] == routes.calls
        assert len(want) == 576 and n["agents"].tobytes() == want.tobytes()
