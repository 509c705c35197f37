"""The tiled step kernel finishes a listed pair's time to collision (root, reciprocal, case analysis) only where the
result can be finite: its lean pass stops at the discriminant and marks a pair as done when disc < 0, or disc == 0 with
bh == 0 (ttc_skip_key; the rule itself: tests/test_ttc_live_exact.py), and a second loop finishes the others.  A wave
takes that split form when all its agents walk at exactly their preferred velocity, the one-pass loop otherwise.  Whatever
is skipped or finished, the bits must be those of the gather kernel (flags = 1), which finishes every pair.  The cases
sit where the split could go wrong: lists that are mostly skipped and mostly finished, a discriminant of exactly zero
on either side of the rule, an overlapping pair (the guarded repeat), lists that cross the 32-entry word and are odd,
lists beyond the LDS rows, a thrown agent in the tile.  All grids are 8 x 8 cells of 2 m, eyesight 2 m.  Needs an MI355X."""
import numpy as np
import pytest

from rmf_crowdsim_amd import LocationHash2D, Simulation, StubHighLevelPlan, Zanlungo, _abi, scenes

pytestmark = pytest.mark.gpu

GRID = dict(width=16.0, height=16.0, cell_size=2.0, offset=(0.0, 0.0))
LP = scenes.METRIC_ZANLUNGO
UNITS = 2.0 ** 22  # fixed units per metre at a cell of 2 m (cs_fix = 2^23 per cell)
STEPS = 3


def lattice_512():
    """the bench's walking lattice (2.5 agents / m^2, jittered), 512 agents inside the 16 m grid"""
    pts, _, extent, group = scenes.uniform_crowd(512, seed=7, cell_size=2.0, margin=0.75)
    assert pts.min() > 0.5 and pts.max() < 15.5 and extent < 14.6
    return pts, group


def both_kernels(build, dt=0.05, steps=STEPS, flags=0, before_step=None):
    """build(sim) adds the agents; returns [(agents, reports)] for the tiled (flags 2) and the gather kernel (flags 1)"""
    out = []
    for kernel in (_abi.CS_CFG_FORCE_TILED, _abi.CS_CFG_FORCE_GATHER):
        sim = Simulation(LocationHash2D(**GRID), flags=kernel | flags)
        build(sim)
        sim.step(0.0)  # velocities are (0, 0) until a step has set them; nobody moves
        reps = []
        for k in range(steps):
            if before_step is not None:
                before_step(sim, k)
            sim.step(dt)
            reps.append(dict(sim.last_report))
        out.append((sim.read_agents(), reps))
    return out


def assert_same(out):
    (a, ra), (g, rg) = out
    assert len(a) == len(g) and a.tobytes() == g.tobytes()
    assert ra == rg  # last_report of every step, field for field


def random_velocities(seed, speed=1.0):
    """writes every agent a velocity of ~`speed` m/s in a seeded random direction before each step"""
    def write(sim, k):
        a = sim.read_agents()
        rng = np.random.default_rng(seed + k)
        ang = rng.uniform(0.0, 2.0 * np.pi, len(a))
        mag = speed * rng.uniform(0.7, 1.3, len(a))
        a["vx"], a["vy"] = mag * np.cos(ang), mag * np.sin(ang)
        sim.write_agents(a, "velocity")
    return write


def own_velocities(pts, seed, speed=1.0):
    """every agent walks at a preferred velocity of its own (~`speed` m/s, a seeded random direction) and is put back to
    exactly that velocity before each step: a wave of agents at their preferred velocities, which is what takes the
    split form, with relative velocities of every direction.  Returns (build, before_step)."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0.0, 2.0 * np.pi, len(pts))
    mag = speed * rng.uniform(0.7, 1.3, len(pts))
    vel = np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)

    def build(sim):
        lp = Zanlungo(*LP)
        for p, v in zip(pts, vel):  # ids ascend in this order
            sim.add_agents([tuple(p)], StubHighLevelPlan((float(v[0]), float(v[1]))), lp, 2.0)

    def write(sim, k):
        a = sim.read_agents()
        a["vx"], a["vy"] = vel[:, 0], vel[:, 1]
        sim.write_agents(a, "velocity")
    return build, write


def test_walking_counterflow_mostly_skipped():
    """(a) 512 agents walking +x at 1.3 m/s, the groups creeping against each other in y: a neighbour of the own group
    has rv == 0 (disc == 0, bh == 0), one of the other group misses unless it stands in the agent's own column."""
    pts, group = lattice_512()
    out = both_kernels(lambda sim: scenes.add_walking_crowd(sim, pts, group, Zanlungo(*LP), 2.0))
    assert_same(out)
    assert out[1][1][-1]["n_nonfinite"] == 0 and len(out[0][0]) == 512


def test_random_velocities_mostly_finished():
    """(b) the same crowd with velocities of ~1 m/s in random directions, written before every step: relative
    velocities of every size and direction, many pairs on a collision course, and nobody at its preferred velocity:
    the waves take the one-pass loop.  (Forces of 10 - 20 m/s at this density: steps of 0.2 ms, so that nobody is
    carried into anybody within the three of them.)"""
    pts, group = lattice_512()
    out = both_kernels(lambda sim: scenes.add_walking_crowd(sim, pts, group, Zanlungo(*LP), 2.0), dt=2e-4,
                       before_step=random_velocities(100))
    assert_same(out)
    a = out[1][0]
    # the forces are real: many agents are off their preferred velocity (1.3, +-0.001)
    off_pref = np.hypot(a["vx"] - scenes.WALK_SPEED, np.abs(a["vy"]) - scenes.CREEP_SPEED)
    print(f"agents off their preferred velocity by more than 1 mm/s: {(off_pref > 1e-3).mean():.2f}")
    assert (off_pref > 1e-3).mean() > 0.2


def disc_of(pi, pj, vi, vj, R):
    """a, bh, c, disc of agent i looking at j as the kernels form them: f32, positions in fixed units"""
    f = np.float32
    rpx, rpy = f((pj[0] - pi[0]) * UNITS), f((pj[1] - pi[1]) * UNITS)
    rvx, rvy = f(f(vj[0]) - f(vi[0])), f(f(vj[1]) - f(vi[1]))
    Rs = f(f(R) * f(UNITS))
    d2 = f(np.float64(rpx) * np.float64(rpx) + np.float64(f(rpy * rpy)))
    c = f(d2 - f(Rs * Rs))
    a = f(np.float64(rvx) * np.float64(rvx) + np.float64(f(rvy * rvy)))
    bh = f(np.float64(rvx) * np.float64(rpx) + np.float64(f(rvy * rpy)))
    disc = f(np.float64(bh) * np.float64(bh) - np.float64(f(a * c)))
    return a, bh, c, disc


def test_grazing_pair_with_a_zero_discriminant_is_finished():
    """(c) R = 0.25 m is 2^20 fixed units; two agents 0.25 m apart across their paths and 1 m apart along them walk
    head-on at 0.5 m/s each: rv = (0, -+1), a = 1, bh = -+2^22, c = 2^44, disc = 2^44 - 2^44 = 0 exactly, bh != 0.  The
    pair grazes after 1 s; the yielding agent feels the force."""
    R = 0.25
    pi, pj, vi, vj = (5.0, 5.0), (5.25, 6.0), (0.0, 0.5), (0.0, -0.5)
    a, bh, c, disc = disc_of(pi, pj, vi, vj, R)
    assert disc == 0.0 and bh == -UNITS and a == 1.0 and c == 2.0 ** 44
    lp = Zanlungo(*LP[:5], R)

    def build(sim):
        sim.add_agents([pi], StubHighLevelPlan(vi), lp, 2.0)
        sim.add_agents([pj], StubHighLevelPlan(vj), lp, 2.0)
        sim.add_agents([(12.0, 12.0)], StubHighLevelPlan((0.0, 0.0)), lp, 2.0)
    out = both_kernels(build, steps=1)
    assert_same(out)
    g = out[1][0]
    assert g["vx"][0] != 0.0 and g["vy"][1] == -0.5  # the smaller id yields: a finite t_i, a force across its path
    assert_same(both_kernels(build))


def test_pair_with_equal_velocities_is_skipped():
    """(d) two agents 2 R apart (bodies touching) with the same velocity: rv == 0, a = bh = disc = 0: +inf, no force."""
    lp = Zanlungo(*LP[:5], 0.25)

    def build(sim):
        sim.add_agents([(5.0, 5.0), (5.5, 5.0)], StubHighLevelPlan((0.25, 0.5)), lp, 2.0)
    a, bh, c, disc = disc_of((5.0, 5.0), (5.5, 5.0), (0.25, 0.5), (0.25, 0.5), 0.25)
    assert a == 0.0 and bh == 0.0 and disc == 0.0 and c > 0.0
    out = both_kernels(build)
    assert_same(out)
    g = out[1][0]
    assert (g["vx"] == 0.25).all() and (g["vy"] == 0.5).all()


def test_overlapping_pair_takes_the_guarded_repeat():
    """(e) two agents 0.15 m apart (d2 < R2): colliding now in both kernels (n_tti_zero), whatever the lean pass marked.
    (Steps so short that whoever is thrown at 1e15 m/s stays on the grid.)"""
    lp = Zanlungo(*LP)

    def build(sim):
        sim.add_agents([(5.0, 5.0)], StubHighLevelPlan((0.3, 0.0)), lp, 2.0)
        sim.add_agents([(5.15, 5.01)], StubHighLevelPlan((0.0, 0.0)), lp, 2.0)
        sim.add_agents([(6.0, 5.5)], StubHighLevelPlan((-0.3, 0.1)), lp, 2.0)
        sim.add_agents([(12.0, 12.0)], StubHighLevelPlan((0.0, 0.0)), lp, 2.0)
    out = both_kernels(build, dt=1e-18, steps=2)
    assert_same(out)
    assert out[0][1][0]["n_tti_zero"] == 2 and out[1][1][0]["n_tti_zero"] == 2


def cluster(centre, k, spacing=0.38, reach=1.9):
    """the centre and the k sites of a square lattice nearest to it, all within `reach`: the centre sees exactly k"""
    n = int(np.ceil(reach / spacing))
    ij = np.array([(i, j) for i in range(-n, n + 1) for j in range(-n, n + 1) if (i, j) != (0, 0)], dtype=float)
    d = np.hypot(ij[:, 0], ij[:, 1]) * spacing
    order = np.argsort(d, kind="stable")[:k]
    assert d[order].max() < reach
    return np.concatenate([[centre], np.asarray(centre) + ij[order] * spacing])


def in_sight(pts, i, eyesight=2.0):
    d = np.hypot(pts[:, 0] - pts[i, 0], pts[:, 1] - pts[i, 1])
    assert (np.abs(d - eyesight) > 1e-3).all()  # nobody on the rim, where f32 could count differently
    return int((d < eyesight).sum()) - 1


def test_lists_across_the_word_boundary_and_odd(monkeypatch):
    """(f) four clusters whose centres see 32, 33, 62 and 63 others (33 / 34 / 63 / 64 list entries with the agent
    itself, which the lean filter lists too): entry 32 opens the second word of bits, odd lists repeat their last entry.
    64 LDS rows, so every list is walked by the lean pass.  Everybody at a random preferred velocity of its own: the
    split form, skipped and finished pairs mixed (forces of up to ~100 m/s in such clusters: steps of 0.1 ms)."""
    monkeypatch.setenv("CS_TILE_LIST_CAP", "64")
    parts = [cluster(c, k) for c, k in (((4.0, 4.0), 32), ((12.0, 4.0), 33), ((4.0, 12.0), 62), ((12.0, 12.0), 63))]
    pts = np.concatenate(parts)
    starts = np.cumsum([0] + [len(p) for p in parts[:-1]])
    assert [in_sight(pts, int(s)) for s in starts] == [32, 33, 62, 63]
    build, write = own_velocities(pts, 200)
    out = both_kernels(build, dt=1e-4, before_step=write)
    assert_same(out)
    # ... and the same lists in the one-pass loop (velocities written that are nobody's preferred ones)
    assert_same(both_kernels(build, dt=1e-4, before_step=random_velocities(201)))


def test_dense_lists_beyond_the_lds_rows(monkeypatch):
    """(g) CS_CFG_DENSE, 24 LDS rows: the cluster centres above hold up to 64 entries, the tail of every longer list
    lies in spilled rows and goes through the general loop behind the lean one."""
    monkeypatch.setenv("CS_TILE_LIST_CAP", "24")
    pts = np.concatenate([cluster((4.0, 4.0), 63), cluster((12.0, 12.0), 40), cluster((12.0, 4.0), 20)])
    assert in_sight(pts, 0) == 63
    build, write = own_velocities(pts, 300)
    assert_same(both_kernels(build, dt=1e-4, flags=_abi.CS_CFG_DENSE, before_step=write))


def test_a_thrown_agent_in_the_tile():
    """(h) one agent at 2^33 m/s among the walking crowd (beyond TTC_HUGE_SPEED: its tile repeats the pass in the
    guarded form).  dt = 0 commits the velocities and leaves everybody on the grid."""
    pts, group = lattice_512()
    # where it stands: 1 m behind an agent of the middle of the crowd, 5 cm beside its line, clear of everybody by 0.3 m
    # (no overlap: that is case (e)); that agent is in its path and has to yield (the newcomer has the largest id)
    spot = None
    for k in np.argsort(np.hypot(pts[:, 0] - 8.0, pts[:, 1] - 8.0)):
        cand = (pts[k, 0] - 1.0, pts[k, 1] + 0.05)
        if np.hypot(pts[:, 0] - cand[0], pts[:, 1] - cand[1]).min() > 0.3:
            spot = (float(cand[0]), float(cand[1]))
            break
    d = np.hypot(pts[:, 0] - spot[0], pts[:, 1] - spot[1])
    assert (d < 2.0).sum() >= 20

    def build(sim):
        scenes.add_walking_crowd(sim, pts, group, Zanlungo(*LP), 2.0)
        sim.add_agents([spot], StubHighLevelPlan((2.0 ** 33, 0.0)), Zanlungo(*LP), 2.0)
    out = both_kernels(build, dt=0.0)
    assert_same(out)
    g = out[1][0]
    assert g["vx"][-1] >= 2.0 ** 32
    print(f"agents pushed off their preferred velocity: {int((np.abs(g['vy'][:-1]) > 0.01).sum())}")
    assert (np.abs(g["vy"][:-1]) > 0.01).any()  # somebody in its path was pushed aside


# ---- case (a) on a 2 x 2 mesh, one rank per tile over gloo ---------------------------------------------------------
def _mesh_scene(target):
    pts, group = lattice_512()
    scenes.add_walking_crowd(target, pts, group, Zanlungo(*LP), 2.0)


def _mesh_rank(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import NativeTileMesh, TorchHostTransport
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 2), 1, device=0, rank=rank, n_ranks=world,
                              flags=_abi.CS_CFG_FORCE_TILED, host_transport=TorchHostTransport(dist))
        _mesh_scene(mesh)
        mesh.step(0.0, report=False)
        for k in range(STEPS):
            mesh.step(0.05, report=(k == STEPS - 1))
        a = mesh.read_agents()
        if rank == 0:
            with open(out_path, "wb") as f:
                pickle.dump(a, f)
    finally:
        dist.destroy_process_group()


def test_two_by_two_mesh_over_gloo_equals_one_engine(tmp_path):
    import pickle
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "mesh.pkl")
    procs = [ctx.Process(target=_mesh_rank, args=(r, 4, 29793, out)) for r in range(4)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    with open(out, "rb") as f:
        both = pickle.load(f)
    single = Simulation(LocationHash2D(**GRID), flags=_abi.CS_CFG_FORCE_GATHER)
    _mesh_scene(single)
    single.step(0.0, report=False)
    for _ in range(STEPS):
        single.step(0.05, report=False)
    a = single.read_agents()
    assert len(a) == 512 and a.tobytes() == both.tobytes()
