"""The force pass of the tiled step kernel skips terms that provably underflow to +0 (zanlungo_forward_vanishes and
forward_terms_vanish in the step kernel).  An agent passes the pre-test when |v| t_i reaches beyond its sight by more
than the distance at which exp2 underflows (160 D / log2(e) + 2R: 44.8 m for the metric scene's D = 0.4 m).  A lane
passes the per-entry check when no forward neighbour has the NaN direction (s == 0 or NaN).  Such lanes keep fx = fy = +0
without running the full loop; every other lane, and every NaN, comes from the unchanged loop.  The gather kernel
(flags = 1) does not take the short cut, so it is the bitwise yardstick; the f64 oracle checks the values.  Needs an
MI355X."""
import numpy as np
import pytest

from oracle_sim import OracleSimulation
from rmf_crowdsim_amd import LocationHash2D, Simulation, StubHighLevelPlan, Zanlungo, scenes

pytestmark = pytest.mark.gpu

LP = scenes.METRIC_ZANLUNGO  # agent_scale, obstacle_scale, reaction_time, force_distance D, mass, radius R
EYESIGHT = 2.0
# |fut| (metres) from which the pre-test passes: (eyesight + 2R + 160 D / log2(e)) (1 + 2^-10)
PRETEST_M = (EYESIGHT + 2 * LP[5] + 160.0 * LP[3] / np.log2(np.e)) * (1.0 + 2.0 ** -10)


def max_rel_err(a, b, scale):
    assert (a["id"] == b["id"]).all()
    return float(np.hypot(a["x"] - b["x"], a["y"] - b["y"]).max() / scale)


def fut_lengths(a):
    """|v_i| t_i in metres per agent (f64, brute force): how far the force term looks ahead (zanlungo.rs:109-111)."""
    p = np.stack([a["x"], a["y"]], 1).astype(np.float64)
    v = np.stack([a["vx"], a["vy"]], 1).astype(np.float64)
    R = LP[5]
    T = np.full(len(a), np.inf)
    for i0 in range(0, len(a), 512):
        rp = p[None, :, :] - p[i0:i0 + 512, None, :]
        rv = v[None, :, :] - v[i0:i0 + 512, None, :]
        d2, aa, b = (rp ** 2).sum(-1), (rv ** 2).sum(-1), (rp * rv).sum(-1)
        c = d2 - R * R
        disc = b * b - aa * c
        with np.errstate(all="ignore"):
            t = (-b - np.sqrt(disc)) / aa
        t = np.where((aa > 0) & (disc >= 0) & (t > 0), t, np.inf)
        t = np.where(c < 0, 0.0, t)
        T[i0:i0 + 512] = np.where((d2 < EYESIGHT ** 2) & (d2 > 0), t, np.inf).min(1)
    return np.hypot(v[:, 0], v[:, 1]) * T


def walking_scene(cls, n, steps, flags=0, seed=7):
    """bench.py's default scene (scenes.add_walking_crowd), with room on the grid for `steps` steps of 0.05 s."""
    pts, grid, extent, group = scenes.uniform_crowd(n, seed=seed, cell_size=2.0,
                                                    room=scenes.WALK_SPEED * 0.05 * (steps + 10) + 4.0)
    sim = cls(LocationHash2D(**grid), flags=flags) if cls is Simulation else cls(LocationHash2D(**grid))
    scenes.add_walking_crowd(sim, pts, group, Zanlungo(*LP), EYESIGHT)
    return sim, extent


@pytest.mark.parametrize("n", [1_000_000, 125_000])
def test_walking_scene_tiled_equals_gather_bitwise(n):
    """The benchmark's scene, where every force term underflows: 60 steps, tiled == gather bit for bit, and the
    velocities stay exactly the preferred ones (forces exactly +0, as the gather kernel's full loop computes them)."""
    outs = []
    for flags in (2, 1):
        sim, _ = walking_scene(Simulation, n, 60, flags=flags)
        for k in range(60):
            sim.step(0.05, report=(k == 59))
        assert sim.last_report["n_tti_zero"] == 0 and sim.last_report["n_nonfinite"] == 0
        outs.append(sim.read_agents())
        del sim
    a, g = outs
    assert len(a) == n and a.tobytes() == g.tobytes()
    assert (a["vx"] == np.float32(scenes.WALK_SPEED)).all()
    assert (np.abs(a["vy"]) == np.float32(scenes.CREEP_SPEED)).all()


def straddle_scene(cls, walk, density, creeps, flags=0):
    """A walking crowd cut into strips along y; in strip k the two groups walk +x at walk +- creeps[k], so that
    |v| t_i ~ walk * gap / creep runs from well beyond the pre-test's threshold (whole waves of candidates) to well
    below it (real forces), with the strips near the threshold mixing candidates and non-candidates in one wave.
    The preferred velocities have no y component: vy = fy / m shows the force's bits, down to the smallest term."""
    pts, grid, extent, group = scenes.uniform_crowd(4000, seed=5, density=density, cell_size=2.0, room=6.0)
    sim = cls(LocationHash2D(**grid), flags=flags) if cls is Simulation else cls(LocationHash2D(**grid))
    lp = Zanlungo(*LP)
    y0, y1 = pts[:, 1].min(), pts[:, 1].max() + 1e-9
    strip = np.minimum(((pts[:, 1] - y0) / (y1 - y0) * len(creeps)).astype(int), len(creeps) - 1)
    order = []
    for k, c in enumerate(creeps):
        for gr, sign in ((0, 1.0), (1, -1.0)):
            sel = np.nonzero((strip == k) & (group == gr))[0]
            if len(sel):
                sim.add_agents(pts[sel], StubHighLevelPlan((walk + sign * c, 0.0)), lp, EYESIGHT)
                order.append(sel)
    return sim, extent, strip[np.concatenate(order)]  # the strip of each agent, in id order


@pytest.mark.parametrize("walk,density,k_gap", [(1.3, 2.5, 0.23), (0.5, 2.5, 0.23), (1.3, 1.0, 0.41), (2.0, 1.0, 0.41)],
                         ids=["walk1.3-dense", "walk0.5-dense", "walk1.3-sparse", "walk2.0-sparse"])
def test_threshold_straddle_matches_gather_and_oracle(walk, density, k_gap):
    """|fut| on both sides of the pre-test's threshold, for several walking speeds and spacings (k_gap: the typical
    approaching gap over which t_i is measured, in metres, for the density).  Tiled == gather bit for bit over 30 steps,
    both within 1e-4 of the extent of the f64 oracle; the scene really straddles the threshold (computed in f64)."""
    creeps = walk * k_gap / np.geomspace(150.0, 20.0, 8)  # median |fut| from 150 m down to 20 m
    runs = {}
    for name, cls, flags in (("tiled", Simulation, 2), ("gather", Simulation, 1), ("oracle", OracleSimulation, 0)):
        sim, extent, strip = straddle_scene(cls, walk, density, creeps, flags)
        for k in range(30):
            sim.step(0.05)
            if k == 1 and name == "oracle":
                fut = fut_lengths(sim.read_agents())
        assert sim.last_report["n_tti_zero"] == 0
        runs[name] = sim.read_agents()
    fin = np.isfinite(fut)
    passing = fut[fin] >= PRETEST_M
    print(f"walk {walk} density {density}: {fin.mean():.3f} with a finite t_i, {passing.mean():.3f} of them beyond "
          f"{PRETEST_M:.1f} m; per strip " + " ".join(f"{(fut[fin & (strip == k)] >= PRETEST_M).mean():.2f}" for k in range(8)))
    assert 0.15 <= passing.mean() <= 0.85
    assert (fut[fin & (strip == 0)] >= PRETEST_M).mean() >= 0.9 and (fut[fin & (strip == 7)] >= PRETEST_M).mean() <= 0.1
    a, g, b = runs["tiled"], runs["gather"], runs["oracle"]
    assert a.tobytes() == g.tobytes()
    # The f64 oracle meets one of the reference's ill-conditioned spots (exact cancellation of the
    # predicted separation for walkers in file) for ~1 % of the far-sighted walkers, which turn NaN there; the engine's
    # f32 terms underflow to +0 first.  The values are compared where the oracle is finite.
    ok = np.isfinite(b["x"])
    assert np.isfinite(a["x"]).all() and ok.mean() >= 0.98
    assert max_rel_err(a[ok], b[ok], extent) <= 1e-4
    # the far-sighted strip has exactly +0 forces, the near-sighted one tiny non-zero ones (1e-20 m/s and less)
    assert (a["vy"][strip == 0] == 0.0).mean() >= 0.95 and (a["vy"][strip == 7] != 0.0).mean() >= 0.5


def defect_scene(flags, creep):
    """A walking crowd (whole waves of candidates when creep > 0, t_i = inf for everybody when creep = 0) with:
    two walkers at one position inside it (a candidate whose forward entry has d2 = 0: s = 0, the NaN direction);
    an agent thrown at 1e10 m/s inside it (its window takes the guarded time-to-collision pass: tile_huge); apart
    from it a standing agent overlapped by a creeping one (t_i = 0 at zero speed: the 0/0 NaN of zanlungo.rs:163),
    a parallel pair at 1e13 m/s (|v| t_i overflows f32: the pre-test passes on an infinite |fut|^2) and a lone agent
    (t_i = inf)."""
    pts, grid, extent, group = scenes.uniform_crowd(3000, seed=9, cell_size=2.0, room=12.0)
    sim = Simulation(LocationHash2D(**grid), flags=flags)
    lp = Zanlungo(*LP)
    scenes.add_walking_crowd(sim, pts, group, lp, EYESIGHT, creep=creep)
    mid = pts[len(pts) // 2]
    sim.add_agents([mid + (0.31, 0.07), mid + (0.31, 0.07)], StubHighLevelPlan((scenes.WALK_SPEED, creep)), lp, EYESIGHT)
    sim.add_agents([pts[len(pts) // 3] + (0.3, 0.3)], StubHighLevelPlan((1e10, 0.0)), lp, EYESIGHT)
    far = np.array([pts[:, 0].max() + 6.0, pts[:, 1].min() + 2.0])
    sim.add_agents([far], StubHighLevelPlan((0.0, 0.0)), lp, EYESIGHT)
    sim.add_agents([far + (0.15, 0.0)], StubHighLevelPlan((-0.001, 0.0)), lp, EYESIGHT)
    sim.add_agents([far + (0.0, 6.0)], StubHighLevelPlan((1e13, 0.001)), lp, EYESIGHT)
    sim.add_agents([far + (0.0, 7.0)], StubHighLevelPlan((1e13, -0.001)), lp, EYESIGHT)
    sim.add_agents([far + (0.0, 12.0)], StubHighLevelPlan((0.3, 0.0)), lp, EYESIGHT)
    return sim


@pytest.mark.parametrize("creep", [scenes.CREEP_SPEED, 0.0], ids=["walking", "equal-velocities"])
def test_nan_and_zero_cases_match_gather_bitwise(creep):
    """Steps of 1e-18 s (whoever is thrown stays on the grid): tiled == gather bit for bit, NaN bits included."""
    outs, reps = [], []
    for flags in (2, 1):
        sim = defect_scene(flags, creep)
        for _ in range(3):
            sim.step(1e-18)
        outs.append(sim.read_agents())
        reps.append((sim.last_report["n_tti_zero"], sim.last_report["n_nonfinite"]))
    a, g = outs
    assert reps[0] == reps[1]
    assert a.tobytes() == g.tobytes()
    n = len(a)
    # (a NaN velocity leaves a NaN position behind; the agent is binned to cell 0, sees nobody and walks at v_pref again)
    if creep > 0.0:  # the pair at one position (3000, 3001): the lower id has the other as a forward entry, d2 = 0
        assert np.isnan(a["x"][3000]) or np.isnan(a["y"][3000])
    # the standing agent overlapped at zero speed (3003): 0/0
    assert np.isnan(a["x"][3003]) or np.isnan(a["y"][3003])
    assert np.isfinite(a["vx"][n - 1]) and a["vx"][n - 1] == np.float32(0.3)  # the lone agent: no force
    if creep == 0.0:  # equal velocities far from the defects: t_i = inf, v = v_pref
        assert (a["vx"][:1000] == np.float32(scenes.WALK_SPEED)).mean() > 0.9


@pytest.mark.parametrize("scene", ["creep", "random"])
def test_full_force_scenes_stay_bitwise_equal_to_gather(scene):
    """Crowds whose forces do not underflow (hardly any candidate) run the unchanged loop: tiled == gather."""
    outs = []
    for flags in (2, 1):
        if scene == "creep":
            pts, grid, extent, group = scenes.uniform_crowd(125_000, seed=7, cell_size=2.0)
        else:
            pts, grid, extent, group = scenes.random_crowd(100_000, seed=7, cell_size=2.0)
        sim = Simulation(LocationHash2D(**grid), flags=flags)
        scenes.add_counterflow(sim, pts, group, scenes.CREEP_SPEED, Zanlungo(*LP), EYESIGHT)
        for _ in range(20):
            sim.step(0.05, report=False)
        outs.append(sim.read_agents())
    assert outs[0].tobytes() == outs[1].tobytes()


def test_the_fast_path_runs(tmp_path):
    """Every test above would also pass with the short cut switched off.  This one builds the diagnostic engine
    (-DCS_TILE_TRIPS, the counters tools/trip_counts.py reports) and asserts that the walking crowd takes the fast path
    on every lane with a finite t_i and skips the full force loop in its waves, and that the creep scene (real forces)
    does not take it."""
    import json
    import os
    import subprocess
    import sys
    from rmf_crowdsim_amd import _native
    lib = str(tmp_path / "trips.so")
    subprocess.run([_native._hipcc()] + _native.HIPCC_FLAGS + ["-DCS_TILE_TRIPS", "-I", os.path.join(_native.REPO_ROOT, "include"),
                    "-o", lib, os.path.join(_native.CSRC, "crowdstep_hip.hip")], check=True, capture_output=True, timeout=600)
    stats = {}
    for scene in ("walk", "creep"):
        out = subprocess.run([sys.executable, os.path.join(_native.REPO_ROOT, "tools", "trip_counts.py"), scene, "60000"],
                             env={**os.environ, "CS_LIB_PATH": lib}, capture_output=True, text=True, timeout=300,
                             check=True).stdout
        print(out)
        line = [l for l in out.splitlines() if l.startswith("SCENE_STATS ")][0]
        stats[scene] = next(iter(json.loads(line[len("SCENE_STATS "):]).values()))
    walk, creep = stats["walk"], stats["creep"]
    assert walk["finite_ttc_frac"] > 0.5 and walk["force_pretest_entry_frac"] > 0.999
    assert walk["force_fast_lane_frac"] > 0.999 and walk["force_fast_wave_frac"] > 0.5
    assert walk["force_trips_per_wave"] < 0.05  # (the full loop's trips after the short cut)
    assert creep["force_fast_lane_frac"] < 0.01 and creep["force_trips_per_wave"] > 10.0
