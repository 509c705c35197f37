"""The engine's kept buffers, regrown with results in them (rmf_crowdsim_amd/csrc/cs_device_mem.hip.inc): every kept
scratch is used small, regrown by a larger call and used again, the agent arrays are regrown by add_agents with live
agents in them (600 agents in the first capacity of 1,024, then 1,400 more), the crowd steps, and every call is
repeated.  Each result must equal, as bytes, that of an engine that made only the final calls on the same crowd, and whose
agent arrays never grew (capacity_hint).  Everything compared is ids, counts, sorted lists and f32 / f64 values from the
same kernels on the same input; no output here comes from floating-point atomics (agent_field is asked for counts only:
its velocity sums are f64 atomic adds, whose order may differ)."""
import numpy as np
import pytest

from rmf_crowdsim_amd import LocationHash2D, Simulation, StubHighLevelPlan, Zanlungo, scenes

pytestmark = pytest.mark.gpu

GRID = dict(width=32.0, height=32.0, cell_size=1.0, offset=(0.0, 0.0))
N_FIRST, N_MORE, STEPS, DT, CREEP = 600, 1400, 5, 0.05, scenes.CREEP_SPEED


def positions():
    """2,000 distinct points of a jittered 50 x 40 lattice inside (1, 31) x (1, 31), shuffled"""
    rng = np.random.default_rng(20261021)
    gx, gy = np.meshgrid(np.arange(50), np.arange(40), indexing="ij")
    pts = np.stack([1.2 + gx.ravel() * 0.59, 1.2 + gy.ravel() * 0.74], axis=1) + rng.uniform(-0.2, 0.2, (2000, 2))
    return pts[rng.permutation(2000)]


class Crowd:
    def __init__(self, capacity_hint=0):
        self.sim = Simulation(LocationHash2D(**GRID), capacity_hint=capacity_hint)
        self.lp = Zanlungo(*scenes.METRIC_ZANLUNGO)
        self.ids = []

    def add(self, pts, creep):
        """(the walking crowd of scenes.add_walking_crowd: everybody walks +x, the two batches creep past each other)"""
        self.ids += self.sim.add_agents(pts, StubHighLevelPlan((0.3, creep)), self.lp, 3.0)

    def walk(self):
        for _ in range(STEPS):
            self.sim.step(DT)


def small_calls(c):
    """each kept buffer at a small size -> the results (for the repeat: the same call twice gives the same bytes)"""
    sim = c.sim
    goals = np.zeros((8, 8), dtype=bool)
    goals[0, 7] = True
    vec, dist, stats = sim.solve_flow_field((0.0, 0.0), 4.0, goals, 1.3, density_weight=0.5, distance=True)
    pairs, d2 = sim.close_pairs(0.3, distances=True)
    return {"by_id": sim.read_agents_by_id(c.ids[:8]).tobytes(),
            "field": sim.agent_field((0.0, 0.0), 8.0, (4, 4)).tobytes(),
            "pairs": pairs.tobytes(), "pairs_d2": d2.tobytes(),
            "flow_vec": vec.tobytes(), "flow_dist": dist.tobytes(), "flow_reached": stats["reached"],
            "select": sim.select_agents(circle=(16.0, 16.0, 2.0)).tobytes()}


def final_calls(c):
    """... and at sizes that no small call's buffer holds"""
    sim = c.sim
    goals = np.zeros((48, 48), dtype=bool)
    goals[0, 47] = goals[40, 3] = True
    blocked = np.zeros((48, 48), dtype=bool)
    blocked[24, 5:43] = True
    vec, dist, stats = sim.solve_flow_field((0.0, 0.0), 32.0 / 48.0, goals, 1.3, blocked=blocked, density_weight=0.5,
                                            distance=True)
    pairs, d2 = sim.close_pairs(1.5, distances=True)
    by_id = sim.read_agents_by_id(c.ids[::-1])
    assert len(by_id) == len(c.ids) and len(pairs) > len(c.ids)  # (a list longer than any the small calls made)
    return {"by_id": by_id.tobytes(),
            "field": sim.agent_field((0.0, 0.0), 0.5, (64, 64)).tobytes(),
            "pairs": pairs.tobytes(), "pairs_d2": d2.tobytes(),
            "flow_vec": vec.tobytes(), "flow_dist": dist.tobytes(), "flow_reached": stats["reached"],
            "select": sim.select_agents(rect=(2.0, 2.0, 30.0, 30.0)).tobytes(),
            "agents": sim.read_agents().tobytes()}


def same(got, want, when):
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], f"{key} {when}"


def test_results_survive_the_regrowth_of_every_kept_buffer():
    pts = positions()
    assert len(pts) == N_FIRST + N_MORE
    grown = Crowd()
    try:
        # 600 agents: every buffer small, then regrown, then used again
        grown.add(pts[:N_FIRST], CREEP)
        bytes_0 = grown.sim.device_bytes
        small = small_calls(grown)
        bytes_small = grown.sim.device_bytes
        first = final_calls(grown)
        bytes_first = grown.sim.device_bytes
        assert bytes_0 < bytes_small < bytes_first  # (the scratches are counted: they grew both times)
        same(small_calls(grown), small, "repeated in the regrown buffers")
        # 1,400 more: the agent arrays regrow with the 600 in them; the crowd walks; every call again
        grown.add(pts[N_FIRST:], -CREEP)
        assert grown.sim.device_bytes > bytes_first
        grown.walk()
        small_calls(grown)
        second = final_calls(grown)
        assert len(second["agents"]) > len(first["agents"]) and grown.sim.device_bytes > bytes_first
    finally:
        grown.sim.close()

    only_first = Crowd()  # the 600, the final calls only
    try:
        only_first.add(pts[:N_FIRST], CREEP)
        same(first, final_calls(only_first), "with 600 agents")
    finally:
        only_first.sim.close()

    only_second = Crowd(capacity_hint=4096)  # the 2,000 in arrays that never grow, the final calls only
    try:
        only_second.add(pts[:N_FIRST], CREEP)
        only_second.add(pts[N_FIRST:], -CREEP)
        only_second.walk()
        same(second, final_calls(only_second), "with 2,000 agents after the steps")
    finally:
        only_second.sim.close()
