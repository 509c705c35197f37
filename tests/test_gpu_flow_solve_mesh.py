"""Solving a flow field on a tile mesh (cs_mesh_flow_field_solve; NativeTileMesh.solve_flow_field): an in-process 2 x 2 mesh
gives the single engine's distances and vectors, byte for byte, with the crowd's density (counted across the tiles, an
agent the index never took included); and a mesh whose planner is re-solved on the device after its third step steps as
the single engine does, by the comparison of tests/test_gpu_hlp_field_mesh.py."""
import numpy as np
import pytest

import flow_solve_reference as ref
from rmf_crowdsim_amd import CrowdSimError, FieldPlanner, LocationHash2D, Selection, Simulation, StubHighLevelPlan, Zanlungo, scenes
from rmf_crowdsim_amd.tiles import NativeTileMesh

pytestmark = pytest.mark.gpu

GRID = dict(width=32.0, height=32.0, cell_size=1.0, offset=(0.0, 0.0))
LP = Zanlungo(*scenes.METRIC_ZANLUNGO)


def test_a_mesh_solves_as_one_engine_with_density():
    origin, cell, shape = (-2.3, -1.7), (0.45, 0.4), (75, 96)
    blocked, goals = ref.random_walls(shape[0], shape[1], 9, 0.1, [(2, 2), (90, 70)])
    pts = scenes.jittered_lattice(500, 0.9, (3.0, 3.0), 0.1, 5)
    walkers, others = StubHighLevelPlan((0.1, 0.0)), StubHighLevelPlan((0.0, 0.1))
    mesh, single = NativeTileMesh(LocationHash2D(**GRID), (2, 2), 1), Simulation(LocationHash2D(**GRID))
    try:
        for t in (mesh, single):
            t.add_agents(pts[0::2], walkers, LP, 1.0)
            t.add_agents(pts[1::2], others, LP, 1.0)
            with pytest.raises(CrowdSimError):  # created, then refused by the index: it still counts
                t.add_agents([(40.0, 5.0)], walkers, LP, 1.0)  # (beyond the grid's last row)
        slow = np.random.default_rng(4).uniform(0.5, 4.0, shape).astype(np.float32)
        for sel in (None, Selection(high_level_planner=walkers, rect=(10.0, 0.0, 45.0, 30.0))):
            counts = single.agent_field(origin, cell, shape, sel)
            assert counts.tobytes() == mesh.agent_field(origin, cell, shape, sel).tobytes() and counts[int((5.0 + 1.7) / 0.4), int((40.0 + 2.3) / 0.45)] == 1
            want_vec, want_dist, reached, _ = ref.solve(blocked, goals, cell, 1.2, slowness=slow, counts=counts, density_weight=0.5)
            for t in (mesh, single):
                vec, dist, stats = t.solve_flow_field(origin, cell, goals, 1.2, blocked=blocked, slowness=slow,
                                                      density_weight=0.5, density_filter=sel, distance=True)
                assert dist.tobytes() == want_dist.tobytes() and vec.tobytes() == want_vec.tobytes()
                assert stats["reached"] == reached and stats["rounds"] >= 2
        # without density no raster of the crowd is made
        want_vec, want_dist, reached, _ = ref.solve(blocked, goals, cell, 1.2)
        vec, dist, stats = mesh.solve_flow_field(origin, cell, goals, 1.2, blocked=blocked, distance=True)
        assert dist.tobytes() == want_dist.tobytes() and vec.tobytes() == want_vec.tobytes() and stats["reached"] == reached
        with pytest.raises(CrowdSimError):
            mesh.solve_flow_field(origin, cell, goals, float("nan"), blocked=blocked)
        with pytest.raises(CrowdSimError):
            mesh.solve_flow_field(origin, cell, goals, 1.0, vectors=False)  # (nothing to write to)
    finally:
        single.close()
        mesh.__del__()


def _same(mesh, single, what):
    a, b = mesh.read_agents(), single.read_agents()
    assert a.tobytes() == b.tobytes(), what
    return b


def test_a_mesh_whose_planner_is_re_solved_steps_as_one_engine():
    blocked = np.zeros((64, 64), dtype=bool)
    blocked[:, 52] = True  # (x from 26 m: beyond the crowd, nobody stands on a wall bin)
    blocked[14:18, 52] = blocked[44:48, 52] = False
    right, left = np.zeros((64, 64), dtype=bool), np.zeros((64, 64), dtype=bool)
    right[:, 63] = True
    left[:, 0] = True
    pts = scenes.jittered_lattice(400, 0.8, (8.0, 8.0), 0.1, 2)  # (across both cuts of the 2 x 2 mesh, at 16 m)
    planner = FieldPlanner((0.0, 0.0), 0.5, np.zeros((64, 64, 2), dtype=np.float32))
    mesh, single = NativeTileMesh(LocationHash2D(**GRID), (2, 2), 1), Simulation(LocationHash2D(**GRID))
    try:
        for t in (mesh, single):
            t.add_agents(pts, planner, LP, 1.0)
        planner.solve(right, 0.1, blocked=blocked, density_weight=0.25, vectors=False)  # (the engine and every tile)
        _same(mesh, single, "before the first step")
        for step in range(6):
            if step == 3:
                vec, _, stats = planner.solve(left, 0.1, blocked=blocked, density_weight=0.25)
                counts = single.agent_field((0.0, 0.0), 0.5, (64, 64))
                assert vec.tobytes() == ref.solve(blocked, left, (0.5, 0.5), 0.1, counts=counts, density_weight=0.25)[0].tobytes()
                assert stats["reached"] == int((~blocked).sum())
            for t in (mesh, single):
                t.step(0.05, report=step % 2 == 0)
            now = _same(mesh, single, step)
            if step == 2:
                third = now
        assert third["vx"].mean() > 0.0 and now["vx"].mean() < third["vx"].mean()
    finally:
        single.close()
        mesh.__del__()
