"""tests/cpp/test_flow_solve.cpp on the GPU: Simulation::solve_flow_field, TiledSimulation::solve_flow_field and
FieldPlanner::solve through include/crowdsim.hpp, on a serpentine maze and on a raster weighted by the density of a crowd,
against the bytes the Python restatement of the rule (tests/flow_solve_reference.py) writes into the case file."""
import struct
import subprocess

import numpy as np
import pytest

import flow_solve_reference as ref
from rmf_crowdsim_amd import LocationHash2D, Simulation, StubHighLevelPlan, Zanlungo, scenes
from test_gpu_cpp_api import build_cpp_test

pytestmark = pytest.mark.gpu


def _case(blocked, goals, origin, cell, speed, weight, pts, counts):
    vec, dist, reached, _ = ref.solve(blocked, goals, cell, speed, counts=counts, density_weight=weight)
    ny, nx = goals.shape
    out = struct.pack("<4I6dQ", nx, ny, 1, len(pts), origin[0], origin[1], cell[0], cell[1], speed, weight, reached)
    out += np.ascontiguousarray(goals, dtype=np.uint8).tobytes() + np.ascontiguousarray(blocked, dtype=np.uint8).tobytes()
    return out + np.ascontiguousarray(pts, dtype=np.float64).tobytes() + vec.tobytes() + dist.tobytes()


def test_cpp_flow_solve_on_an_engine_and_a_mesh(tmp_path):
    blocked, goals = ref.serpentine(40, 96, 4)
    cases = [_case(blocked, goals, (3.0, -2.0), (0.5, 0.25), 1.3, 0.0, np.zeros((0, 2)), None)]
    # 300 agents on the grid of the C++ test (64 m x 64 m, cells of 2 m), counted by the engine
    pts = scenes.jittered_lattice(300, 1.1, (20.0, 20.0), 0.1, 3)
    origin, cell, shape = (14.3, 16.9), (0.55, 0.45), (70, 60)
    sim = Simulation(LocationHash2D(64.0, 64.0, 2.0, (0.0, 0.0)))
    try:
        sim.add_agents(pts, StubHighLevelPlan((0.0, 0.0)), Zanlungo(1.0, 1.0, 0.0, 0.4, 2.0, 0.2), 2.0)
        counts = sim.agent_field(origin, cell, shape)
    finally:
        sim.close()
    assert int(counts.sum()) == 300
    blocked, goals = ref.random_walls(shape[0], shape[1], 6, 0.1, [(0, 0), (59, 69)])
    cases.append(_case(blocked, goals, origin, cell, 0.1, 0.5, pts, counts))  # (a walk slow enough that nobody collides)
    path = tmp_path / "flow_cases.bin"
    path.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    out = subprocess.run([build_cpp_test("test_flow_solve"), str(path)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "flow solve: passed" in out.stdout
