"""Wall time of solving a flow field ("Solving a flow field"): the same raster, the same goals, by
    device          Simulation.solve_flow_field with the distances and the vectors downloaded (host clock; the call waits)
    into planner    FieldPlanner.solve(vectors=False): the vectors go straight into the planner's device samples and
                    nothing is downloaded; timed to the synchronise behind it
    host c++        tools/flow_dijkstra_host.cpp, a std::priority_queue Dijkstra of the same rule, compiled -O2, one
                    thread: the fair baseline.  Its distances are checked against the device's, byte for byte.
    python          flow_field_to_goals, the package's pure-Python producer (rasters of at most --python-bins bins)
for rasters of --sizes bins a side: open (goals on the right edge), 30 % random walls, and a serpentine maze (walls every
4 columns, one-bin gaps), without density and with the density of --agents agents at weight 0.25 (the crowd of bench.py,
the raster over its whole grid; the time then includes the raster of the crowd, and the host baselines are handed the
counts for nothing).  Best and median of --reps after one warm-up solve.  One JSON line on stdout; --text PATH also writes
the table."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_baseline():
    """tools/flow_dijkstra_host.cpp as a shared library in a temporary directory"""
    out = os.path.join(tempfile.mkdtemp(prefix="flow_dijkstra_"), "libflow_dijkstra_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tools", "flow_dijkstra_host.cpp")], check=True)
    lib = C.CDLL(out)
    lib.flow_dijkstra_host.restype = C.c_double
    lib.flow_dijkstra_host.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.POINTER(C.c_uint8),
                                       C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return lib


def scene(kind, n):
    blocked = np.zeros((n, n), dtype=bool)
    goals = np.zeros((n, n), dtype=bool)
    if kind == "open":
        goals[:, n - 1] = True
    elif kind == "walls":
        blocked = np.random.default_rng(1).random((n, n)) < 0.3
        goals[:, n - 1] = True
        blocked[:, n - 1] = False
    else:  # the serpentine maze
        for k, ix in enumerate(range(3, n - 1, 4)):
            blocked[:, ix] = True
            blocked[0 if k % 2 else n - 1, ix] = False
        goals[0, 0] = True
    return blocked, goals


def best_median(fn, reps):
    fn()  # (warm-up: scratch grown, code objects loaded)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t), float(np.median(t))


def measure(sim, planner_of, lib, kind, n, weight, args):
    from rmf_crowdsim_amd import flow_field_to_goals
    origin, cell = sim_origin(sim), (sim_extent(sim)[0] / n * (1.0 + 1e-9), sim_extent(sim)[1] / n * (1.0 + 1e-9))
    blocked, goals = scene(kind, n)
    how = dict(blocked=blocked, density_weight=weight)
    out = {}

    def device():
        out["vec"], out["dist"], out["stats"] = sim.solve_flow_field(origin, cell, goals, 1.0, distance=True, **how)

    planner = planner_of(n, origin, cell)  # (its handful of agents stand before the first solve: every solver sees them)
    row = {"scene": kind, "bins": n, "density_weight": weight}
    row["device_s_best"], row["device_s_median"] = best_median(device, args.reps)
    row["rounds"], row["reached"] = out["stats"]["rounds"], out["stats"]["reached"]

    def into_planner():
        planner.solve(goals, 1.0, vectors=False, **how)
        sim.synchronize()

    row["planner_s_best"], row["planner_s_median"] = best_median(into_planner, args.reps)
    # the host baselines get the counts for nothing
    s = None
    if weight:
        counts = sim.agent_field(origin, cell, (n, n))
        s = np.ascontiguousarray(1.0 * (1.0 + weight * counts.astype(np.float64)))
    g8, b8 = np.ascontiguousarray(goals, dtype=np.uint8), np.ascontiguousarray(blocked, dtype=np.uint8)
    dist = np.zeros((n, n), dtype=np.float64)
    u8, f64 = C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    t = [lib.flow_dijkstra_host(n, n, cell[0], cell[1], g8.ctypes.data_as(u8), b8.ctypes.data_as(u8),
                                s.ctypes.data_as(f64) if s is not None else None, dist.ctypes.data_as(f64))
         for _ in range(max(2, args.reps))]
    row["host_cpp_s_best"], row["host_cpp_s_median"] = min(t), float(np.median(t))
    row["host_cpp_equals_device"] = dist.tobytes() == out["dist"].tobytes()
    if not weight and n * n <= args.python_bins:
        t0 = time.perf_counter()
        flow_field_to_goals(blocked, goals, origin, cell, 1.0)
        row["python_s"] = time.perf_counter() - t0
    print(f"{kind} {n} x {n}, weight {weight}: done", file=sys.stderr, flush=True)
    return row


def sim_origin(sim):
    return sim.bench_grid["offset"]


def sim_extent(sim):
    return sim.bench_grid["height"], sim.bench_grid["width"]  # (x runs over the height)


def text(result):
    lines = [f"flow-field solve, seconds, best (median) of {result['reps']} after a warm-up; density: {result['agents']} "
             "agents at weight 0.25; host c++: std::priority_queue Dijkstra, -O2, one thread; python: flow_field_to_goals", ""]
    lines.append(f"{'scene':<8}{'bins':>12}{'density':>9}{'rounds':>8}{'device':>20}{'into planner':>20}{'host c++':>20}"
                 f"{'python':>10}  c++ == device")
    for r in result["rows"]:
        py = f"{r['python_s']:.3f}" if "python_s" in r else "-"
        lines.append(f"{r['scene']:<8}{r['bins']:>6} x {r['bins']:<4}{'yes' if r['density_weight'] else 'no':>8}{r['rounds']:>8}"
                     f"{r['device_s_best']:>11.5f} ({r['device_s_median']:.5f})"
                     f"{r['planner_s_best']:>11.5f} ({r['planner_s_median']:.5f})"
                     f"{r['host_cpp_s_best']:>11.5f} ({r['host_cpp_s_median']:.5f}){py:>10}  {r['host_cpp_equals_device']}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 2048])
    ap.add_argument("--scenes", nargs="*", default=["open", "walls", "maze"])
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--python-bins", type=int, default=256 * 256)
    ap.add_argument("--text", default=None, help="also write the table to this file")
    args = ap.parse_args()
    from rmf_crowdsim_amd import FieldPlanner, LocationHash2D, Simulation, StubHighLevelPlan, Zanlungo, scenes
    lib = host_baseline()
    pts, grid, extent, group = scenes.uniform_crowd(args.agents, seed=7, cell_size=2.0)
    rows = []
    for weight in (0.0, 0.25):
        sim = Simulation(LocationHash2D(**grid), capacity_hint=args.agents + 4096)
        sim.bench_grid = grid
        planners = {}

        def planner_of(n, origin, cell, sim=sim, planners=planners):
            if n not in planners:  # one planner per raster, registered with a handful of agents of its own
                planners[n] = FieldPlanner(origin, cell, np.zeros((n, n, 2), dtype=np.float32))
                sim.add_agents(pts[:4] + 0.01 * len(planners), planners[n], Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
            return planners[n]

        if weight:
            sim.add_agents(pts, StubHighLevelPlan((0.0, 0.0)), Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
            sim.step(0.05)  # (the agents in cell order, as between the steps of a running crowd)
        for n in args.sizes:
            for kind in args.scenes:
                rows.append(measure(sim, planner_of, lib, kind, n, weight, args))
        sim.close()
    result = {"reps": args.reps, "agents": args.agents, "rows": rows}
    if args.text:
        with open(args.text, "w") as f:
            f.write(text(result))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
