"""Time Simulation.set_targets (cs_set_targets, include/crowdstep_state.h) on a 1,000,000-agent engine of route followers
("Sending agents to goals in batches").

A uniform crowd at 2.5 agents/m^2 under one RouteFollower whose plan_route is a three-point dogleg.  The host clock
around calls that end synchronised, the median of --reps repetitions with the smallest and the largest beside it, for
batches of k seeded random ids (k from --k):
    booked     every (start, goal) hash pair is in the route book (scale 50 m: a few hundred pairs, planned by one
               untimed dispatch of the whole crowd): the device answers every entry, the host plans nothing
    new        every entry is a pair of its own (scale 0.25 m, a fresh goal every repetition): one route_plan call per
               entry.  The planner here is Python behind ctypes, so this row is mostly the host's callback; `plan_us`
               is the time spent inside it, `call_minus_plan_us` the rest
    write      cs_write_agents, position only, of the same k agents to where they stand: the yardstick of the same shape
               (ids mapped and sorted on the host, one match over the slots, one kernel per record, one read back)
How a call splits into host preparation, kernels and read back comes from a run under the profiler:
    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d <dir> -- python tools/set_targets_bench.py --reps 1
(k_write_match / k_target_probe / k_route_assign and the copies, in its statistics; the host's share is the rest).
One JSON line on stdout."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(us):
    return {"median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us))}


class Doglegs:
    def __init__(self):
        self.calls, self.seconds = 0, 0.0

    def __call__(self, s, g):
        t0 = time.perf_counter()
        self.calls += 1
        dx, dy = g[0] - s[0], g[1] - s[1]
        n = math.hypot(dx, dy) or 1.0
        out = [s, (0.5 * (s[0] + g[0]) - 2.0 * dy / n, 0.5 * (s[1] + g[1]) + 2.0 * dx / n), g]
        self.seconds += time.perf_counter() - t0
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, nargs="*", default=[1000, 100_000, 1_000_000])
    args = ap.parse_args()
    from rmf_crowdsim_amd import LocationHash2D, NoLocalPlan, RouteFollower, Simulation, _abi
    side = math.sqrt(args.agents / 2.5)
    extent = side + 20.0
    rng = np.random.default_rng(1)
    pts = rng.uniform(10.0, 10.0 + side, (args.agents, 2))
    exits = np.array([(5.0, 5.0), (extent - 5.0, 5.0), (extent - 5.0, extent - 5.0), (5.0, extent - 5.0),
                      (0.5 * extent, 5.0)])
    u64p, f64p, u8p, viewp = C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(_abi.AgentView)
    out = {"agents": args.agents, "booked": {}, "new": {}, "write": {}}

    def engine(scale):
        routes = Doglegs()
        sim = Simulation(LocationHash2D(extent, extent, 2.0, (0.0, 0.0)))
        ids = np.asarray(sim.add_agents(pts, RouteFollower(routes, scale=scale, speed=1.2), NoLocalPlan(), 1.0),
                         dtype=np.uint64)
        sim.step(0.05)
        return sim, routes, ids

    def send(sim, ids, goals, status):
        t0 = time.perf_counter()
        rc = sim._lib.cs_set_targets(sim._engine, ids.ctypes.data_as(u64p), goals.ctypes.data_as(f64p), len(ids), 0.0, 0.0,
                                     status.ctypes.data_as(u8p))
        t1 = time.perf_counter()
        assert rc == 0, sim._lib.cs_last_error(sim._engine).decode()
        return (t1 - t0) * 1e6

    # ---- booked, and the write beside it, on one engine ----
    sim, routes, ids_all = engine(50.0)
    goal_of = exits[(ids_all % 5).astype(np.int64)]
    status = np.zeros(len(ids_all), dtype=np.uint8)
    out["first_dispatch_us"] = send(sim, ids_all, np.ascontiguousarray(goal_of), status)
    out["routes_planned"] = routes.calls
    rows_all = sim.read_agents()
    for k in args.k:
        k = min(k, len(ids_all))
        us_b, us_w = [], []
        for rep in range(args.reps + 1):  # (the first repetition warms up)
            pick = rng.choice(len(ids_all), size=k, replace=False)
            ids, goals = np.ascontiguousarray(ids_all[pick]), np.ascontiguousarray(goal_of[pick])
            st = np.zeros(k, dtype=np.uint8)
            planned = routes.calls
            t = send(sim, ids, goals, st)
            assert (st == _abi.CS_TARGET_BOOKED).all() and routes.calls == planned
            rows = np.ascontiguousarray(rows_all[pick])
            sim.synchronize()
            t0 = time.perf_counter()
            rc = sim._lib.cs_write_agents(sim._engine, rows.ctypes.data_as(viewp), k, _abi.CS_WRITE_POSITION)
            t1 = time.perf_counter()
            assert rc == 0, sim._lib.cs_last_error(sim._engine).decode()
            if rep:
                us_b.append(t)
                us_w.append((t1 - t0) * 1e6)
        out["booked"][str(k)] = _stats(us_b)
        out["write"][str(k)] = _stats(us_w)
    del sim

    # ---- all new ----
    sim, routes, ids_all = engine(0.25)
    for k in args.k:
        k = min(k, len(ids_all))
        us, plan = [], []
        # (a route index has 22 bits: the million-entry batch is timed once, cold)
        warm, reps = (0, 1) if k >= 500_000 else (1, min(args.reps, 3))
        for rep in range(warm + reps):
            pick = rng.choice(len(ids_all), size=k, replace=False)
            ids = np.ascontiguousarray(ids_all[pick])
            goals = np.ascontiguousarray(exits[(ids % 5).astype(np.int64)] + rng.uniform(-4.0, 4.0, (k, 2)))
            st = np.zeros(k, dtype=np.uint8)
            routes.seconds = 0.0
            t = send(sim, ids, goals, st)
            if rep >= warm:
                assert (st == _abi.CS_TARGET_PLANNED).mean() > 0.99
                us.append(t)
                plan.append(routes.seconds * 1e6)
        out["new"][str(k)] = dict(_stats(us), plan_us=float(np.median(plan)),
                                  call_minus_plan_us=float(np.median(np.array(us) - np.array(plan))))
    out["routes_in_book"] = routes.calls
    print(json.dumps(out))


if __name__ == "__main__":
    main()
