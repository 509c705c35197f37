"""Time cs_close_pairs on bench.py's walk scene at 1,000,000 and at 125,000 agents ("Pairs of
agents between steps"), against what a host had before it: reading the whole crowd back and asking a radius query at
every agent's position.

After 20 steps, the host clock around calls that end synchronised, the median of --reps repetitions after --warmup
unrecorded ones, with the smallest and the largest beside it, for distance = 0.4 m (overlap: 2 * agent_radius) and 1.5 m:
    count        cs_close_pairs, the count-only form
    list         cs_close_pairs listing every pair with its d2 (one counting call sizes the arrays and is timed with it)
    robots       the same two forms with 8 robots (agents of a NoLocalPlan planner added into the crowd) against everyone
    parent_path  cs_read_agents of the whole crowd, cs_query_radius_batch at every agent's position (room for --cap ids per
                 query), and the numpy pass that keeps each pair once (a < b): the only way on the parent commit.  Its
                 pairs are judged in f32 and are not compared bit for bit; the two counts are printed side by side.
Kernel times come from a separate run under the profiler:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/close_pairs_bench.py --reps 3 --warmup 1
One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(us):
    return {"median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us))}


def _timed(fn, warmup, reps):
    us = []
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if rep >= warmup:
            us.append((t1 - t0) * 1e6)
    return _stats(us)


def run(agents, args):
    import bench
    from rmf_crowdsim_amd import NoLocalPlan, Simulation, StubHighLevelPlan, _abi, scenes
    sim = bench.build_crowd(Simulation, agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[0]
    lib, eng = sim._lib, sim._engine
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    rec = sim.read_agents()
    # 8 robots standing in the crowd, a third of a metre from an agent each
    nolp = NoLocalPlan()
    picks = rec[np.linspace(0, len(rec) - 1, 8).astype(np.int64)]
    sim.add_agents(np.stack([picks["x"] + 0.3, picks["y"] + 0.1], axis=1), StubHighLevelPlan((0.0, 0.0)), nolp, 2.0)
    robots = _abi.Selection()
    robots.terms = _abi.CS_SEL_LP
    robots.lp = sim._planner_handles[id(nolp)]
    n = len(sim)
    out = {"agents": n}
    pairp, dblp, u64p, viewp = C.POINTER(_abi.IdPair), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(_abi.AgentView)
    size_max = C.c_size_t(-1).value

    def count(distance, sel):
        got = lib.cs_close_pairs(eng, distance, C.byref(sel) if sel is not None else None, None, None, None, 0)
        assert got != size_max, lib.cs_last_error(eng).decode()
        return got

    def listing(distance, sel):
        m = count(distance, sel)
        pairs = np.empty((max(m, 1), 2), dtype=np.uint64)
        d2 = np.empty(max(m, 1))
        got = lib.cs_close_pairs(eng, distance, C.byref(sel) if sel is not None else None, None,
                                 pairs.ctypes.data_as(pairp), d2.ctypes.data_as(dblp), m)
        assert got == m, lib.cs_last_error(eng).decode()
        return pairs[:m]

    buf = np.zeros(n, dtype=np.dtype(_abi.AgentView))
    overfull = [0]

    def parent_path(distance):
        got = lib.cs_read_agents(eng, buf.ctypes.data_as(viewp), lib.cs_agent_count(eng))
        assert got == n
        xy = np.ascontiguousarray(np.stack([buf["x"], buf["y"]], axis=1))
        radius = np.full(n, distance)
        ids = np.zeros((n, args.cap), dtype=np.uint64)
        counts = np.zeros(n, dtype=np.uint64)
        rc = lib.cs_query_radius_batch(eng, n, xy.ctypes.data_as(dblp), radius.ctypes.data_as(dblp), args.cap,
                                       ids.ctypes.data_as(u64p), counts.ctypes.data_as(u64p), None, None)
        assert rc == 0, lib.cs_last_error(eng).decode()
        overfull[0] = max(overfull[0], int(counts.max()))  # (above --cap: the list is short and the time flatters this path)
        mine = np.repeat(buf["id"].astype(np.uint64), args.cap).reshape(n, args.cap)
        keep = (np.arange(args.cap)[None, :] < counts[:, None]) & (ids > mine)  # each pair once; the agent itself dropped
        pairs = np.stack([mine[keep], ids[keep]], axis=1)
        return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]

    for distance in args.distances:
        row = {"pairs": int(count(distance, None)), "pairs_with_a_robot": int(count(distance, robots))}
        row["count"] = _timed(lambda: count(distance, None), args.warmup, args.reps)
        row["list"] = _timed(lambda: listing(distance, None), args.warmup, args.reps)
        row["robots_count"] = _timed(lambda: count(distance, robots), args.warmup, args.reps)
        row["robots_list"] = _timed(lambda: listing(distance, robots), args.warmup, args.reps)
        row["parent_path"] = _timed(lambda: parent_path(distance), 1, args.parent_reps)
        row["parent_path_pairs"] = int(len(parent_path(distance)))
        row["parent_path_most_per_query"], row["parent_path_cap"] = overfull[0], args.cap
        overfull[0] = 0
        row["parent_over_list"] = row["parent_path"]["median_us"] / row["list"]["median_us"]
        row["parent_over_count"] = row["parent_path"]["median_us"] / row["count"]["median_us"]
        out[f"{distance} m"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[1_000_000, 125_000])
    ap.add_argument("--distances", type=float, nargs="*", default=[0.4, 1.5])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-reps", type=int, default=3)
    ap.add_argument("--cap", type=int, default=24)
    args = ap.parse_args()
    print(json.dumps({"reps": args.reps, "warmup": args.warmup, "parent_reps": args.parent_reps,
                      "runs": [run(n, args) for n in args.agents]}))


if __name__ == "__main__":
    main()
