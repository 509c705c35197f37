"""Time Simulation.read_agents_by_id and remove_agents_by_id on bench.py's 1,000,000-agent walk scene (DESIGN.md
section 4, the by-id row), against what they replace: read_agents() of the whole crowd and a loop of single removes.

After 20 warm-up steps, the host clock around calls that end synchronised, the median of --reps repetitions with the
smallest and the largest beside it:
    read_all      cs_agent_count + cs_read_agents of the whole crowd
    read_by_id    cs_read_agents_by_id for k seeded random ids (k from --read-k), fresh ids every repetition
    remove        k ids (k from --remove-k), a fresh disjoint batch every repetition (a removal is not repeatable):
                  "batched" = one cs_remove_agents, "loop" = k calls of cs_remove_agent; then the first step after it
                  (it sorts again, as after a single remove) and an ordinary step
A library without include/crowdstep_state.h's by-id entry points (an older build chosen with CS_LIB_PATH, the baseline
of a comparison) is timed on read_all and the loop only.  Kernel times and launch counts come from a separate run under
the profiler:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/agents_by_id_bench.py --reps 1
(k_write_match / k_agents_gather / k_agents_kill, against k_remove_by_id, in its kernel statistics).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--read-k", type=int, nargs="*", default=[1, 1000, 100_000])
    ap.add_argument("--remove-k", type=int, nargs="*", default=[1000, 10_000])
    ap.add_argument("--remove", choices=["auto", "batched", "loop"], default="auto",
                    help="auto: batched where the library has cs_remove_agents, else the loop of single removes")
    args = ap.parse_args()
    import bench
    from rmf_crowdsim_amd import Simulation, _abi, scenes
    sim, _ = bench.build_crowd(Simulation, args.agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[:2]
    lib, eng = sim._lib, sim._engine
    has_by_id = hasattr(lib, "cs_remove_agents")  # (dlsym: an older build does not export it)
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    ids_all = sim.read_agents()["id"].copy()
    n = len(ids_all)
    rng = np.random.default_rng(1)
    mode = args.remove if args.remove != "auto" else ("batched" if has_by_id else "loop")
    out = {"agents": n, "by_id": bool(has_by_id), "remove_mode": mode, "read_by_id": {}, "remove": {}}
    u64p, viewp = C.POINTER(C.c_uint64), C.POINTER(_abi.AgentView)

    def timed_step():
        sim.synchronize()
        t0 = time.perf_counter()
        sim.step(0.05, report=False)
        sim.synchronize()
        return (time.perf_counter() - t0) * 1e6

    us = []
    buf = np.zeros(n, dtype=np.dtype(_abi.AgentView))
    for rep in range(args.reps + 1):  # (the first repetition warms up)
        t0 = time.perf_counter()
        count = lib.cs_agent_count(eng)
        got = lib.cs_read_agents(eng, buf.ctypes.data_as(viewp), count)
        t1 = time.perf_counter()
        assert got == n
        if rep:
            us.append((t1 - t0) * 1e6)
    out["read_all"] = _stats(us)

    if has_by_id:
        for k in args.read_k:
            k, us = min(k, n), []
            rec = np.zeros(k, dtype=np.dtype(_abi.AgentView))
            for rep in range(args.reps + 1):
                ids = np.ascontiguousarray(rng.choice(ids_all, size=k, replace=False))
                t0 = time.perf_counter()
                rc = lib.cs_read_agents_by_id(eng, ids.ctypes.data_as(u64p), k, rec.ctypes.data_as(viewp), None)
                t1 = time.perf_counter()
                assert rc == 0, lib.cs_last_error(eng).decode()
                if rep:
                    us.append((t1 - t0) * 1e6)
            out["read_by_id"][str(k)] = _stats(us)

    left = rng.permutation(ids_all)
    for k in args.remove_k:
        call, first, plain = [], [], []
        for rep in range(args.reps + 1):
            batch, left = np.ascontiguousarray(left[:k]), left[k:]
            assert len(batch) == k
            sim.synchronize()
            if mode == "batched":
                t0 = time.perf_counter()
                rc = lib.cs_remove_agents(eng, batch.ctypes.data_as(u64p), k)
                t1 = time.perf_counter()
                assert rc == 0, lib.cs_last_error(eng).decode()
            else:
                one = [int(i) for i in batch]
                t0 = time.perf_counter()
                for i in one:
                    lib.cs_remove_agent(eng, i)
                t1 = time.perf_counter()
            f = timed_step()
            p = timed_step()
            if rep:
                call.append((t1 - t0) * 1e6)
                first.append(f)
                plain.append(p)
        out["remove"][str(k)] = dict(_stats(call), first_step_us=float(np.median(first)),
                                     plain_step_us=float(np.median(plain)))
    out["agents_left"] = int(lib.cs_agent_count(eng))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
