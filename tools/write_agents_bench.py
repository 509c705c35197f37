"""Time Simulation.write_agents on bench.py's 1,000,000-agent walk scene (the write row).

For k = 1, 10^3, 10^5 and 10^6 records (position + velocity, every agent moved by 1 cm): the host clock around calls
that end synchronised (cs_write_agents reads its match count back), split into
    prep    the Python side: the records and their AGENT_DTYPE array
    call    cs_write_agents itself: validation, placement and sort on the host, the one upload, both kernels, the read back
and the first step after a write (it sorts every agent: the written cells void the kept histogram) against an
ordinary step.  Kernel times come from a separate run under the profiler:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/write_agents_bench.py
(k_write_match / k_write_apply in its kernel statistics).  One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import bench
    from rmf_crowdsim_amd import Simulation, _abi, scenes
    from rmf_crowdsim_amd.simulation import write_records
    sim, _ = bench.build_crowd(Simulation, args.agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[:2]
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    base = sim.read_agents()
    n = len(base)
    rng = np.random.default_rng(1)
    out = {"agents": n, "write": {}}

    def timed_step():
        sim.synchronize()
        t0 = time.perf_counter()
        sim.step(0.05, report=False)
        sim.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for k in (1, 1000, 100_000, 1_000_000):
        k = min(k, n)
        prep, call, first, plain = [], [], [], []
        for rep in range(args.reps + 1):  # (the first repetition warms up)
            cur = sim.read_agents()
            t0 = time.perf_counter()
            pick = np.sort(rng.choice(n, size=k, replace=False)) if k < n else np.arange(n)
            rec = cur[pick].copy()
            rec["x"] += 0.01
            arr = write_records(rec)
            t1 = time.perf_counter()
            rc = sim._lib.cs_write_agents(sim._engine, arr.ctypes.data_as(C.POINTER(_abi.AgentView)), len(arr),
                                          _abi.CS_WRITE_POSITION | _abi.CS_WRITE_VELOCITY)
            t2 = time.perf_counter()
            assert rc == 0, sim._lib.cs_last_error(sim._engine).decode()
            f = timed_step()
            p = timed_step()
            if rep:
                prep.append((t1 - t0) * 1e6)
                call.append((t2 - t1) * 1e6)
                first.append(f)
                plain.append(p)
        out["write"][str(k)] = {"prep_us": float(np.median(prep)), "call_us": float(np.median(call)),
                                "call_us_min": float(np.min(call)), "first_step_us": float(np.median(first)),
                                "plain_step_us": float(np.median(plain))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
