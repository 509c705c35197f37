#!/usr/bin/env python3
"""CS_CFG_WIDE_IDS on the device: what the flag costs per step, and what a renumbering costs.

  walk      the 1M-agent counterflow walk (bench.py's crowd), K steps without a report, flag off vs on: the per-step
            path is the same, so the two must agree within noise;
  single    ~1M live agents plus 25,000 source-sinks whose agents reach their sink in the step they spawn (25,000 ids
            per step, the live count stays put), CS_DEVICE_ID_LIMIT just above twice the live count: the renumberings
            timed by the engine itself (CS_STAT_RENUMBER_NS: gather, 31-bit radix sort, rewrite, new table and its copy
            to the host, host wall time);
  mesh      the same on an in-process 2 x 2 cs_mesh (per tile sort, gather, merge, binary-search mapping);
  limit     a configs[3]-shaped stream (100k agents, 25,000 source-sinks) whose DEVICE counter starts just below the
            real limit 2^31 - 1 (CS_FIRST_DEVICE_ID): every step must succeed; the steps before and after the one real
            renumbering are timed (all 8 radix passes over 31-bit ids run there).
Prints one JSON line.  Run: python tools/wide_ids_bench.py [--agents N] [--steps K]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def walk(n, steps, wide):
    from rmf_crowdsim_amd import CS_CFG_WIDE_IDS, LocationHash2D, Simulation, Zanlungo, scenes
    pts, grid, extent, group = scenes.uniform_crowd(n, seed=7, cell_size=2.0)
    sim = Simulation(LocationHash2D(**grid), flags=CS_CFG_WIDE_IDS if wide else 0)
    scenes.add_counterflow(sim, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sim.step(0.05, report=False)
    sim.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    sim.close()
    return ms


def stream(part, n, n_sinks):
    """Crowd + sinks whose agents die in the step they spawn; returns per-step times and the renumbering statistics."""
    import numpy as np
    from rmf_crowdsim_amd import (CS_CFG_WIDE_IDS, LocationHash2D, MonotonicCrowd, NoLocalPlan, Simulation, SourceSink,
                                  StubHighLevelPlan, Zanlungo, _abi, scenes)
    from rmf_crowdsim_amd.tiles import NativeTileMesh
    pts, grid, extent, group = scenes.uniform_crowd(n, seed=7, cell_size=2.0, room=60.0)
    if part == "mesh":
        sim = NativeTileMesh(LocationHash2D(**grid), (2, 2), 2, flags=CS_CFG_WIDE_IDS)
    else:
        sim = Simulation(LocationHash2D(**grid), flags=CS_CFG_WIDE_IDS)
    scenes.add_counterflow(sim, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    side = int(np.ceil(np.sqrt(n_sinks)))
    for k in range(n_sinks):  # sources 0.3 m apart in the free band; each agent is inside its sink at once
        x, y = extent + 15.0 + 0.3 * (k % side), 5.0 + 0.3 * (k // side)
        sim.add_source_sink(SourceSink((x, y), 1.0, MonotonicCrowd(100.0), StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(),
                                       [(x, y)], False, 1.0))
    eng = sim.tile(0) if part == "mesh" else sim
    times, renumbered_at = [], []
    for s in range(int(os.environ.get("WIDE_BENCH_STEPS", "72"))):
        before = eng.kernel_stat(_abi.CS_STAT_RENUMBERINGS)
        t0 = time.perf_counter()
        sim.step(0.05, report=False)
        sim.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
        if eng.kernel_stat(_abi.CS_STAT_RENUMBERINGS) != before:
            renumbered_at.append(s)
    n_ren = eng.kernel_stat(_abi.CS_STAT_RENUMBERINGS)
    ns = eng.kernel_stat(_abi.CS_STAT_RENUMBER_NS)
    tail = sim.add_agents([(extent + 10.0, 2.0)], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.0)[0]
    live = len(sim)
    out = dict(live=live, next_external_id=tail, renumberings=n_ren,
               renumber_ms_each=round(ns / 1e6 / max(n_ren, 1), 3), median_step_ms=round(float(np.median(times)), 3),
               renumbered_at_steps=renumbered_at)
    if renumbered_at:
        k = renumbered_at[0]
        out["steps_around_first_ms"] = [round(t, 3) for t in times[max(k - 3, 0):k + 4]]
    return out


def sub(part, env_extra, args):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--agents", str(args.agents),
                        "--sinks", str(args.sinks)], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("%s run failed (%d): %s" % (part, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sinks", type=int, default=25_000)
    ap.add_argument("--part", default="")
    args = ap.parse_args()
    if args.part:
        print(json.dumps(stream(args.part, args.agents, args.sinks)))
        return
    out = {"agents": args.agents,
           "walk_step_ms_flag_off": round(walk(args.agents, args.steps, False), 4),
           "walk_step_ms_flag_on": round(walk(args.agents, args.steps, True), 4)}
    # each renumbering run in a process of its own: the knobs are read at cs_create
    limit = {"CS_DEVICE_ID_LIMIT": str(2 * (args.agents + args.sinks) + 200_000)}
    out["single"] = sub("single", limit, args)
    out["mesh_2x2"] = sub("mesh", limit, args)
    small = argparse.Namespace(agents=100_000, sinks=args.sinks)
    out["real_limit_100k"] = sub("limit", {"CS_FIRST_AGENT_ID": str(2 ** 31 - 2 - 100_000),
                                           "CS_FIRST_DEVICE_ID": str(2 ** 31 - 2 - 100_000 - 30 * args.sinks),
                                           "WIDE_BENCH_STEPS": "60"}, small)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
