"""Steps per second of bench.py's walking workload under four high-level planners ("Flow-field
planner"): the same crowd, the same preferred velocities, so the same trajectories; only where they come from differs:
    constant       StubHighLevelPlan, the CONSTANT planner of bench.py's own run (the step kernel holds the velocity)
    nearest        a FieldPlanner with "nearest" sampling: k_hlp_field fills pref on the device, one launch a step
    bilinear       the same with "bilinear" sampling
    callback       the same field through as_host_planner(): download, host call, upload, wait, every step.  Its host
                   call is numpy over all agents at once (the per-agent Python of the default thunk would measure the
                   interpreter); it runs --callback-steps steps, because it is slow by design.
Each crowd has two uniform fields of --bins x --bins bins over the whole grid (walkers drifting +y and -y), stepped
fire-and-forget and synchronised once: the host clock over --steps steps after --warmup, best and median of --reps.  The
field kernel's own time comes from events either side of its launches (CS_HLP_FIELD_TIME=1, cs_kernel_stat
CS_STAT_HLP_FIELD_NS); its traffic is counted as 16 B read and 8 B written per agent.  One JSON line on stdout; --text
PATH also writes the table."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES_PER_AGENT = 24  # cell 4, meta 4, offset 8 read; pref 8 written (the group and the samples come from the caches)


class BatchedHostField:
    """FieldPlanner.as_host_planner() with the host call vectorised: NEAREST of a field without NaN, in numpy f64"""

    def __new__(cls, field):
        import ctypes as C
        from rmf_crowdsim_amd import HighLevelPlanner, _abi

        class Planner(HighLevelPlanner):
            def _desc(self):
                (x0, y0), (cw, ch), v = field.origin, field.cell, field.vectors
                ny, nx = v.shape[:2]

                def velocity(_user, n, ids, pos, vel, time_s, out, some):
                    p = np.ctypeslib.as_array(pos, shape=(2 * n,)).reshape(n, 2)
                    fx, fy = (p[:, 0] - x0) / cw, (p[:, 1] - y0) / ch
                    inside = (0.0 <= fx) & (fx < nx) & (0.0 <= fy) & (fy < ny)
                    ix, iy = np.where(inside, fx, 0.0).astype(np.int64), np.where(inside, fy, 0.0).astype(np.int64)
                    np.ctypeslib.as_array(out, shape=(2 * n,)).reshape(n, 2)[:] = v[iy, ix]
                    np.ctypeslib.as_array(some, shape=(n,))[:] = inside

                fv = _abi.HlpVelocityFn(velocity)
                return _abi.HlpDesc(_abi.CS_HLP_CALLBACK, 0.0, 0.0, fv, _abi.HlpSetTargetFn(), _abi.HlpRemoveFn(), None,
                                    _abi.RoutePlanFn(), 0.0, 0.0, 0.0), [fv]
        return Planner()


def crowd(agents, planner, steps, bins):
    """bench.py's walking crowd with its two preferred velocities from `planner` kind"""
    import bench
    from rmf_crowdsim_amd import FieldPlanner, LocationHash2D, Simulation, StubHighLevelPlan, Zanlungo, scenes
    pts, grid, extent, group = scenes.uniform_crowd(agents, seed=7, cell_size=2.0, room=bench.walk_room(steps))
    sim = Simulation(LocationHash2D(**grid), capacity_hint=agents + 4096)
    lp = Zanlungo(*scenes.METRIC_ZANLUNGO)
    for g, creep in ((0, scenes.CREEP_SPEED), (1, -scenes.CREEP_SPEED)):
        vel = (scenes.WALK_SPEED, creep)
        if planner == "constant":
            hlp = StubHighLevelPlan(vel)
        else:
            v = np.zeros((bins, bins, 2), dtype=np.float32)
            v[...] = vel
            cell = (grid["height"] / bins * (1.0 + 1e-9), grid["width"] / bins * (1.0 + 1e-9))  # (x runs over the height)
            hlp = FieldPlanner(grid["offset"], cell, v, "bilinear" if planner == "bilinear" else "nearest")
            if planner == "callback":
                hlp = BatchedHostField(hlp)
        sim.add_agents(pts[group == g], hlp, lp, 2.0)
    return sim


def measure(agents, planner, args):
    from rmf_crowdsim_amd import _abi
    steps = args.callback_steps if planner == "callback" else args.steps
    on_device = planner in ("nearest", "bilinear")
    os.environ.pop("CS_HLP_FIELD_TIME", None)  # (read when an engine is created: the rates are taken without the events)
    sim = crowd(agents, planner, (steps + args.warmup) * args.reps + 8, args.bins)
    rates = []
    for _ in range(args.reps):
        for _ in range(args.warmup):
            sim.step(0.05, report=False)
        sim.synchronize()
        n0 = sim.kernel_stat(_abi.CS_STAT_HLP_FIELD_LAUNCHES)
        t0 = time.perf_counter()
        for _ in range(steps):
            sim.step(0.05, report=False)
        sim.synchronize()
        rates.append(steps / (time.perf_counter() - t0))
        launches = sim.kernel_stat(_abi.CS_STAT_HLP_FIELD_LAUNCHES) - n0
    speed = float(np.median(sim.read_agents()["vx"]))
    sim.close()
    row = {"planner": planner, "agents": agents, "steps": steps, "steps_per_s_best": max(rates),
           "steps_per_s_median": float(np.median(rates)), "us_per_step_best": 1e6 / max(rates),
           "median_vx": speed, "field_launches_per_step": launches / steps}
    if on_device:  # the kernel's own time, in an engine of its own: an event either side of every launch
        os.environ["CS_HLP_FIELD_TIME"] = "1"
        sim = crowd(agents, planner, args.steps + args.warmup + 8, args.bins)
        for _ in range(args.warmup):
            sim.step(0.05, report=False)
        ns0 = sim.kernel_stat(_abi.CS_STAT_HLP_FIELD_NS)
        for _ in range(args.steps):
            sim.step(0.05, report=False)
        k = (sim.kernel_stat(_abi.CS_STAT_HLP_FIELD_NS) - ns0) / 1e3 / args.steps
        sim.close()
        os.environ.pop("CS_HLP_FIELD_TIME", None)
        row.update(field_kernel_us=k, field_kernel_gb_per_s=agents * BYTES_PER_AGENT / (k * 1e-6) / 1e9)
    print(f"{agents} agents, {planner}: done", file=sys.stderr, flush=True)
    return row


def text(result):
    lines = [f"walking workload of bench.py, two uniform fields of {result['bins']} x {result['bins']} bins; best (median) of "
             f"{result['reps']} runs of {result['steps']} steps ({result['callback_steps']} for the callback planner) after "
             f"{result['warmup']}; the kernel's bytes: {BYTES_PER_AGENT} per agent"]
    for n in sorted(set(r["agents"] for r in result["rows"])):
        rows = {r["planner"]: r for r in result["rows"] if r["agents"] == n}
        base = rows["constant"]["us_per_step_best"]
        lines.append("")
        lines.append(f"{n} agents")
        for name in ("constant", "nearest", "bilinear", "callback"):
            r = rows[name]
            line = (f"  {name:<10}{r['steps_per_s_best']:>10.1f} steps/s ({r['steps_per_s_median']:.1f}){r['us_per_step_best']:>12.1f} us/step"
                    f"{r['us_per_step_best'] - base:>+10.1f} us against constant")
            if "field_kernel_us" in r:
                line += f"   k_hlp_field {r['field_kernel_us']:.1f} us, {r['field_kernel_gb_per_s']:.0f} GB/s"
            lines.append(line)
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[1_000_000, 20_000])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--callback-steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--text", default=None, help="also write the table to this file")
    args = ap.parse_args()
    rows = [measure(n, p, args) for n in args.agents for p in ("constant", "nearest", "bilinear", "callback")]
    result = {"steps": args.steps, "callback_steps": args.callback_steps, "warmup": args.warmup, "reps": args.reps,
              "bins": args.bins, "rows": rows}
    if args.text:
        with open(args.text, "w") as f:
            f.write(text(result))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
