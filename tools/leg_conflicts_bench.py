"""Time cs_leg_conflicts on bench.py's walk scene at 1,000,000 agents ("Paths against the moving
crowd"): --paths robot paths of --legs legs of --leg-seconds each at 1 m/s, every path starting on an agent of the crowd
that its legs ignore, every fourth leg a wait; distance --distance, speed_max --speed-max.  Two sets of the same legs:
    short          t1 as the path gives it: a reach of distance + speed_max * t1, a few cells
    stretched      every t1 raised so that the walk's reach distance + speed_max * t1 + cell is --grow metres (15)

After 20 steps, the host clock around calls that end synchronised, the median of --reps repetitions after --warmup
unrecorded ones, with the smallest and the largest beside it:
    conflicts      cs_leg_conflicts with the rows (one upload, one kernel, one download)
    count          the same with a null `out`
    read_agents    cs_read_agents alone: what any host-side answer has to do first
    host_path      cs_read_agents and, per path, the rule of the header in numpy over the agents within the reach of the
                   path's bounding box (the restriction that makes the comparison fair)
    cast_rays      cs_cast_rays for as many rays from the same starts along the same headings, for orientation
The rows of both ways are compared (the same ids and the same bits of s).
One JSON line on stdout; --text PATH also writes the table."""
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


def host_rule(x, y, vx, vy, ids, legs, distance, speed_max):
    """The rule of include/crowdstep_state.h for `legs` against the agents (x, y, vx, vy, ids), one numpy operation each
    -> the rows (id, s)"""
    from rmf_crowdsim_amd import _abi
    from rmf_crowdsim_amd.simulation import LEG_HIT_DTYPE
    D2 = np.float64(distance) * np.float64(distance)
    S2 = np.float64(speed_max) * np.float64(speed_max)
    x0, y0, lvx, lvy, t0 = (legs[f][:, None] for f in ("x0", "y0", "vx", "vy", "t0"))
    T = (legs["t1"] - legs["t0"])[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        slow = (vx * vx + vy * vy < S2)[None, :]
        px, py = x[None, :] + vx[None, :] * t0, y[None, :] + vy[None, :] * t0
        rx, ry = px - x0, py - y0
        wx, wy = vx[None, :] - lvx, vy[None, :] - lvy
        d2 = rx * rx + ry * ry
        inside = d2 < D2
        a = rx * wx + ry * wy
        ww = wx * wx + wy * wy
        cr = rx * wy - ry * wx
        h2 = D2 * ww - cr * cr
        s = (-a - np.sqrt(h2)) / ww
        s = np.where(s < 0, np.float64(0.0), s)
        s = np.where(inside, np.float64(0.0), s)
        hit = slow & (inside | ((a < 0) & (h2 > 0))) & (s < T) & (ids[None, :] != legs["ignore"][:, None])
    s = np.where(hit, s, np.inf)
    out = np.zeros(len(legs), dtype=LEG_HIT_DTYPE)
    out["s"] = s.min(axis=1) if len(ids) else np.inf
    first = hit & (s == out["s"][:, None])
    out["id"] = np.where(first, ids[None, :], np.uint64(_abi.CS_NO_HIT)).min(axis=1) if len(ids) else _abi.CS_NO_HIT
    return out


def run(agents, args):
    import bench
    from rmf_crowdsim_amd import Simulation, _abi, scenes
    from rmf_crowdsim_amd.simulation import LEG_HIT_DTYPE, RAY_HIT_DTYPE, legs_array, rays_array
    sim = bench.build_crowd(Simulation, agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[0]
    lib, eng = sim._lib, sim._engine
    cell = 2.0
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    rec = sim.read_agents()
    robots = rec[np.linspace(0, len(rec) - 1, args.paths + 2).astype(np.int64)[1:-1]]  # (none of them at an end of the crowd)
    rng = np.random.default_rng(17)
    phi = rng.uniform(0.0, 2.0 * np.pi, (len(robots), args.legs))
    v = np.stack([np.cos(phi), np.sin(phi)], axis=2)
    v[:, 3::4] = 0.0
    step = v * args.leg_seconds
    starts = np.stack([robots["x"], robots["y"]], axis=1)[:, None, :] + np.cumsum(step, axis=1) - step
    t0 = np.tile(np.arange(args.legs) * args.leg_seconds, len(robots))
    ignore = np.repeat(robots["id"].astype(np.uint64), args.legs)
    short = legs_array(starts.reshape(-1, 2), v.reshape(-1, 2), t0, t0 + args.leg_seconds, ignore)
    stretched = short.copy()
    stretched["t1"] = np.maximum(short["t1"], (args.grow - args.distance - cell) / args.speed_max)
    size_max = C.c_size_t(-1).value
    out = {"agents": len(sim), "paths": len(robots), "legs_per_path": args.legs, "distance": args.distance,
           "speed_max": args.speed_max, "faster_than_speed_max": int(sim.count_agents([dict(speed=(args.speed_max, np.inf))])[0])}

    def ask(legs, rows):
        got = lib.cs_leg_conflicts(eng, legs.ctypes.data_as(C.POINTER(_abi.Leg)), len(legs), args.distance, args.speed_max,
                                   None, rows.ctypes.data_as(C.POINTER(_abi.LegHit)) if rows is not None else None)
        assert got != size_max, lib.cs_last_error(eng).decode()
        return got

    def host_path(legs):
        now = sim.read_agents()
        x, y, ids = now["x"], now["y"], now["id"].astype(np.uint64)
        vx, vy = now["vx"].astype(np.float64), now["vy"].astype(np.float64)
        rows = np.zeros(len(legs), dtype=LEG_HIT_DTYPE)
        for k in range(len(robots)):
            mine = slice(k * args.legs, (k + 1) * args.legs)
            l = legs[mine]
            reach = np.float64(args.distance) + np.float64(args.speed_max) * l["t1"].max() + 1e-6
            ex, ey = l["x0"] + l["vx"] * (l["t1"] - l["t0"]), l["y0"] + l["vy"] * (l["t1"] - l["t0"])
            near = np.nonzero((x >= min(l["x0"].min(), ex.min()) - reach) & (x <= max(l["x0"].max(), ex.max()) + reach) &
                              (y >= min(l["y0"].min(), ey.min()) - reach) & (y <= max(l["y0"].max(), ey.max()) + reach))[0]
            rows[mine] = host_rule(x[near], y[near], vx[near], vy[near], ids[near], l, args.distance, args.speed_max)
        return rows

    out["read_agents"] = _timed(sim.read_agents, 1, args.host_reps + 1)
    for name, legs in (("short", short), ("stretched", stretched)):
        rows = np.zeros(len(legs), dtype=LEG_HIT_DTYPE)
        hits = int(ask(legs, rows))
        hit = rows["id"] != _abi.CS_NO_HIT
        grow = args.distance + args.speed_max * float(legs["t1"].max()) + cell
        row = {"legs": len(legs), "conflicts": hits, "at_s_0": int((hit & (rows["s"] == 0.0)).sum()), "largest_grow_m": grow,
               "conflicts_rows": _timed(lambda: ask(legs, rows), args.warmup, args.reps),
               "count": _timed(lambda: ask(legs, None), args.warmup, args.reps),
               "host_path": _timed(lambda: host_path(legs), 0, args.host_reps)}
        row["rows_equal"] = bool(host_path(legs).tobytes() == rows.tobytes())
        print(f"{agents} agents, {name}: done", file=sys.stderr, flush=True)
        out[name] = row
    moving = (short["vx"] != 0.0) | (short["vy"] != 0.0)
    rays = rays_array(np.column_stack([short["x0"], short["y0"]]), np.where(moving[:, None], np.column_stack([short["vx"], short["vy"]]), (1.0, 0.0)),
                      args.leg_seconds, short["ignore"])
    ray_rows = np.zeros(len(rays), dtype=RAY_HIT_DTYPE)

    def cast():
        got = lib.cs_cast_rays(eng, rays.ctypes.data_as(C.POINTER(_abi.Ray)), len(rays), args.distance, None,
                               ray_rows.ctypes.data_as(C.POINTER(_abi.RayHit)))
        assert got != size_max, lib.cs_last_error(eng).decode()

    out["cast_rays"] = dict(_timed(cast, args.warmup, args.reps), rays=len(rays))
    return out


def text(result):
    lines = []
    for r in result["runs"]:
        lines += ["", f"{r['agents']} agents, {r['paths']} paths x {r['legs_per_path']} legs, distance {r['distance']}, speed_max "
                      f"{r['speed_max']} ({r['faster_than_speed_max']} agents at or above it)"]
        ra = r["read_agents"]
        lines.append(f"  read_agents alone {ra['median_us']:>10.0f} us [{ra['min_us']:.0f}-{ra['max_us']:.0f}]")
        cr = r["cast_rays"]
        lines.append(f"  cast_rays, {cr['rays']} rays {cr['median_us']:>10.0f} us [{cr['min_us']:.0f}-{cr['max_us']:.0f}]")
        for name in ("short", "stretched"):
            row = r[name]
            lines.append(f"  {name}: {row['conflicts']} of {row['legs']} legs conflict, {row['at_s_0']} of them at s == 0, largest grow "
                         f"{row['largest_grow_m']:.2f} m; rows equal to the host path's: {row['rows_equal']}")
            for form in ("conflicts_rows", "count", "host_path"):
                v = row[form]
                lines.append(f"    {form:<15}{v['median_us']:>10.0f} us [{v['min_us']:.0f}-{v['max_us']:.0f}]")
            lines.append(f"    read_agents / conflicts_rows {ra['median_us'] / row['conflicts_rows']['median_us']:.1f}, "
                         f"host_path / conflicts_rows {row['host_path']['median_us'] / row['conflicts_rows']['median_us']:.1f}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[1_000_000])
    ap.add_argument("--paths", type=int, default=512)
    ap.add_argument("--legs", type=int, default=8)
    ap.add_argument("--leg-seconds", type=float, default=0.5)
    ap.add_argument("--distance", type=float, default=0.5)
    ap.add_argument("--speed-max", type=float, default=2.0)
    ap.add_argument("--grow", type=float, default=15.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--text", default=None, help="also write the table to this file")
    args = ap.parse_args()
    result = {"reps": args.reps, "warmup": args.warmup, "host_reps": args.host_reps, "runs": [run(n, args) for n in args.agents]}
    if args.text:
        with open(args.text, "w") as f:
            f.write(text(result))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
