"""Time cs_cast_rays on bench.py's walk scene at 1,000,000 agents ("Rays against the crowd between
steps"): range scans of --robots robots (agents of the crowd, each ignored by its own beams) with --beams beams each, discs
of --radius, at t_max of 5 m, 30 m and +inf (unit directions, so t is a distance).

After 20 steps, the host clock around calls that end synchronised, the median of --reps repetitions after --warmup
unrecorded ones, with the smallest and the largest beside it:
    cast           cs_cast_rays with the rows (one upload, one kernel, one download)
    count          the same with a null `out`
    host_path      what a host had before the call: cs_read_agents and, per robot, the rule of the header in numpy over the
                   agents within t_max + radius of the robot (the restriction that makes the comparison fair); at
                   t_max = +inf there is no such restriction and the path is not run
The three t_max side by side show what the early exit saves: at +inf a ray in a crowd ends at its first hit, not at the
edge of the grid.  The rows of both ways are compared (the same ids and the same bits of t).
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


def host_rule(x, y, ids, rays, radius):
    """The rule of include/crowdstep_state.h for `rays` against the agents (x, y, ids), one numpy operation each -> the
    rows (id, t)"""
    from rmf_crowdsim_amd import _abi
    from rmf_crowdsim_amd.simulation import RAY_HIT_DTYPE
    R2 = np.float64(radius) * np.float64(radius)
    ox, oy, ux, uy = (rays[f][:, None] for f in ("ox", "oy", "ux", "uy"))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        uu = ux * ux + uy * uy
        rx, ry = x[None, :] - ox, y[None, :] - oy
        d2 = rx * rx + ry * ry
        inside = d2 < R2
        b = rx * ux + ry * uy
        cr = rx * uy - ry * ux
        h2 = R2 * uu - cr * cr
        t = (b - np.sqrt(h2)) / uu
        t = np.where(t < 0, np.float64(0.0), t)
        t = np.where(inside, np.float64(0.0), t)
        hit = (inside | ((b > 0) & (h2 > 0))) & (t < rays["t_max"][:, None]) & (ids[None, :] != rays["ignore"][:, None])
    t = np.where(hit, t, np.inf)
    out = np.zeros(len(rays), dtype=RAY_HIT_DTYPE)
    out["t"] = t.min(axis=1) if len(ids) else np.inf
    first = hit & (t == out["t"][:, None])
    out["id"] = np.where(first, ids[None, :], np.uint64(_abi.CS_NO_HIT)).min(axis=1) if len(ids) else _abi.CS_NO_HIT
    return out


def run(agents, args):
    import bench
    from rmf_crowdsim_amd import Simulation, _abi, scenes
    from rmf_crowdsim_amd.simulation import RAY_HIT_DTYPE, rays_array
    sim = bench.build_crowd(Simulation, agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[0]
    lib, eng = sim._lib, sim._engine
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    rec = sim.read_agents()
    robots = rec[np.linspace(0, len(rec) - 1, args.robots + 2).astype(np.int64)[1:-1]]  # (none of them at an end of the crowd)
    phi = 2.0 * np.pi * np.arange(args.beams) / args.beams
    unit = np.column_stack([np.cos(phi), np.sin(phi)])
    origins = np.repeat(np.column_stack([robots["x"], robots["y"]]), args.beams, axis=0)
    directions = np.tile(unit, (len(robots), 1))
    ignore = np.repeat(robots["id"].astype(np.uint64), args.beams)
    size_max = C.c_size_t(-1).value
    out = {"agents": len(sim), "robots": len(robots), "beams": args.beams, "radius": args.radius}

    def cast(rays, rows):
        got = lib.cs_cast_rays(eng, rays.ctypes.data_as(C.POINTER(_abi.Ray)), len(rays), args.radius, None,
                               rows.ctypes.data_as(C.POINTER(_abi.RayHit)) if rows is not None else None)
        assert got != size_max, lib.cs_last_error(eng).decode()
        return got

    def host_path(rays, t_max):
        now = sim.read_agents()
        x, y, ids = now["x"], now["y"], now["id"].astype(np.uint64)
        rows = np.zeros(len(rays), dtype=RAY_HIT_DTYPE)
        reach = np.float64(t_max) + np.float64(args.radius) + 1e-6
        for k in range(len(robots)):
            near = np.nonzero((np.abs(x - robots["x"][k]) <= reach) & (np.abs(y - robots["y"][k]) <= reach))[0]
            near = near[np.hypot(x[near] - robots["x"][k], y[near] - robots["y"][k]) <= reach]
            beams = slice(k * args.beams, (k + 1) * args.beams)
            rows[beams] = host_rule(x[near], y[near], ids[near], rays[beams], args.radius)
        return rows

    for t_max in args.t_max:
        rays = rays_array(origins, directions, t_max, ignore)
        rows = np.zeros(len(rays), dtype=RAY_HIT_DTYPE)
        hits = int(cast(rays, rows))
        hit = rows["id"] != _abi.CS_NO_HIT
        row = {"rays": len(rays), "hits": hits, "mean_t_of_hits": float(rows["t"][hit].mean()) if hits else None,
               "cast": _timed(lambda: cast(rays, rows), args.warmup, args.reps),
               "count": _timed(lambda: cast(rays, None), args.warmup, args.reps)}
        if np.isfinite(t_max):
            row["host_path"] = _timed(lambda: host_path(rays, t_max), 0, args.host_reps)
            row["rows_equal"] = bool(host_path(rays, t_max).tobytes() == rows.tobytes())
        else:
            row["host_path"] = "not run"
        print(f"{agents} agents, t_max {t_max}: done", file=sys.stderr, flush=True)
        out[f"t_max {t_max}"] = row
    return out


def text(result):
    lines = []
    for r in result["runs"]:
        lines += ["", f"{r['agents']} agents, {r['robots']} robots x {r['beams']} beams, radius {r['radius']}"]
        for name, row in r.items():
            if not isinstance(row, dict):
                continue
            mean = "-" if row["mean_t_of_hits"] is None else f"{row['mean_t_of_hits']:.2f}"
            lines.append(f"  {name}: {row['hits']} of {row['rays']} rays hit, mean t of the hits {mean}; rows equal to the host "
                         f"path's: {row.get('rows_equal', '-')}")
            for form in ("cast", "count", "host_path"):
                v = row[form]
                lines.append(f"    {form:<12}" + (f"{v:>10}" if isinstance(v, str) else
                                                  f"{v['median_us']:>10.0f} us [{v['min_us']:.0f}-{v['max_us']:.0f}]"))
            if isinstance(row["host_path"], dict):
                lines.append(f"    host_path / cast {row['host_path']['median_us'] / row['cast']['median_us']:.1f}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[1_000_000])
    ap.add_argument("--robots", type=int, default=64)
    ap.add_argument("--beams", type=int, default=720)
    ap.add_argument("--radius", type=float, default=0.2)
    ap.add_argument("--t-max", type=float, nargs="*", default=[5.0, 30.0, float("inf")])
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
