"""Time cs_leg_intervals on the scene of tools/leg_conflicts_bench.py (bench.py's walk scene at 1,000,000 agents; DESIGN.md
section 2, "Every agent that enters a leg"): --paths robot paths of --legs legs of --leg-seconds each at 1 m/s, every path
starting on an agent of the crowd that its legs ignore, every fourth leg a wait; distance --distance, speed_max
--speed-max.  Two sets of the same legs:
    short          t1 as the path gives it: a reach of distance + speed_max * t1, a few cells
    stretched      every t1 raised so that the walk's reach distance + speed_max * t1 + cell is --grow metres (15)

After 20 steps, the host clock around calls that end synchronised, the median of --reps repetitions after --warmup
unrecorded ones, with the smallest and the largest beside it:
    conflicts      cs_leg_conflicts with the rows: the yardstick.  Run the tool once more with CS_LIB_PATH set to the
                   parent commit's library for the parent's number; a library without cs_leg_intervals times this alone
    count          cs_leg_intervals with out == NULL and out_counts == NULL (one kernel, one word back)
    counts         the same with out_counts (and the download of a count per leg)
    list           cs_leg_intervals with room for every row (count, emit, sort, gather, download)
The first row of every leg by (s_in, id) is compared with the row of cs_leg_conflicts.
One JSON line on stdout; --text PATH also writes the table."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from leg_conflicts_bench import _timed  # noqa: E402


def run(agents, args):
    import bench
    from rmf_crowdsim_amd import Simulation, _abi, scenes
    from rmf_crowdsim_amd.simulation import LEG_HIT_DTYPE, LEG_INTERVAL_DTYPE, legs_array
    sim = bench.build_crowd(Simulation, agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[0]
    lib, eng = sim._lib, sim._engine
    has_intervals = hasattr(lib, "cs_leg_intervals")  # (an older library chosen with CS_LIB_PATH has no such symbol)
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
           "speed_max": args.speed_max, "library_has_leg_intervals": bool(has_intervals)}

    def conflicts(legs, rows):
        got = lib.cs_leg_conflicts(eng, legs.ctypes.data_as(C.POINTER(_abi.Leg)), len(legs), args.distance, args.speed_max,
                                   None, rows.ctypes.data_as(C.POINTER(_abi.LegHit)))
        assert got != size_max, lib.cs_last_error(eng).decode()
        return got

    def ask(legs, counts, rows):
        got = lib.cs_leg_intervals(eng, legs.ctypes.data_as(C.POINTER(_abi.Leg)), len(legs), args.distance, args.speed_max, None,
                                   counts.ctypes.data_as(C.POINTER(C.c_uint64)) if counts is not None else None,
                                   rows.ctypes.data_as(C.POINTER(_abi.LegInterval)) if rows is not None else None,
                                   len(rows) if rows is not None else 0)
        assert got != size_max, lib.cs_last_error(eng).decode()
        return got

    for name, legs in (("short", short), ("stretched", stretched)):
        first = np.zeros(len(legs), dtype=LEG_HIT_DTYPE)
        row = {"legs": len(legs), "conflicts": int(conflicts(legs, first)),
               "largest_grow_m": args.distance + args.speed_max * float(legs["t1"].max()) + cell,
               "conflicts_rows": _timed(lambda: conflicts(legs, first), args.warmup, args.reps)}
        if has_intervals:
            counts = np.zeros(len(legs), dtype=np.uint64)
            total = int(ask(legs, counts, None))
            rows = np.zeros(max(total, 1), dtype=LEG_INTERVAL_DTYPE)
            assert ask(legs, None, rows) == total == int(counts.sum())
            rows = rows[:total]
            T = (legs["t1"] - legs["t0"])[rows["leg"].astype(np.int64)]
            order = np.lexsort((rows["id"], rows["s_in"], rows["leg"]))
            leg = rows["leg"][order].astype(np.int64)
            head = order[np.nonzero(np.concatenate([[True], leg[1:] != leg[:-1]]))[0]] if total else order
            mine = np.zeros(len(legs), dtype=LEG_HIT_DTYPE)
            mine["id"], mine["s"] = _abi.CS_NO_HIT, np.inf
            mine["id"][rows["leg"][head].astype(np.int64)], mine["s"][rows["leg"][head].astype(np.int64)] = rows["id"][head], rows["s_in"][head]
            row.update({"intervals": total, "legs_with_rows": int((counts > 0).sum()), "most_rows_of_a_leg": int(counts.max()),
                        "still_inside_at_t1": int((rows["s_out"] == T).sum()),
                        "first_rows_equal_conflicts": bool(mine.tobytes() == first.tobytes()),
                        "count": _timed(lambda: ask(legs, None, None), args.warmup, args.reps),
                        "counts": _timed(lambda: ask(legs, counts, None), args.warmup, args.reps),
                        "list": _timed(lambda: ask(legs, counts, rows), args.warmup, args.reps)})
        print(f"{agents} agents, {name}: done", file=sys.stderr, flush=True)
        out[name] = row
    return out


def text(result):
    lines = []
    for r in result["runs"]:
        lines += ["", f"{r['agents']} agents, {r['paths']} paths x {r['legs_per_path']} legs, distance {r['distance']}, speed_max "
                      f"{r['speed_max']}; the library has cs_leg_intervals: {r['library_has_leg_intervals']}"]
        for name in ("short", "stretched"):
            row = r[name]
            lines.append(f"  {name}: {row['conflicts']} of {row['legs']} legs conflict, largest grow {row['largest_grow_m']:.2f} m")
            if "intervals" in row:
                lines.append(f"    {row['intervals']} intervals on {row['legs_with_rows']} legs, at most {row['most_rows_of_a_leg']} on one, "
                             f"{row['still_inside_at_t1']} still inside at t1; first rows equal to cs_leg_conflicts: "
                             f"{row['first_rows_equal_conflicts']}")
            for form in ("conflicts_rows", "count", "counts", "list"):
                if form in row:
                    v = row[form]
                    lines.append(f"    {form:<15}{v['median_us']:>10.0f} us [{v['min_us']:.0f}-{v['max_us']:.0f}]")
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
    ap.add_argument("--text", default=None, help="also write the table to this file")
    args = ap.parse_args()
    result = {"reps": args.reps, "warmup": args.warmup, "runs": [run(n, args) for n in args.agents]}
    if args.text:
        with open(args.text, "w") as f:
            f.write(text(result))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
