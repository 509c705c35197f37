"""Time cs_zone_agents on bench.py's walk scene at 1,000,000 agents ("Agents in polygon zones between
steps").  After 20 steps, three sets of zones over the crowd's bounding box:
    rectangles     a floor plan of --side x --side (32 x 32 = 1,024) rectangles that tile the box, as four-vertex zones,
                   against the same 1,024 CS_SEL_RECT selections through cs_count_agents: the counts are asserted equal
    rooms          in each of those rectangles an eight-vertex concave room (a notch cut into its high side)
    whole          one four-vertex zone over the whole grid

The host clock around calls that end synchronised, the median of --reps repetitions after --warmup unrecorded ones, with
the smallest and the largest beside it:
    count_agents   cs_count_agents on the 1,024 rectangle selections (rectangles only): the yardstick
    count          cs_zone_agents with out == NULL and out_counts == NULL (one kernel, one word back)
    counts         the same with out_counts (and the download of a count per zone)
    list           cs_zone_agents with room for every row (count, emit, sort, download)
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
    from rmf_crowdsim_amd.simulation import ZONE_AGENT_DTYPE, zones_array
    sim = bench.build_crowd(Simulation, agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[0]
    lib, eng = sim._lib, sim._engine
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    rec = sim.read_agents()
    x0, x1 = float(rec["x"].min()), float(np.nextafter(rec["x"].max(), np.inf))
    y0, y1 = float(rec["y"].min()), float(np.nextafter(rec["y"].max(), np.inf))
    xs, ys = np.linspace(x0, x1, args.side + 1), np.linspace(y0, y1, args.side + 1)
    boxes = [(xs[i], ys[j], xs[i + 1], ys[j + 1]) for i in range(args.side) for j in range(args.side)]
    rects = [np.array([(a, b), (c, b), (c, d), (a, d)]) for a, b, c, d in boxes]
    rooms = []
    for a, b, c, d in boxes:
        w, h = c - a, d - b
        rooms.append(np.array([(a, b), (c, b), (c, d), (a + 0.6 * w, d), (a + 0.6 * w, b + 0.5 * h), (a + 0.3 * w, b + 0.5 * h),
                               (a + 0.3 * w, d), (a, d)]))
    whole = [np.array([(-1e7, -1e7), (1e7, -1e7), (1e7, 1e7), (-1e7, 1e7)])]
    sels = (_abi.Selection * len(boxes))()
    for s, (a, b, c, d) in zip(sels, boxes):
        s.terms, s.x0, s.y0, s.x1, s.y1 = _abi.CS_SEL_RECT, a, b, c, d
    by_count = np.zeros(len(boxes), dtype=np.uint64)
    size_max = C.c_size_t(-1).value
    out = {"agents": len(sim), "side": args.side, "box_m": [x0, y0, x1, y1]}

    def count_agents():
        rc = lib.cs_count_agents(eng, sels, len(boxes), by_count.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert rc == 0, lib.cs_last_error(eng).decode()

    def ask(zones, vertices, counts, rows):
        got = lib.cs_zone_agents(eng, zones.ctypes.data_as(C.POINTER(_abi.Zone)), len(zones),
                                 vertices.ctypes.data_as(C.POINTER(C.c_double)), len(vertices), None,
                                 counts.ctypes.data_as(C.POINTER(C.c_uint64)) if counts is not None else None,
                                 rows.ctypes.data_as(C.POINTER(_abi.ZoneAgent)) if rows is not None else None,
                                 len(rows) if rows is not None else 0)
        assert got != size_max, lib.cs_last_error(eng).decode()
        return got

    for name, rings in (("rectangles", rects), ("rooms", rooms), ("whole", whole)):
        zones, vertices = zones_array(rings)
        counts = np.zeros(len(zones), dtype=np.uint64)
        total = int(ask(zones, vertices, counts, None))
        rows = np.zeros(max(total, 1), dtype=ZONE_AGENT_DTYPE)
        assert ask(zones, vertices, None, rows) == total == int(counts.sum())
        row = {"zones": len(zones), "vertices": len(vertices), "rows": total, "most_in_a_zone": int(counts.max())}
        if name == "rectangles":
            count_agents()
            assert by_count.tobytes() == counts.tobytes() and total == len(rec)
            row["counts_equal_count_agents"] = True
            row["count_agents"] = _timed(count_agents, args.warmup, args.reps)
        if name == "whole":
            assert total == len(rec) and np.array_equal(rows["id"][:total], np.sort(rec["id"]).astype(np.uint64))
        row.update({"count": _timed(lambda: ask(zones, vertices, None, None), args.warmup, args.reps),
                    "counts": _timed(lambda: ask(zones, vertices, counts, None), args.warmup, args.reps),
                    "list": _timed(lambda: ask(zones, vertices, counts, rows), args.warmup, args.reps)})
        print(f"{agents} agents, {name}: done", file=sys.stderr, flush=True)
        out[name] = row
    return out


def text(result):
    lines = []
    for r in result["runs"]:
        lines += ["", f"{r['agents']} agents, a floor plan of {r['side']} x {r['side']} zones over the crowd's box "
                      f"{[round(v, 1) for v in r['box_m']]} m"]
        for name in ("rectangles", "rooms", "whole"):
            row = r[name]
            lines.append(f"  {name}: {row['zones']} zones, {row['vertices']} vertices, {row['rows']} rows, at most "
                         f"{row['most_in_a_zone']} in one zone"
                         + ("; counts equal to cs_count_agents" if row.get("counts_equal_count_agents") else ""))
            for form in ("count_agents", "count", "counts", "list"):
                if form in row:
                    v = row[form]
                    lines.append(f"    {form:<15}{v['median_us']:>10.0f} us [{v['min_us']:.0f}-{v['max_us']:.0f}]")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[1_000_000])
    ap.add_argument("--side", type=int, default=32)
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
