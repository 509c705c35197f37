"""Time cs_select_agents and cs_count_agents on bench.py's 1,000,000-agent walk scene ("Selecting
agents"), against the only other route to the same answer: read_agents() of the whole crowd plus a numpy filter.

After 20 warm-up steps, the host clock around calls that end synchronised, the median of --reps repetitions with the
smallest and the largest beside it:
    route         cs_agent_count + cs_read_agents of the whole crowd, then the numpy mask of the rectangle and the ids
                  (the read alone is reported beside it); per selection size, since the filter's cost varies with it
    select        cs_select_agents of a centred rectangle sized for ~10^2, ~10^4 and all agents (--select-k), ids
                  written into a buffer of the crowd's size; the answer is checked against the route's
    select_speed  the same rectangles with a CS_SEL_SPEED term (the pass reads the velocities too: 28 B per slot)
    count         cs_count_agents of 1, 32 and 1024 rectangles of a lattice over the crowd (--zones)
Also derived: the selection pass against what it must read (20 B per live slot, 28 B with a speed term) at --hbm-gbs, and
the 1024-zone count in compares per second.  Kernel times come from a separate run under the profiler:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/select_bench.py --reps 1
(k_select, k_select_count, k_ids_hist / k_ids_scan / k_ids_scatter in its kernel statistics).
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
    ap.add_argument("--select-k", type=int, nargs="*", default=[100, 10_000, 1_000_000])
    ap.add_argument("--zones", type=int, nargs="*", default=[1, 32, 1024])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the chip's HBM rate the pass is set against (GB/s)")
    args = ap.parse_args()
    import bench
    from rmf_crowdsim_amd import Simulation, _abi, scenes
    sim, _ = bench.build_crowd(Simulation, args.agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[:2]
    lib, eng = sim._lib, sim._engine
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    rec = sim.read_agents()
    n = len(rec)
    out = {"agents": n, "route": {}, "select": {}, "select_speed": {}, "count": {}}
    u64p, viewp = C.POINTER(C.c_uint64), C.POINTER(_abi.AgentView)
    cx, cy = float(np.median(rec["x"])), float(np.median(rec["y"]))
    order_x, order_y = np.sort(np.abs(rec["x"] - cx)), np.sort(np.abs(rec["y"] - cy))

    def rectangle(k):
        """a centred rectangle that holds about k agents (the crowd is uniform: a fraction sqrt(k / n) of each axis)"""
        sel = _abi.Selection()
        sel.terms = _abi.CS_SEL_RECT
        if k >= n:
            sel.x0 = sel.y0 = -np.inf
            sel.x1 = sel.y1 = np.inf
            return sel
        at = min(n - 1, int(np.sqrt(k / n) * n))
        sel.x0, sel.x1, sel.y0, sel.y1 = cx - order_x[at], cx + order_x[at], cy - order_y[at], cy + order_y[at]
        return sel

    buf = np.zeros(n, dtype=np.dtype(_abi.AgentView))
    ids = np.zeros(n, dtype=np.uint64)
    read_only = []
    for k in args.select_k:
        sel = rectangle(k)
        route, want = [], None
        for rep in range(args.reps + 1):  # (the first repetition warms up)
            t0 = time.perf_counter()
            count = lib.cs_agent_count(eng)
            got = lib.cs_read_agents(eng, buf.ctypes.data_as(viewp), count)
            t1 = time.perf_counter()
            x, y = buf["x"][:got], buf["y"][:got]
            mask = (sel.x0 <= x) & (x < sel.x1) & (sel.y0 <= y) & (y < sel.y1)
            want = buf["id"][:got][mask].copy()
            t2 = time.perf_counter()
            assert got == n
            if rep:
                route.append((t2 - t0) * 1e6)
                read_only.append((t1 - t0) * 1e6)
        out["route"][str(k)] = dict(_stats(route), selected=int(len(want)))
        for name, terms in (("select", _abi.CS_SEL_RECT), ("select_speed", _abi.CS_SEL_RECT | _abi.CS_SEL_SPEED)):
            sel.terms, sel.speed_lo, sel.speed_hi = terms, 0.0, np.inf
            us = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                found = lib.cs_select_agents(eng, C.byref(sel), ids.ctypes.data_as(u64p), n)
                t1 = time.perf_counter()
                assert found == len(want) and (ids[:found] == want).all(), lib.cs_last_error(eng).decode()
                if rep:
                    us.append((t1 - t0) * 1e6)
            out[name][str(k)] = dict(_stats(us), selected=int(found),
                                     ratio_to_route=out["route"][str(k)]["median_us"] / float(np.median(us)))
    out["read_all"] = _stats(read_only)
    # the count only (no sort, no download): the pass itself, against the bytes it must read
    sel = rectangle(args.select_k[0] if args.select_k else 100)
    for name, terms, per_slot in (("pass_20B", _abi.CS_SEL_RECT, 20), ("pass_28B", _abi.CS_SEL_RECT | _abi.CS_SEL_SPEED, 28)):
        sel.terms, sel.speed_lo, sel.speed_hi = terms, 0.0, np.inf
        us = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            lib.cs_select_agents(eng, C.byref(sel), None, 0)
            t1 = time.perf_counter()
            if rep:
                us.append((t1 - t0) * 1e6)
        ideal_us = n * per_slot / (args.hbm_gbs * 1e9) * 1e6
        out[name] = dict(_stats(us), ideal_us=ideal_us, fraction_of_hbm_rate=ideal_us / float(np.median(us)))

    # zones: a lattice of rectangles over the crowd
    x_lo, x_hi, y_lo, y_hi = (float(v) for v in (rec["x"].min(), rec["x"].max(), rec["y"].min(), rec["y"].max()))
    for z in args.zones:
        side = int(np.ceil(np.sqrt(z)))
        zones = (_abi.Selection * z)()
        for k in range(z):
            i, j = divmod(k, side)
            zones[k].terms = _abi.CS_SEL_RECT
            zones[k].x0 = x_lo + (x_hi - x_lo) * i / side
            zones[k].x1 = x_lo + (x_hi - x_lo) * (i + 1) / side
            zones[k].y0 = y_lo + (y_hi - y_lo) * j / side
            zones[k].y1 = y_lo + (y_hi - y_lo) * (j + 1) / side
        counts = np.zeros(z, dtype=np.uint64)
        us = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            rc = lib.cs_count_agents(eng, zones, z, counts.ctypes.data_as(u64p))
            t1 = time.perf_counter()
            assert rc == 0, lib.cs_last_error(eng).decode()
            if rep:
                us.append((t1 - t0) * 1e6)
        # the route: the whole crowd, then one mask per zone
        route = []
        for rep in range((min(args.reps, 2) if z <= 32 else 0) + 1):  # (1024 masks over the crowd take seconds)
            t0 = time.perf_counter()
            got = lib.cs_read_agents(eng, buf.ctypes.data_as(viewp), lib.cs_agent_count(eng))
            x, y = buf["x"][:got], buf["y"][:got]
            want = [int(((zones[k].x0 <= x) & (x < zones[k].x1) & (zones[k].y0 <= y) & (y < zones[k].y1)).sum()) for k in range(z)]
            t1 = time.perf_counter()
            if rep or z > 32:
                route.append((t1 - t0) * 1e6)
        assert counts.tolist() == want
        med = float(np.median(us))
        out["count"][str(z)] = dict(_stats(us), route_median_us=float(np.median(route)),
                                    ratio_to_route=float(np.median(route)) / med, compares_per_s=n * z / (med * 1e-6),
                                    counted=int(counts.sum()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
