"""Time cs_agent_field on bench.py's 1,000,000-agent walk scene ("Rasterising the crowd"), against
what a host had before it: reading the whole crowd back, binning it with numpy, or counting one rectangle per bin.

After 20 steps, the host clock around calls that end synchronised, the median of --reps repetitions after --warmup
unrecorded ones, with the smallest and the largest beside it:
    field       cs_agent_field for rasters of --sizes bins a side over the crowd: counts only, with the velocity sums,
                and counts with a one-term filter (CS_SEL_HLP: one of the two streams).  Where a raster is small enough
                for the LDS-privatised form of the kernel, it is timed in that form and (CS_FIELD_LDS_BYTES=0) in the form
                that adds to global memory; the threshold between the two is set from this table.  Every answer is
                checked against numpy binning of read_agents() (counts equal).
    read_all    (a) cs_agent_count + cs_read_agents of the whole crowd: what binning on the host must do first
    read_bin    (b) the same plus the numpy binning of a 1024 x 1024 raster (subtract, divide, truncate, bincount)
    count_zones (c) cs_count_agents with 1024 rectangles as a 32 x 32 map, beside cs_agent_field at 32 x 32
Kernel times come from a separate run under the profiler:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/field_bench.py --reps 5 --warmup 1
(k_field<true> / k_field<false> in its kernel statistics).  One JSON line on stdout."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[32, 64, 1024, 2048])
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
    out = {"agents": n, "reps": args.reps, "warmup": args.warmup, "field": {}}
    u32p, u64p, dblp, viewp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(_abi.AgentView)
    x_lo, y_lo = float(rec["x"].min()), float(rec["y"].min())
    span = max(float(rec["x"].max()) - x_lo, float(rec["y"].max()) - y_lo) * 1.0001
    one_stream = _abi.Selection()
    one_stream.terms = _abi.CS_SEL_HLP
    one_stream.hlp = 0

    def desc(side):
        d = _abi.FieldDesc()
        d.x0, d.y0, d.cell_w, d.cell_h, d.nx, d.ny = x_lo, y_lo, span / side, span / side, side, side
        return d

    def numpy_bins(d, x, y):
        fx, fy = (x - d.x0) / d.cell_w, (y - d.y0) / d.cell_h
        inside = (0.0 <= fx) & (fx < d.nx) & (0.0 <= fy) & (fy < d.ny)
        flat = fy[inside].astype(np.uint32).astype(np.int64) * d.nx + fx[inside].astype(np.uint32)
        return np.bincount(flat, minlength=d.nx * d.ny)

    for side in args.sizes:
        d = desc(side)
        bins = side * side
        count = np.zeros(bins, dtype=np.uint32)
        vx, vy = np.zeros(bins), np.zeros(bins)
        want = numpy_bins(d, rec["x"], rec["y"])
        row = {"occupied_bins": int((want > 0).sum()), "fullest_bin": int(want.max())}
        forms = [("default", None)]
        if bins * 4 <= 65536:  # (small enough for the LDS form with counts only: time the other form as well)
            forms.append(("global", "0"))
        for form, limit in forms:
            if limit is None:
                os.environ.pop("CS_FIELD_LDS_BYTES", None)
            else:
                os.environ["CS_FIELD_LDS_BYTES"] = limit
            for name, sel, with_sums in (("count", None, False), ("count_sums", None, True), ("count_filter", one_stream, False)):
                def call():
                    rc = lib.cs_agent_field(eng, C.byref(d), C.byref(sel) if sel is not None else None,
                                            count.ctypes.data_as(u32p), vx.ctypes.data_as(dblp) if with_sums else None,
                                            vy.ctypes.data_as(dblp) if with_sums else None)
                    assert rc == 0, lib.cs_last_error(eng).decode()
                entry = _timed(call, args.warmup, args.reps)
                if sel is None:
                    assert (count == want).all()
                entry["agents_binned"] = int(count.sum())
                entry["lds_bytes"] = bins * (20 if with_sums else 4)
                entry["form"] = "lds" if limit is None and entry["lds_bytes"] <= 65536 else "global"
                row[f"{name}:{form}"] = entry
        os.environ.pop("CS_FIELD_LDS_BYTES", None)
        out["field"][str(side)] = row

    # (a) the read-back alone, (b) with the numpy binning of 1024 x 1024
    buf = np.zeros(n, dtype=np.dtype(_abi.AgentView))

    def read_all():
        got = lib.cs_read_agents(eng, buf.ctypes.data_as(viewp), lib.cs_agent_count(eng))
        assert got == n
    out["read_all"] = _timed(read_all, args.warmup, args.reps)
    d1k = desc(1024)

    def read_bin():
        read_all()
        numpy_bins(d1k, buf["x"], buf["y"])
    out["read_bin_1024"] = _timed(read_bin, min(args.warmup, 2), min(args.reps, 10))

    # (c) 1024 rectangles as a 32 x 32 map
    d32 = desc(32)
    zones = (_abi.Selection * 1024)()
    for k in range(1024):
        iy, ix = divmod(k, 32)
        zones[k].terms = _abi.CS_SEL_RECT
        zones[k].x0, zones[k].x1 = d32.x0 + ix * d32.cell_w, d32.x0 + (ix + 1) * d32.cell_w
        zones[k].y0, zones[k].y1 = d32.y0 + iy * d32.cell_h, d32.y0 + (iy + 1) * d32.cell_h
    counts = np.zeros(1024, dtype=np.uint64)

    def count_zones():
        rc = lib.cs_count_agents(eng, zones, 1024, counts.ctypes.data_as(u64p))
        assert rc == 0, lib.cs_last_error(eng).decode()
    out["count_zones_32x32"] = _timed(count_zones, args.warmup, args.reps)
    assert int(counts.sum()) > 0.99 * n  # (the rectangles' edges are products, the raster's a quotient: a few agents differ)

    # the two conditions of the feature
    f1k = out["field"].get("1024", {}).get("count:default")
    f32 = out["field"].get("32", {}).get("count:default")
    if f1k:
        out["field_1024_count_vs_read_all"] = out["read_all"]["median_us"] / f1k["median_us"]
    if f32:
        out["field_32_count_vs_count_zones"] = out["count_zones_32x32"]["median_us"] / f32["median_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
