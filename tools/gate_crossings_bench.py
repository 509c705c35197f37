"""Time cs_gate_crossings on bench.py's walk scene at 1,000,000 agents ("Who crosses a line"): two
sets of gates across the flow (the crowd walks +x), window 0 .. --window seconds, speed_max --speed-max:
    doors          --doors gates of --door metres (4,096 of 2 m), each one metre ahead of an agent of the crowd
    long           --long gates of --long-metres metres (64 of 100 m), spread over the crowd

After 20 steps, the host clock around calls that end synchronised, the median of --reps repetitions after --warmup
unrecorded ones, with the smallest and the largest beside it:
    count          cs_gate_crossings with out == NULL and out_counts == NULL (one kernel, one word back)
    counts         the same with out_counts (and the download of two counts per gate)
    list           cs_gate_crossings with room for every row (count, emit, sort, gather, download)
    host           the path the call replaces: read_agents() and the rule in numpy, one gate at a time over all agents.
                   For the doors it is timed on the first --host-doors gates and scaled to all of them (it is linear in
                   the gates); its rows for the gates it ran are compared with the device's, bit for bit.
The VGPRs and the private segment of k_gate_count and k_gate_emit are read from the loaded code object
(hipFuncGetAttributes).  One JSON line on stdout; --text PATH also writes the table."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from leg_conflicts_bench import _timed  # noqa: E402


def host_rule(x, y, vx, vy, ids, gate, k, speed_max):
    """The rule of include/crowdstep_state.h for one gate against the agents (x, y, vx, vy, ids: ascending), one numpy
    operation each -> its GATE_CROSSING_DTYPE rows"""
    from rmf_crowdsim_amd.simulation import GATE_CROSSING_DTYPE
    S2 = np.float64(speed_max) * np.float64(speed_max)
    ax, ay, t0 = gate["ax"], gate["ay"], gate["t0"]
    T = gate["t1"] - gate["t0"]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        slow = vx * vx + vy * vy < S2
        px, py = x + vx * t0, y + vy * t0
        ex, ey = gate["bx"] - ax, gate["by"] - ay
        rx, ry = px - ax, py - ay
        c0 = ex * ry - ey * rx
        cv = ex * vy - ey * vx
        cu = rx * vy - ry * vx
        towards = ((cv > 0) & (c0 <= 0)) | ((cv < 0) & (c0 >= 0))
        s = (-c0) / cv
        s = np.where(s > 0, s, np.float64(0.0))
        u = cu / cv
        hit = np.nonzero(slow & towards & (s < T) & (u >= 0) & (u < 1))[0]
    rows = np.zeros(len(hit), dtype=GATE_CROSSING_DTYPE)
    rows["gate"], rows["dir"], rows["id"], rows["s"], rows["u"] = k, np.where(cv[hit] > 0, 1, -1), ids[hit], s[hit], u[hit]
    return rows


def host_path(sim, gates, speed_max):
    """read_agents() and host_rule over `gates` -> the rows, ascending by (gate, id)"""
    rec = sim.read_agents()
    rec = rec[np.argsort(rec["id"], kind="stable")]
    x, y = rec["x"].astype(np.float64), rec["y"].astype(np.float64)
    vx, vy = rec["vx"].astype(np.float32).astype(np.float64), rec["vy"].astype(np.float32).astype(np.float64)
    ids = rec["id"].astype(np.uint64)
    return np.concatenate([host_rule(x, y, vx, vy, ids, g, k, speed_max) for k, g in enumerate(gates)])


def kernel_resources(lib_path):
    """{kernel: (VGPRs, private segment bytes)} of the two kernels as the runtime loaded them; {} where it cannot tell"""
    class Attr(C.Structure):
        _fields_ = [("binaryVersion", C.c_int), ("cacheModeCA", C.c_int), ("constSizeBytes", C.c_size_t),
                    ("localSizeBytes", C.c_size_t), ("maxDynamicSharedSizeBytes", C.c_int), ("maxThreadsPerBlock", C.c_int),
                    ("numRegs", C.c_int), ("preferredShmemCarveout", C.c_int), ("ptxVersion", C.c_int),
                    ("sharedSizeBytes", C.c_size_t)]
    out = {}
    try:
        names = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, timeout=60).stdout
        lib, hip = C.CDLL(lib_path), C.CDLL("libamdhip64.so")
        hip.hipFuncGetAttributes.argtypes = [C.POINTER(Attr), C.c_void_p]
        for kernel in ("k_gate_count", "k_gate_emit"):
            handle = [ln.split()[-1] for ln in names.splitlines() if f"{len(kernel)}{kernel}7GridDev" in ln and " D " in ln]
            attr = Attr()
            if len(handle) == 1 and hip.hipFuncGetAttributes(C.byref(attr), C.addressof(C.c_void_p.in_dll(lib, handle[0]))) == 0:
                out[kernel] = (int(attr.numRegs), int(attr.localSizeBytes))
    except (OSError, ValueError, subprocess.SubprocessError):
        pass
    return out


def run(agents, args):
    import bench
    from rmf_crowdsim_amd import Simulation, _abi, _native, scenes
    from rmf_crowdsim_amd.simulation import GATE_CROSSING_DTYPE, gates_array
    sim = bench.build_crowd(Simulation, agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[0]
    lib, eng = sim._lib, sim._engine
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    rec = sim.read_agents()
    at = rec[np.linspace(0, len(rec) - 1, args.doors + 2).astype(np.int64)[1:-1]]  # (none of them at an end of the crowd)
    half = 0.5 * args.door
    doors = gates_array(np.column_stack([at["x"] + 1.0, at["y"] - half, at["x"] + 1.0, at["y"] + half]), 0.0, args.window)
    lo_x, hi_x, mid_y = float(rec["x"].min()), float(rec["x"].max()), float(np.median(rec["y"]))
    xs = np.linspace(lo_x, hi_x, args.long + 2)[1:-1]
    half = 0.5 * args.long_metres
    long_ = gates_array(np.column_stack([xs, np.full_like(xs, mid_y - half), xs, np.full_like(xs, mid_y + half)]), 0.0, args.window)
    size_max = C.c_size_t(-1).value
    out = {"agents": len(sim), "window": args.window, "speed_max": args.speed_max,
           "kernel_resources": kernel_resources(os.environ.get("CS_LIB_PATH") or _native.build())}

    def ask(gates, counts, rows):
        got = lib.cs_gate_crossings(eng, gates.ctypes.data_as(C.POINTER(_abi.Gate)), len(gates), args.speed_max, None,
                                    counts.ctypes.data_as(C.POINTER(C.c_uint64)) if counts is not None else None,
                                    rows.ctypes.data_as(C.POINTER(_abi.GateCrossing)) if rows is not None else None,
                                    len(rows) if rows is not None else 0)
        assert got != size_max, lib.cs_last_error(eng).decode()
        return got

    for name, gates, on_host in (("doors", doors, min(args.host_doors, len(doors))), ("long", long_, len(long_))):
        counts = np.zeros((len(gates), 2), dtype=np.uint64)
        total = int(ask(gates, counts, None))
        rows = np.zeros(max(total, 1), dtype=GATE_CROSSING_DTYPE)
        assert ask(gates, None, rows) == total == int(counts.sum())
        rows = rows[:total]
        t0 = time.perf_counter()
        host = host_path(sim, gates[:on_host], args.speed_max)
        host_us = (time.perf_counter() - t0) * 1e6
        row = {"gates": len(gates), "metres": float(np.hypot(gates["bx"] - gates["ax"], gates["by"] - gates["ay"]).max()),
               "crossings": total, "to_the_left": int(counts[:, 0].sum()), "to_the_right": int(counts[:, 1].sum()),
               "gates_with_rows": int((counts.sum(axis=1) > 0).sum()), "most_rows_of_a_gate": int(counts.sum(axis=1).max()),
               "host_gates": on_host, "host_us_measured": host_us, "host_us_all_gates": host_us * len(gates) / max(on_host, 1),
               "host_rows_equal": bool(host.tobytes() == rows[rows["gate"] < on_host].tobytes()),
               "count": _timed(lambda: ask(gates, None, None), args.warmup, args.reps),
               "counts": _timed(lambda: ask(gates, counts, None), args.warmup, args.reps),
               "list": _timed(lambda: ask(gates, counts, rows), args.warmup, args.reps)}
        print(f"{agents} agents, {name}: done", file=sys.stderr, flush=True)
        out[name] = row
    return out


def text(result):
    lines = []
    for r in result["runs"]:
        lines += ["", f"{r['agents']} agents, window 0 .. {r['window']} s, speed_max {r['speed_max']}; (VGPRs, private segment bytes): "
                      f"{r['kernel_resources']}"]
        for name in ("doors", "long"):
            row = r[name]
            lines.append(f"  {name}: {row['gates']} gates of {row['metres']:.0f} m: {row['crossings']} crossings ({row['to_the_left']} to the "
                         f"left, {row['to_the_right']} to the right) on {row['gates_with_rows']} gates, at most "
                         f"{row['most_rows_of_a_gate']} on one")
            for form in ("count", "counts", "list"):
                v = row[form]
                lines.append(f"    {form:<15}{v['median_us']:>12.0f} us [{v['min_us']:.0f}-{v['max_us']:.0f}]")
            lines.append(f"    {'host':<15}{row['host_us_all_gates']:>12.0f} us (read_agents() and numpy; measured on {row['host_gates']} gates: "
                         f"{row['host_us_measured']:.0f} us; its rows equal the device's: {row['host_rows_equal']})")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[1_000_000])
    ap.add_argument("--doors", type=int, default=4096)
    ap.add_argument("--door", type=float, default=2.0)
    ap.add_argument("--long", type=int, default=64)
    ap.add_argument("--long-metres", type=float, default=100.0)
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--speed-max", type=float, default=2.0)
    ap.add_argument("--host-doors", type=int, default=64)
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
