"""usage (on the GPU): python tools/rounds_sweep.py LIB_A.so LIB_B.so [--agents 900000 950000 ...] [--steps 200]
Does the neighbour kernel's time follow whole rounds of workgroups (the chip holds 1,024 of them: 256 CUs x 4) or a
latency plus a throughput term?  For every crowd size the bench scene (walk) is timed on both builds, alternating, each
run a process of its own (`bench.py --agents N --no-cpu-baseline --no-creep-leg`), and the windows the builder listed
for a step of that scene (CS_STAT_WINDOWS_LISTED; a library without that statistic answers 0) are printed beside the
times, with the rounds they make.  One line per size and build; profiles/K4_LEVERS.md quotes the table."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = 1024  # workgroups of k_step_tiled the chip holds at once


def windows_listed(n):
    """(this process, the library of CS_LIB_PATH) windows listed for the 30th step of the bench scene at n agents"""
    sys.path.insert(0, ROOT)
    import bench
    from rmf_crowdsim_amd import Simulation, _abi, scenes
    sim, _, _ = bench.build_crowd(Simulation, n, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=60)
    for _ in range(30):
        sim.step(0.05, report=False)
    print(json.dumps({"windows": sim.kernel_stat(_abi.CS_STAT_WINDOWS_LISTED)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--agents", type=int, nargs="+", default=[900_000, 950_000, 1_000_000, 1_050_000, 1_100_000])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows-of", type=int, default=0, help="(internal) print the windows listed at this size and leave")
    args = ap.parse_args()
    if args.windows_of:
        return windows_listed(args.windows_of)
    print("agents build windows rounds k4_us step_us")
    for n in args.agents:
        for lib in args.libs:
            env = dict(os.environ, CS_LIB_PATH=os.path.abspath(lib))
            w = subprocess.run([sys.executable, os.path.abspath(__file__), "--windows-of", str(n)], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=300)
            if w.returncode != 0:  # (nothing more is started on the GPU after a failure)
                sys.exit(f"windows run failed ({w.returncode}) for {lib} at {n}:\n{w.stderr[-2000:]}")
            windows = json.loads(w.stdout.strip().splitlines()[-1])["windows"]
            b = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--agents", str(n), "--steps", str(args.steps),
                                "--warmup", "20", "--no-cpu-baseline", "--no-creep-leg"], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=600)
            if b.returncode != 0:
                sys.exit(f"bench failed ({b.returncode}) for {lib} at {n}:\n{b.stderr[-2000:]}")
            r = json.loads(b.stdout.strip().splitlines()[-1])
            name = os.path.basename(os.path.dirname(os.path.abspath(lib))) + "/" + os.path.basename(lib)
            print(f"{n} {name} {windows} {windows / SLOTS:.2f} {1e3 * r['roofline']['kernel_ms']:.1f} {1e3 * r['ms_per_step']:.1f}",
                  flush=True)


if __name__ == "__main__":
    main()
