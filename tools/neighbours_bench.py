"""Time cs_agent_neighbours on bench.py's walk scene at 1,000,000 and at 125,000 agents ("Neighbours of
each agent between steps"), against what a host had before it: listing every pair with its distance by cs_close_pairs and
reducing the list per id on the host.

After 20 steps, the host clock around calls that end synchronised, the median of --reps repetitions after --warmup
unrecorded ones, with the smallest and the largest beside it, for distance = 0.4 m and 1.5 m, with everyone x everyone and
with a small subject set (a disc of 25 m around the middle of the crowd) x everyone:
    count        cs_agent_neighbours with out == NULL and min_count = 1: how many subjects have somebody that close
    list         cs_agent_neighbours listing every subject, the isolated ones included (one counting call sizes the array
                 and is timed with it)
    min_count_1  the same listing with min_count = 1: only the subjects that have a neighbour
    parent_path  cs_close_pairs(distance, subjects, others) listing every pair with its d2 (one counting call first; with a
                 subject set also cs_select_agents for the subjects' ids), then numpy on the host: both orientations of
                 every pair, those whose first id is a subject, a lexsort by (id, d2, other id), the count and the first
                 row per id.  The parent path gives the rows of the subjects that have a neighbour only (those of
                 min_count_1); it is not charged for the isolated ones.  A pair list above CS_PAIRS_MAX cannot be listed:
                 the parent path is then "refused".
--reach-distances (default 5.0 m = 2.5 cells: 49 cells per lane, all candidates) adds rows of the three forms alone, to
see what one lane per slot costs at a large reach.
The rows of both ways are compared (min_count_1 against the parent path: the same ids, counts, nearest and d2 bits).
One JSON line on stdout; --text PATH also writes the table."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMS = ("count", "list", "min_count_1", "parent_path")


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


def host_reduce(pairs, d2, subject_ids):
    """(uint64[m, 2] pairs, float64[m] d2, the subjects' ids or None for everyone) -> (ids, counts, nearest, nearest_d2) of
    the subjects that are in a pair, ascending by id"""
    first = np.concatenate([pairs[:, 0], pairs[:, 1]])
    other = np.concatenate([pairs[:, 1], pairs[:, 0]])
    dd = np.concatenate([d2, d2])
    if subject_ids is not None:
        keep = np.isin(first, subject_ids)
        first, other, dd = first[keep], other[keep], dd[keep]
    order = np.lexsort((other, dd, first))
    first, other, dd = first[order], other[order], dd[order]
    ids, at, counts = np.unique(first, return_index=True, return_counts=True)
    return ids, counts.astype(np.uint64), other[at], dd[at]


def run(agents, args):
    import bench
    from rmf_crowdsim_amd import Simulation, _abi, scenes
    from rmf_crowdsim_amd.simulation import NEIGHBOUR_DTYPE
    sim = bench.build_crowd(Simulation, agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[0]
    lib, eng = sim._lib, sim._engine
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    rec = sim.read_agents()
    disc = _abi.Selection()
    disc.terms = _abi.CS_SEL_CIRCLE
    disc.cx, disc.cy, disc.r = float(np.median(rec["x"])), float(np.median(rec["y"])), 25.0
    out = {"agents": len(sim)}
    u64p, pairp, rowp, dblp = C.POINTER(C.c_uint64), C.POINTER(_abi.IdPair), C.POINTER(_abi.NeighbourStat), C.POINTER(C.c_double)
    size_max = C.c_size_t(-1).value

    def ref(sel):
        return C.byref(sel) if sel is not None else None

    def count(distance, sel, min_count=1):
        n = lib.cs_agent_neighbours(eng, distance, ref(sel), None, min_count, None, 0)
        assert n != size_max, lib.cs_last_error(eng).decode()
        return n

    def listing(distance, sel, min_count=0):
        n = count(distance, sel, min_count)
        rows = np.empty(max(n, 1), dtype=NEIGHBOUR_DTYPE)
        got = lib.cs_agent_neighbours(eng, distance, ref(sel), None, min_count, rows.ctypes.data_as(rowp), n)
        assert got == n, lib.cs_last_error(eng).decode()
        return rows[:n]

    def parent_path(distance, sel):
        subject_ids = None
        if sel is not None:
            k = lib.cs_select_agents(eng, ref(sel), None, 0)
            subject_ids = np.empty(max(k, 1), dtype=np.uint64)
            assert lib.cs_select_agents(eng, ref(sel), subject_ids.ctypes.data_as(u64p), k) == k
            subject_ids = subject_ids[:k]
        m = lib.cs_close_pairs(eng, distance, ref(sel), None, None, None, 0)
        assert m != size_max, lib.cs_last_error(eng).decode()
        pairs, d2 = np.empty((max(m, 1), 2), dtype=np.uint64), np.empty(max(m, 1), dtype=np.float64)
        got = lib.cs_close_pairs(eng, distance, ref(sel), None, pairs.ctypes.data_as(pairp), d2.ctypes.data_as(dblp), m)
        assert got == m, lib.cs_last_error(eng).decode()
        return host_reduce(pairs[:m], d2[:m], subject_ids)

    cases = [(d, True) for d in args.distances] + [(d, False) for d in args.reach_distances]
    for distance, with_parent in cases:
        for who, sel in (("everyone x everyone", None), ("a disc of 25 m x everyone", disc)):
            rows = listing(distance, sel)
            pairs = int(lib.cs_close_pairs(eng, distance, ref(sel), None, None, None, 0))
            row = {"subjects": int(len(rows)), "with_a_neighbour": int((rows["count"] > 0).sum()),
                   "largest_count": int(rows["count"].max()) if len(rows) else 0, "pairs": pairs}
            row["count"] = _timed(lambda: count(distance, sel), args.warmup, args.reps)
            row["list"] = _timed(lambda: listing(distance, sel), args.warmup, args.reps)
            row["min_count_1"] = _timed(lambda: listing(distance, sel, 1), args.warmup, args.reps)
            if not with_parent:
                row["parent_path"] = "not timed"
            elif pairs > _abi.CS_PAIRS_MAX:
                row["parent_path"] = "refused"
            else:
                row["parent_path"] = _timed(lambda: parent_path(distance, sel), args.warmup, args.reps)
                ids, counts, nearest, d2 = parent_path(distance, sel)
                mine = listing(distance, sel, 1)
                row["rows_equal"] = bool(np.array_equal(mine["id"], ids) and np.array_equal(mine["count"], counts)
                                         and np.array_equal(mine["nearest"], nearest)
                                         and mine["nearest_d2"].tobytes() == d2.tobytes())
                for form in FORMS[:3]:
                    row[f"parent_over_{form}"] = row["parent_path"]["median_us"] / row[form]["median_us"]
            out[f"{distance} m, {who}"] = row
            print(f"{agents} agents, {distance} m, {who}: done", file=sys.stderr, flush=True)
    return out


def text(result):
    lines = []
    for r in result["runs"]:
        lines += ["", f"{r['agents']} agents"]
        for name, row in r.items():
            if name == "agents":
                continue
            lines.append(f"  {name}: {row['subjects']} subjects, {row['with_a_neighbour']} with a neighbour, the largest count "
                         f"{row['largest_count']}; {row['pairs']} pairs on the parent path"
                         + (f", rows equal: {row['rows_equal']}" if "rows_equal" in row else ""))
            for form in FORMS:
                v = row[form]
                if isinstance(v, str):
                    lines.append(f"    {form:<14}{v:>10}")
                else:
                    lines.append(f"    {form:<14}{v['median_us']:>10.0f} us  [{v['min_us']:.0f}-{v['max_us']:.0f}]")
            if "parent_over_list" in row:
                lines.append("    " + ", ".join(f"parent_path / {f} {row['parent_over_' + f]:.2f}" for f in FORMS[:3]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[1_000_000, 125_000])
    ap.add_argument("--distances", type=float, nargs="*", default=[0.4, 1.5])
    ap.add_argument("--reach-distances", type=float, nargs="*", default=[5.0])
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
