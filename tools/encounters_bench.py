"""Time cs_encounters on bench.py's walk scene at 1,000,000 and at 125,000 agents ("Encounters between
steps"), against two yardsticks: the count of the pairs in range, which is the same walk without the velocity load and the
arithmetic, and what a host had before the call: listing every pair in range with its distance, fetching the agents of the
pairs by id and doing the arithmetic in numpy.

After 20 steps, the host clock around calls that end synchronised, the median of --reps repetitions after --warmup
unrecorded ones, with the smallest and the largest beside it, for (distance, horizon, range) = (0.5, 3.0, 4.0) and
(1.5, 2.0, 6.0):
    count          cs_encounters, the count-only form
    list           cs_encounters listing every row (one counting call sizes the array and is timed with it)
    robots_*       the same two forms with 8 robots (agents of a NoLocalPlan planner added into the crowd) against everyone
    pairs_count    yardstick (a): cs_close_pairs(range), the count-only form (robots_pairs_count: robots against everyone)
    parent_path    yardstick (b): cs_close_pairs(range) listing every pair with its d2 (one counting call first),
                   cs_read_agents_by_id of the agents in a pair, and the rule of the header in numpy on the host
                   (robots_parent_path: robots against everyone).  A pair list above CS_PAIRS_MAX cannot be listed: the
                   parent path is then "refused", as is a listing of more encounters than that.
The rows of both ways are compared (the same ids and the same bits of t and d2).
A library without cs_encounters (the parent commit's, chosen with CS_LIB_PATH) is timed on the two yardsticks alone;
--parent-json PATH folds the JSON line of such a run into the table of this one.
One JSON line on stdout; --text PATH also writes the table."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMS = ("count", "pairs_count", "list", "parent_path", "robots_count", "robots_pairs_count", "robots_list",
         "robots_parent_path")


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


def host_rule(pairs, rec_of, ids, distance, horizon):
    """(uint64[m, 2] pairs in range, the records of `ids` (ascending), distance, horizon) -> (keep mask, t, m2): the rule
    of include/crowdstep_state.h, one numpy operation each"""
    at = np.searchsorted(ids, pairs)
    p, q = at[:, 0], at[:, 1]
    x, y = rec_of["x"], rec_of["y"]
    vx, vy = rec_of["vx"].astype(np.float32).astype(np.float64), rec_of["vy"].astype(np.float32).astype(np.float64)
    rx, ry, wx, wy = x[q] - x[p], y[q] - y[p], vx[q] - vx[p], vy[q] - vy[p]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ww = wx * wx + wy * wy
        rw = rx * wx + ry * wy
        free = (-rw) / ww
        free = np.where(free < horizon, free, np.float64(horizon))
        t = np.where(rw < 0, free, np.float64(0.0))
        cx, cy = rx + wx * t, ry + wy * t
        m2 = cx * cx + cy * cy
        keep = m2 < np.float64(distance) * np.float64(distance)
    return keep, t, m2


def run(agents, args):
    import bench
    from rmf_crowdsim_amd import NoLocalPlan, Simulation, StubHighLevelPlan, _abi, scenes
    from rmf_crowdsim_amd.simulation import AGENT_DTYPE, ENCOUNTER_DTYPE as row_dtype
    sim = bench.build_crowd(Simulation, agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[0]
    lib, eng = sim._lib, sim._engine
    have = hasattr(lib, "cs_encounters")
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    rec = sim.read_agents()
    # 8 robots standing in the crowd, a third of a metre from an agent each
    nolp = NoLocalPlan()
    picks = rec[np.linspace(0, len(rec) - 1, 8).astype(np.int64)]
    sim.add_agents(np.stack([picks["x"] + 0.3, picks["y"] + 0.1], axis=1), StubHighLevelPlan((0.0, 0.0)), nolp, 2.0)
    robots = _abi.Selection()
    robots.terms = _abi.CS_SEL_LP
    robots.lp = sim._planner_handles[id(nolp)]
    out = {"agents": len(sim), "library_has_encounters": have}
    pairp, dblp, u64p, viewp = C.POINTER(_abi.IdPair), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(_abi.AgentView)
    size_max = C.c_size_t(-1).value

    def ref(sel):
        return C.byref(sel) if sel is not None else None

    def count(numbers, sel):
        got = lib.cs_encounters(eng, *numbers, ref(sel), None, None, 0)
        assert got != size_max, lib.cs_last_error(eng).decode()
        return got

    def listing(numbers, sel):
        m = count(numbers, sel)
        rows = np.empty(max(m, 1), dtype=row_dtype)
        got = lib.cs_encounters(eng, *numbers, ref(sel), None, rows.ctypes.data_as(C.POINTER(_abi.Encounter)), m)
        assert got == m, lib.cs_last_error(eng).decode()
        return rows[:m]

    def pairs_count(range_, sel):
        got = lib.cs_close_pairs(eng, range_, ref(sel), None, None, None, 0)
        assert got != size_max, lib.cs_last_error(eng).decode()
        return got

    def parent_path(numbers, sel):
        distance, horizon, range_ = numbers
        m = pairs_count(range_, sel)
        pairs, d2 = np.empty((max(m, 1), 2), dtype=np.uint64), np.empty(max(m, 1))
        got = lib.cs_close_pairs(eng, range_, ref(sel), None, pairs.ctypes.data_as(pairp), d2.ctypes.data_as(dblp), m)
        assert got == m, lib.cs_last_error(eng).decode()
        pairs = pairs[:m]
        ids = np.unique(pairs)
        rec_of = np.zeros(max(len(ids), 1), dtype=AGENT_DTYPE)
        rc = lib.cs_read_agents_by_id(eng, ids.ctypes.data_as(u64p), len(ids), rec_of.ctypes.data_as(viewp), None)
        assert rc == 0, lib.cs_last_error(eng).decode()
        keep, t, m2 = host_rule(pairs, rec_of, ids, distance, horizon)
        rows = np.empty(int(keep.sum()), dtype=row_dtype)
        rows["a"], rows["b"], rows["t"], rows["d2"] = pairs[keep, 0], pairs[keep, 1], t[keep], m2[keep]
        return rows

    for numbers in args.queries:
        name = "distance {}, horizon {}, range {}".format(*numbers)
        row = {}
        for prefix, sel in (("", None), ("robots_", robots)):
            in_range = int(pairs_count(numbers[2], sel))
            row[prefix + "pairs_in_range"] = in_range
            row[prefix + "pairs_count"] = _timed(lambda: pairs_count(numbers[2], sel), args.warmup, args.reps)
            found = None
            if have:
                found = int(count(numbers, sel))
                row[prefix + "encounters"] = found
                row[prefix + "count"] = _timed(lambda: count(numbers, sel), args.warmup, args.reps)
                row[prefix + "list"] = ("refused" if found > _abi.CS_PAIRS_MAX else
                                        _timed(lambda: listing(numbers, sel), args.warmup, args.reps))
            if in_range > _abi.CS_PAIRS_MAX:
                row[prefix + "parent_path"] = "refused"
            else:
                row[prefix + "parent_path"] = _timed(lambda: parent_path(numbers, sel), 1, args.parent_reps)
                if have and found <= _abi.CS_PAIRS_MAX:
                    row[prefix + "rows_equal"] = bool(parent_path(numbers, sel).tobytes() == listing(numbers, sel).tobytes())
            print(f"{agents} agents, {name}, {prefix or 'everyone'}: done", file=sys.stderr, flush=True)
        out[name] = row
    return out


def text(result, parent=None):
    lines = []
    for k, r in enumerate(result["runs"]):
        lines += ["", f"{r['agents']} agents"]
        for name, row in r.items():
            if not isinstance(row, dict):
                continue
            lines.append(f"  {name}: {row.get('encounters', '-')} encounters of {row['pairs_in_range']} pairs in range; with a robot "
                         f"{row.get('robots_encounters', '-')} of {row['robots_pairs_in_range']}; rows equal to the parent path's: "
                         f"{row.get('rows_equal', '-')} / {row.get('robots_rows_equal', '-')}")
            other = parent["runs"][k].get(name, {}) if parent else {}
            for form in FORMS:
                cells = []
                for label, v in (("this", row.get(form)), ("parent library", other.get(form))):
                    if v is None:
                        continue
                    cells.append(f"{label} {v:>10}" if isinstance(v, str) else
                                 f"{label} {v['median_us']:>10.0f} us [{v['min_us']:.0f}-{v['max_us']:.0f}]")
                if cells:
                    lines.append(f"    {form:<20}" + "   ".join(cells))
            for prefix in ("", "robots_"):
                c, p = row.get(prefix + "count"), row.get(prefix + "pairs_count")
                if isinstance(c, dict) and isinstance(p, dict):
                    lines.append(f"    {prefix}count / {prefix}pairs_count {c['median_us'] / p['median_us']:.2f}")
                ls = row.get(prefix + "list")
                for label, src in (("this library", row), ("the parent library", other)):
                    pp = src.get(prefix + "parent_path")
                    if isinstance(ls, dict) and isinstance(pp, dict):
                        lines.append(f"    {prefix}parent_path ({label}) / {prefix}list {pp['median_us'] / ls['median_us']:.2f}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[1_000_000, 125_000])
    ap.add_argument("--queries", type=float, nargs="*", default=[0.5, 3.0, 4.0, 1.5, 2.0, 6.0],
                    help="distance horizon range, three numbers per query")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-reps", type=int, default=3)
    ap.add_argument("--parent-json", default=None, help="the JSON line of a run on the parent commit's library")
    ap.add_argument("--text", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if len(args.queries) % 3:
        ap.error("--queries takes three numbers per query")
    args.queries = [tuple(args.queries[k:k + 3]) for k in range(0, len(args.queries), 3)]
    result = {"reps": args.reps, "warmup": args.warmup, "parent_reps": args.parent_reps,
              "runs": [run(n, args) for n in args.agents]}
    if args.text:
        parent = json.loads(open(args.parent_json).read().strip().splitlines()[-1]) if args.parent_json else None
        with open(args.text, "w") as f:
            f.write(text(result, parent))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
