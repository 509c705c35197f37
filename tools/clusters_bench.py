"""Time cs_agent_clusters on bench.py's walk scene at 1,000,000 and at 125,000 agents ("Clusters of
agents between steps"), against what a host had before it: listing every pair with cs_close_pairs and merging them on the
host.

After 20 steps, the host clock around calls that end synchronised, the median of --reps repetitions after --warmup
unrecorded ones, with the smallest and the largest beside it, for distance = 0.4 m and 1.5 m, with everyone and with the
agents slower than 0.2 m/s (speed=(0, 0.2)) as members:
    count        cs_agent_clusters with every output NULL but the two counts
    list         cs_agent_clusters listing every member with its label and every cluster row (one counting call sizes the
                 arrays and is timed with it)
    jams         the same listing with min_size = 8: only the clusters a jam detector would look at
    parent_path  cs_close_pairs(distance, members, members) listing every pair (one counting call first), then connected
                 components over the list on the host: scipy.sparse.csgraph.connected_components if scipy is importable,
                 otherwise a numpy union by repeated label minimisation; the JSON says which.  The parent path gives the
                 labels of the agents that are in a pair only; it is not charged for the singletons, the sizes, the boxes
                 or the sums.
The numbers of clusters of both ways are printed side by side (the parent's: components of the pair list).
One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    HOST_MERGE = "scipy.sparse.csgraph.connected_components"
except ImportError:  # (not a fallback of the engine: the host half of the parent path, as the host would write it)
    connected_components = None
    HOST_MERGE = "numpy: labels minimised over the pair list until nothing changes"


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


def host_components(pairs):
    """the number of connected components of the graph of a uint64[n, 2] pair list (over the ids that are in a pair)"""
    if len(pairs) == 0:
        return 0
    ids, flat = np.unique(pairs, return_inverse=True)
    edges = flat.reshape(-1, 2)
    n = len(ids)
    if connected_components is not None:
        graph = coo_matrix((np.ones(len(edges), dtype=np.int8), (edges[:, 0], edges[:, 1])), shape=(n, n))
        return int(connected_components(graph, directed=False)[0])
    label = np.arange(n)
    while True:
        low = np.minimum(label[edges[:, 0]], label[edges[:, 1]])
        before = label.copy()
        np.minimum.at(label, edges[:, 0], low)
        np.minimum.at(label, edges[:, 1], low)
        label = label[label]  # (pointer jumping)
        if np.array_equal(before, label):
            return int(len(np.unique(label)))


def run(agents, args):
    import bench
    from rmf_crowdsim_amd import Simulation, _abi, scenes
    from rmf_crowdsim_amd.simulation import CLUSTER_DTYPE
    sim = bench.build_crowd(Simulation, agents, 2.0, 2.0, scenes.CREEP_SPEED, workload="walk", steps=200)[0]
    lib, eng = sim._lib, sim._engine
    for _ in range(20):
        sim.step(0.05, report=False)
    sim.synchronize()
    slow = _abi.Selection()
    slow.terms = _abi.CS_SEL_SPEED
    slow.speed_lo, slow.speed_hi = 0.0, 0.2
    out = {"agents": len(sim)}
    u64p, pairp, clup = C.POINTER(C.c_uint64), C.POINTER(_abi.IdPair), C.POINTER(_abi.Cluster)
    size_max = C.c_size_t(-1).value

    def ref(sel):
        return C.byref(sel) if sel is not None else None

    def count(distance, sel, min_size=1):
        na, nc = C.c_size_t(0), C.c_size_t(0)
        rc = lib.cs_agent_clusters(eng, distance, ref(sel), min_size, None, None, 0, C.byref(na), None, 0, C.byref(nc))
        assert rc == 0, lib.cs_last_error(eng).decode()
        return na.value, nc.value

    def listing(distance, sel, min_size=1):
        na, nc = count(distance, sel, min_size)
        ids, labels = np.empty(max(na, 1), dtype=np.uint64), np.empty(max(na, 1), dtype=np.uint64)
        table = np.empty(max(nc, 1), dtype=CLUSTER_DTYPE)
        a, c = C.c_size_t(0), C.c_size_t(0)
        rc = lib.cs_agent_clusters(eng, distance, ref(sel), min_size, ids.ctypes.data_as(u64p), labels.ctypes.data_as(u64p), na,
                                   C.byref(a), table.ctypes.data_as(clup), nc, C.byref(c))
        assert rc == 0 and (a.value, c.value) == (na, nc), lib.cs_last_error(eng).decode()
        return ids[:na], labels[:na], table[:nc]

    def parent_path(distance, sel):
        m = lib.cs_close_pairs(eng, distance, ref(sel), ref(sel), None, None, 0)
        assert m != size_max, lib.cs_last_error(eng).decode()
        pairs = np.empty((max(m, 1), 2), dtype=np.uint64)
        got = lib.cs_close_pairs(eng, distance, ref(sel), ref(sel), pairs.ctypes.data_as(pairp), None, m)
        assert got == m, lib.cs_last_error(eng).decode()
        return host_components(pairs[:m])

    for distance in args.distances:
        for who, sel in (("everyone", None), ("speed below 0.2", slow)):
            na, nc = count(distance, sel)
            table = listing(distance, sel)[2]
            row = {"members": int(na), "clusters": int(nc), "clusters_of_2_or_more": int((table["size"] >= 2).sum()),
                   "largest": int(table["size"].max()) if len(table) else 0,
                   "pairs": int(lib.cs_close_pairs(eng, distance, ref(sel), ref(sel), None, None, 0))}
            row["count"] = _timed(lambda: count(distance, sel), args.warmup, args.reps)
            row["list"] = _timed(lambda: listing(distance, sel), args.warmup, args.reps)
            row["jams"] = _timed(lambda: listing(distance, sel, 8), args.warmup, args.reps)
            row["parent_path"] = _timed(lambda: parent_path(distance, sel), args.warmup, args.reps)
            row["parent_path_components"] = parent_path(distance, sel)
            row["parent_over_list"] = row["parent_path"]["median_us"] / row["list"]["median_us"]
            row["parent_over_count"] = row["parent_path"]["median_us"] / row["count"]["median_us"]
            out[f"{distance} m, {who}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[1_000_000, 125_000])
    ap.add_argument("--distances", type=float, nargs="*", default=[0.4, 1.5])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    print(json.dumps({"reps": args.reps, "warmup": args.warmup, "host_merge": HOST_MERGE,
                      "runs": [run(n, args) for n in args.agents]}))


if __name__ == "__main__":
    main()
