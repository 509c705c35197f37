"""The rules of cs_agent_clusters (include/crowdstep_state.h, "Clusters of agents between steps") restated in numpy and
plain Python, and what the cluster tests share.

`clusters` is the definition the engine is compared with, applied to the engine's OWN read_agents(): the members by the
rectangle rule (close_pairs_reference.takes_part) and select_reference.pred, the links from close_pairs_reference.pairs with
both roles set to the member mask (brute force, f64, every operation rounded once), the components from a plain union-find
over ids, the label the smallest id, the table by per-cluster loops.  It knows nothing of cells, slots, tiles or the
device.  Ids, labels, order, sizes and boxes are compared exactly; the sums under the bound the header states."""
import ctypes as C
import math

import numpy as np

from rmf_crowdsim_amd import _abi
from rmf_crowdsim_amd.simulation import CLUSTER_DTYPE
from close_pairs_reference import last_error, pairs, roles, takes_part

EPS = 2.0 ** -52


def components(ids, links):
    """{id: smallest id of its component} for the graph (ids, links); a plain union-find with path halving"""
    parent = {int(i): int(i) for i in ids}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for p, q in np.asarray(links, dtype=np.uint64).reshape(-1, 2).tolist():
        a, b = find(p), find(q)
        if a != b:
            parent[max(a, b)] = min(a, b)  # (the smaller id stays the root: the root IS the label)
    return {i: find(i) for i in parent}


def clusters(records, grid, distance, member_mask=None, min_size=1, cache=None):
    """-> (uint64 ids of the members of reported clusters, ascending; uint64 label of each; the table of the reported
    clusters, ascending by label, with sum_x / sum_y the exactly rounded sums; {label: sum|x|, sum|y|} for the bound)"""
    mask = np.ones(len(records), dtype=bool) if member_mask is None else np.asarray(member_mask, dtype=bool)
    member = takes_part(records, grid) & mask
    links, _ = pairs(records, grid, distance, mask, mask, cache=cache)
    ids = records["id"][member].astype(np.uint64)
    label_of = components(ids.tolist(), links)
    by_label = {}
    for k in np.nonzero(member)[0]:
        by_label.setdefault(label_of[int(records["id"][k])], []).append(k)
    table, absum = [], {}
    for label in sorted(by_label):
        rows = by_label[label]
        if len(rows) < max(int(min_size), 1):
            continue
        x, y = records["x"][rows].astype(np.float64), records["y"][rows].astype(np.float64)
        table.append((label, len(rows), x.min(), y.min(), x.max(), y.max(), math.fsum(x.tolist()), math.fsum(y.tolist())))
        absum[label] = (math.fsum(np.abs(x).tolist()), math.fsum(np.abs(y).tolist()))
    table = np.array(table, dtype=CLUSTER_DTYPE) if table else np.zeros(0, dtype=CLUSTER_DTYPE)
    reported = set(int(v) for v in table["label"])
    out = sorted((int(i), label_of[int(i)]) for i in ids.tolist() if label_of[int(i)] in reported)
    out_ids = np.array([p for p, _ in out], dtype=np.uint64)
    out_labels = np.array([q for _, q in out], dtype=np.uint64)
    return out_ids, out_labels, table, absum


def agent_clusters(sim, distance, sel=None, min_size=1, agent_cap=None, cluster_cap=None, fill=None, labels=True,
                   counts=True):
    """cs_agent_clusters / cs_mesh_agent_clusters on a Simulation or a NativeTileMesh by the C entry point -> (rc, n_agents,
    n_clusters, ids, labels, table): the whole arrays given, each with two entries of room beyond its cap, so a test sees
    what was written.  A cap of None: that output is NULL."""
    mesh = not hasattr(sim, "_engine")
    fn = sim._lib.cs_mesh_agent_clusters if mesh else sim._lib.cs_agent_clusters
    handle = sim._mesh if mesh else sim._engine
    ids = lab = table = None
    if agent_cap is not None:
        ids = np.zeros(agent_cap + 2, dtype=np.uint64)
        lab = np.zeros(agent_cap + 2, dtype=np.uint64)
    if cluster_cap is not None:
        table = np.zeros(cluster_cap + 2, dtype=CLUSTER_DTYPE)
    if fill is not None:
        for arr in (ids, lab, table):
            if arr is not None:
                arr.view(np.uint8)[...] = fill
    na, nc = C.c_size_t(2 ** 62), C.c_size_t(2 ** 62)
    u64 = C.POINTER(C.c_uint64)
    rc = fn(handle, float(distance), C.byref(sel) if sel is not None else None, int(min_size),
            ids.ctypes.data_as(u64) if ids is not None else None,
            lab.ctypes.data_as(u64) if (lab is not None and labels) else None, agent_cap or 0,
            C.byref(na) if counts else None,
            table.ctypes.data_as(C.POINTER(_abi.Cluster)) if table is not None else None, cluster_cap or 0,
            C.byref(nc) if counts else None)
    return rc, na.value, nc.value, ids, lab, table


def same_table(got, want, absum, name=""):
    """label, size and box exactly; the sums within size * 2^-52 * sum|x| of the exactly rounded sum"""
    assert len(got) == len(want), name
    for f in ("label", "size", "min_x", "min_y", "max_x", "max_y"):
        assert got[f].tobytes() == want[f].tobytes(), (name, f)
    for g, w in zip(got, want):
        ax, ay = absum[int(w["label"])]
        n = float(w["size"])
        assert abs(float(g["sum_x"]) - float(w["sum_x"])) <= n * EPS * ax, (name, "sum_x", g, w)
        assert abs(float(g["sum_y"]) - float(w["sum_y"])) <= n * EPS * ay, (name, "sum_y", g, w)
        if w["size"] == 1:
            assert g["sum_x"] == g["min_x"] == g["max_x"] and g["sum_y"] == g["min_y"] == g["max_y"], (name, g)


def agree(sim, records, grid, distance, members=None, min_size=1, cols=(None, None, None), name="", cache=None):
    """The engine's (or mesh's) clusters equal the restatement on `records`: both counts, ids, labels, label order, sizes
    and boxes exactly, the sums under the bound; the capped forms write the first `cap` entries and leave the fill bytes
    beyond; the count-only form gives the same counts.  Returns the restatement's (ids, labels, table).  cache: a dict a
    test keeps for ONE `records` array (close_pairs_reference.pairs)."""
    mask, _ = roles(members, None, records, *cols)
    ids, labels, table, absum = clusters(records, grid, distance, None if members is None else mask, min_size, cache)
    rc, na, nc, _, _, _ = agent_clusters(sim, distance, members, min_size)  # the count-only form
    print(f"  {name}: restatement {len(table)} clusters of {len(ids)} members, engine {nc} of {na}")
    assert rc == 0, (name, last_error(sim))
    assert (na, nc) == (len(ids), len(table)), name
    rc, na, nc, g_ids, g_lab, g_tab = agent_clusters(sim, distance, members, min_size, len(ids) + 3, len(table) + 3, fill=0xAB)
    assert rc == 0 and (na, nc) == (len(ids), len(table)), name
    assert np.array_equal(g_ids[:na], ids) and np.array_equal(g_lab[:na], labels), name
    same_table(g_tab[:nc], table, absum, name)
    for arr, n in ((g_ids, na), (g_lab, na), (g_tab, nc)):  # nothing beyond
        assert (arr[n:].view(np.uint8) == 0xAB).all(), name
    if len(ids) > 1:
        ca, cc = len(ids) // 2, len(table) // 2
        rc, na, nc, g_ids, g_lab, g_tab = agent_clusters(sim, distance, members, min_size, ca, cc, fill=0xAB)
        assert rc == 0 and (na, nc) == (len(ids), len(table)), name
        assert np.array_equal(g_ids[:ca], ids[:ca]) and np.array_equal(g_lab[:ca], labels[:ca]), name
        same_table(g_tab[:cc], table[:cc], absum, name)
        for arr, n in ((g_ids, ca), (g_lab, ca), (g_tab, cc)):
            assert (arr[n:].view(np.uint8) == 0xAB).all(), name
    return ids, labels, table
