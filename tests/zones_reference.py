"""The rule of cs_zone_agents (include/crowdstep_state.h, "Agents in polygon zones") restated in numpy, and what the zone
tests share.

`in_ring` is the ring test: f64, one numpy operation per operation of the header (rounded once each), every edge against
every point, no shortcut but the box, which is part of the rule.  `zone_agents` is the definition the engine is compared
with, applied to the engine's OWN read_agents(): who takes part by the rectangle rule of the pairs
(close_pairs_reference.takes_part), zones x agents by brute force, the rows in (zone, id) order.  It knows nothing of
cells, rows of cells, items or an order of visits.  Equality with the engine is exact; there is no tolerance."""
import ctypes as C

import numpy as np

from rmf_crowdsim_amd import _abi
from rmf_crowdsim_amd.simulation import ZONE_AGENT_DTYPE, ZONE_DTYPE, zones_array
from close_pairs_reference import SIZE_MAX, last_error, roles, takes_part


def box(ring):
    """(bx0, bx1, by0, by1): the exact minimum and maximum of the vertices' coordinates"""
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    return ring[:, 0].min(), ring[:, 0].max(), ring[:, 1].min(), ring[:, 1].max()


def crossings(x, y, ring):
    """The number of crossing edges of `ring` (k, 2) for every point (x[i], y[i])"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    k = len(ring)
    n = np.zeros(x.shape, dtype=np.int64)
    for i in range(k):
        ax, ay = ring[i]
        bx, by = ring[(i + 1) % k]
        if ay <= by:
            lx, ly, hx, hy = ax, ay, bx, by
        else:
            lx, ly, hx, hy = bx, by, ax, ay
        if ly == hy:
            continue  # a horizontal edge never straddles
        with np.errstate(invalid="ignore", over="ignore"):
            straddles = (ly <= y) & (y < hy)
            ex = hx - lx
            ey = hy - ly
            px = x - lx
            py = y - ly
            t1 = ex * py
            t2 = ey * px
            c = t1 - t2
            n += straddles & (c > 0.0)
    return n


def in_ring(x, y, ring):
    """Bool per point: inside the box of `ring` and an odd number of crossing edges"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    bx0, bx1, by0, by1 = box(ring)
    with np.errstate(invalid="ignore"):
        boxed = (bx0 <= x) & (x <= bx1) & (by0 <= y) & (y <= by1)
    return boxed & (crossings(x, y, ring) % 2 == 1)


def rect_ring(x0, y0, x1, y1, reverse=False):
    ring = np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], dtype=np.float64)
    return ring[::-1].copy() if reverse else ring


def in_rect(x, y, x0, y0, x1, y1):
    """the CS_SEL_RECT expression"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return (x0 <= x) & (x < x1) & (y0 <= y) & (y < y1)


def zone_agents(records, grid, zones, vertices, mask=None):
    """-> (ZONE_AGENT_DTYPE rows ascending by (zone, id), uint64 counts per zone).  mask: a bool mask over records, the
    filter (None: everyone)."""
    zones = np.ascontiguousarray(zones, dtype=ZONE_DTYPE)
    vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    part = takes_part(records, grid)
    if mask is not None:
        part = part & np.asarray(mask, dtype=bool)
    ids = records["id"][part].astype(np.uint64)
    order = np.argsort(ids, kind="stable")
    ids = ids[order]
    x, y = records["x"][part].astype(np.float64)[order], records["y"][part].astype(np.float64)[order]
    counts = np.zeros(len(zones), dtype=np.uint64)
    out = []
    for k, z in enumerate(zones):
        ring = vertices[int(z["first"]):int(z["first"]) + int(z["count"])]
        inside = in_ring(x, y, ring) if len(ids) else np.zeros(0, dtype=bool)
        rows = np.zeros(int(inside.sum()), dtype=ZONE_AGENT_DTYPE)
        rows["zone"], rows["id"] = k, ids[inside]
        out.append(rows)
        counts[k] = len(rows)
    rows = np.concatenate(out) if out else np.zeros(0, dtype=ZONE_AGENT_DTYPE)
    return rows, counts


def call(sim, zones, vertices, sel=None, cap=0, rows=True, counts=True, fill=0xAB, n=None, n_vertices=None,
         null_zones=False, null_vertices=False):
    """cs_zone_agents / cs_mesh_zone_agents on a Simulation or a NativeTileMesh by the C entry point -> (the returned
    count, the uint64 counts buffer or None, the ZONE_AGENT_DTYPE buffer of cap + 2 rows or None), both buffers filled
    with `fill` before the call.  rows=False passes the null array with `cap` as given; n, n_vertices: the numbers passed,
    where they are not the lengths of the arrays."""
    mesh = not hasattr(sim, "_engine")
    fn = sim._lib.cs_mesh_zone_agents if mesh else sim._lib.cs_zone_agents
    handle = sim._mesh if mesh else sim._engine
    zones = np.ascontiguousarray(zones, dtype=ZONE_DTYPE)
    vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 2)
    out = per_zone = None
    if rows:
        out = np.zeros(cap + 2, dtype=ZONE_AGENT_DTYPE)
        out.view(np.uint8)[...] = fill
    if counts:
        per_zone = np.zeros(max(len(zones), 1), dtype=np.uint64)
        per_zone.view(np.uint8)[...] = fill
    got = fn(handle, None if null_zones else zones.ctypes.data_as(C.POINTER(_abi.Zone)), len(zones) if n is None else n,
             None if null_vertices else vertices.ctypes.data_as(C.POINTER(C.c_double)),
             len(vertices) if n_vertices is None else n_vertices, C.byref(sel) if sel is not None else None,
             per_zone.ctypes.data_as(C.POINTER(C.c_uint64)) if counts else None,
             out.ctypes.data_as(C.POINTER(_abi.ZoneAgent)) if rows else None, cap)
    return got, per_zone, out


def agree(sim, records, grid, zones, vertices, sel=None, cols=(None, None, None), name="", want=None):
    """The engine's (or mesh's) rows and per-zone counts equal the restatement on `records` byte for byte: listing with
    room for every row (nothing is written behind them), and counting only (a null array; an array with cap == 0, left
    alone; with and without the counts).  Returns the restatement's (rows, counts).  want: the restatement's answer for
    these very arguments, where a test has it already."""
    if want is None:
        mask = None if sel is None else roles(sel, None, records, *cols)[0]
        want = zone_agents(records, grid, zones, vertices, mask)
    rows, counts = want
    total = len(rows)
    assert int(counts.sum()) == total
    n, per_zone, got = call(sim, zones, vertices, sel, cap=total)
    print(f"  {name}: {len(zones)} zones, restatement {total} rows, engine {n}")
    assert n == total, (name, last_error(sim) if n == SIZE_MAX else n)
    bad = np.nonzero(per_zone[:len(zones)] != counts)[0]
    assert len(bad) == 0, (name, "counts", [(int(k), int(per_zone[k]), int(counts[k])) for k in bad[:6]])
    bad = np.nonzero((got[:total]["zone"] != rows["zone"]) | (got[:total]["id"] != rows["id"]))[0]
    assert len(bad) == 0, (name, len(bad), [(got[k].tolist(), rows[k].tolist()) for k in bad[:4]])
    assert got[:total].tobytes() == rows.tobytes() and (got[total:].view(np.uint8) == 0xAB).all(), name
    n, per_zone, none = call(sim, zones, vertices, sel, cap=total + 5, rows=False)
    assert n == total and none is None and per_zone[:len(zones)].tobytes() == counts.tobytes(), name
    n, per_zone, kept = call(sim, zones, vertices, sel, cap=0, counts=False)
    assert n == total and per_zone is None and (kept.view(np.uint8) == 0xAB).all(), name
    return want


__all__ = ["ZONE_DTYPE", "ZONE_AGENT_DTYPE", "zones_array", "box", "crossings", "in_ring", "rect_ring", "in_rect",
           "zone_agents", "call", "agree", "SIZE_MAX", "last_error"]
