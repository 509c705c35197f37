"""The rule of cs_leg_conflicts (include/crowdstep_state.h, "Paths against the moving crowd between steps") restated in
numpy, and what the leg tests share.

`conflicts` is the definition the engine is compared with, applied to the engine's OWN read_agents(): who takes part by
the rectangle rule of the pairs (close_pairs_reference.takes_part), the rule in f64 with every difference, product, sum,
the square root and the division a separate numpy operation (rounded once each), legs x agents by brute force in blocks of
legs, the answer of a leg the lexicographic minimum of (s, id) in two passes.  It knows nothing of cells, rows, reaches or
an order of visits.  Equality with the engine is exact, on the id and on the bits of s; there is no tolerance."""
import ctypes as C

import numpy as np

from rmf_crowdsim_amd import _abi
from rmf_crowdsim_amd.simulation import LEG_DTYPE, LEG_HIT_DTYPE, legs_array
from close_pairs_reference import SIZE_MAX, last_error, roles, takes_part

BLOCK = 256  # legs of one block, at most
NO_HIT = np.uint64(_abi.CS_NO_HIT)
INF = np.float64(np.inf)


def block_of(n_agents):
    """The legs taken at a time: the [legs, agents] temporaries of a block stay near 64K numbers each, in cache (the answer
    does not depend on it: every operation is per (leg, agent), every reduction per leg)."""
    return max(1, min(BLOCK, 65536 // max(n_agents, 1)))


def rule(x, y, vx, vy, legs, distance, speed_max):
    """(conflict, s, d2) for every (leg, agent): bool and float64 arrays [len(legs), len(x)], one numpy operation per
    operation of the header's rule.  x, y, vx, vy: float64 (the velocity the f32 of the record, widened)."""
    D2 = np.float64(distance) * np.float64(distance)
    S2 = np.float64(speed_max) * np.float64(speed_max)
    x0, y0 = legs["x0"][:, None], legs["y0"][:, None]
    lvx, lvy = legs["vx"][:, None], legs["vy"][:, None]
    t0 = legs["t0"][:, None]
    T = (legs["t1"] - legs["t0"])[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ss = vx * vx + vy * vy
        slow = (ss < S2)[None, :]
        px = x[None, :] + vx[None, :] * t0
        py = y[None, :] + vy[None, :] * t0
        rx = px - x0
        ry = py - y0
        wx = vx[None, :] - lvx
        wy = vy[None, :] - lvy
        d2 = rx * rx + ry * ry
        inside = d2 < D2
        a = rx * wx + ry * wy
        ww = wx * wx + wy * wy
        cr = rx * wy - ry * wx
        h2 = D2 * ww - cr * cr
        closing = (a < 0) & (h2 > 0)
        s = (-a - np.sqrt(h2)) / ww
        s = np.where(s < 0, np.float64(0.0), s)
        s = np.where(inside, np.float64(0.0), s)
        hit = slow & (inside | closing) & (s < T)
    return hit, s, d2


def conflicts(records, grid, legs, distance, speed_max, targets=None, stats=None):
    """-> LEG_HIT_DTYPE[len(legs)]: per leg the lexicographic minimum of (s, id) over its conflicts, or (CS_NO_HIT, +inf).
    targets: a bool mask over records (None: everyone).  stats (a dict): gets "not_nearest", the number of legs whose
    winner is not the candidate (a participant among the targets that the leg does not ignore) standing nearest the
    leg's start now."""
    legs = np.ascontiguousarray(legs, dtype=LEG_DTYPE)
    part = takes_part(records, grid)
    if targets is not None:
        part = part & np.asarray(targets, dtype=bool)
    ids = records["id"][part].astype(np.uint64)
    x, y = records["x"][part].astype(np.float64), records["y"][part].astype(np.float64)
    vx, vy = records["vx"][part].astype(np.float32).astype(np.float64), records["vy"][part].astype(np.float32).astype(np.float64)
    out = np.zeros(len(legs), dtype=LEG_HIT_DTYPE)
    out["id"], out["s"] = NO_HIT, INF
    not_nearest = 0
    BLOCK = block_of(len(ids))
    for lo in range(0, len(legs) if len(ids) else 0, BLOCK):
        block = legs[lo:lo + BLOCK]
        hit, s, _ = rule(x, y, vx, vy, block, distance, speed_max)
        others = ids[None, :] != block["ignore"][:, None]
        hit &= others
        s_hit = np.where(hit, s, INF)
        s_min = s_hit.min(axis=1)
        first = hit & (s_hit == s_min[:, None])  # pass two: the smallest id among the conflicts at the smallest s
        id_min = np.where(first, ids[None, :], NO_HIT).min(axis=1)
        some = hit.any(axis=1)
        out["id"][lo:lo + BLOCK] = np.where(some, id_min, NO_HIT)
        out["s"][lo:lo + BLOCK] = np.where(some, s_min, INF)
        if stats is not None:
            col = np.argmax(first & (ids[None, :] == id_min[:, None]), axis=1)
            dx, dy = x[None, :] - block["x0"][:, None], y[None, :] - block["y0"][:, None]
            nearest = np.argmin(np.where(others, dx * dx + dy * dy, INF), axis=1)
            not_nearest += int((some & (col != nearest)).sum())
    if stats is not None:
        stats["not_nearest"] = not_nearest
    return out


def classes(rows):
    """(conflicts with s > 0, conflicts with s == 0, misses)"""
    hit = rows["id"] != NO_HIT
    return int((hit & (rows["s"] > 0.0)).sum()), int((hit & (rows["s"] == 0.0)).sum()), int((~hit).sum())


def call(sim, legs, distance, speed_max, sel=None, rows=True, fill=0xAB, n=None):
    """cs_leg_conflicts / cs_mesh_leg_conflicts on a Simulation or a NativeTileMesh by the C entry point -> (the returned
    count, LEG_HIT_DTYPE[len(legs)] filled with `fill` before the call, or None with rows=False: the null array).  n: the
    number of legs passed, where it is not len(legs)."""
    mesh = not hasattr(sim, "_engine")
    fn = sim._lib.cs_mesh_leg_conflicts if mesh else sim._lib.cs_leg_conflicts
    handle = sim._mesh if mesh else sim._engine
    legs = np.ascontiguousarray(legs, dtype=LEG_DTYPE)
    out = None
    if rows:
        out = np.zeros(max(len(legs), 1), dtype=LEG_HIT_DTYPE)
        out.view(np.uint8)[...] = fill
    got = fn(handle, legs.ctypes.data_as(C.POINTER(_abi.Leg)), len(legs) if n is None else n, float(distance),
             float(speed_max), C.byref(sel) if sel is not None else None,
             out.ctypes.data_as(C.POINTER(_abi.LegHit)) if rows else None)
    return got, out


def agree(sim, records, grid, legs, distance, speed_max, sel=None, cols=(None, None, None), name="", stats=None, want=None):
    """The engine's (or mesh's) rows equal the restatement on `records` byte for byte, the returned count is the number
    of legs with a conflict, with rows and without.  Returns the restatement's rows.  want: the restatement's rows for
    these very arguments, where a test has them already (a mesh after the single engine)."""
    if want is None:
        mask = None if sel is None else roles(sel, None, records, *cols)[0]
        want = conflicts(records, grid, legs, distance, speed_max, mask, stats=stats)
    hits = int((want["id"] != NO_HIT).sum())
    n, got = call(sim, legs, distance, speed_max, sel)
    print(f"  {name}: {len(legs)} legs, restatement {classes(want)} (s > 0, s == 0, miss), engine {n} conflicts")
    assert n == hits, (name, last_error(sim) if n == SIZE_MAX else n)
    bad = np.nonzero((got["id"][:len(want)] != want["id"]) | (got["s"][:len(want)].view(np.uint64) != want["s"].view(np.uint64)))[0]
    assert len(bad) == 0, (name, len(bad), [(int(k), got[k].tolist(), want[k].tolist(), legs[k].tolist()) for k in bad[:4]])
    assert got[:len(want)].tobytes() == want.tobytes(), name
    n, none = call(sim, legs, distance, speed_max, sel, rows=False)
    assert n == hits and none is None, name
    return want


__all__ = ["LEG_DTYPE", "LEG_HIT_DTYPE", "legs_array", "rule", "conflicts", "classes", "call", "agree", "NO_HIT",
           "SIZE_MAX", "last_error"]
