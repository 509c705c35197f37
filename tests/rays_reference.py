"""The rule of cs_cast_rays (include/crowdstep_state.h, "Rays against the crowd between steps") restated in numpy, and what
the ray tests share.

`cast` is the definition the engine is compared with, applied to the engine's OWN read_agents(): who takes part by the
rectangle rule of the pairs (close_pairs_reference.takes_part), the rule in f64 with every difference, product, sum, the
square root and the division a separate numpy operation (rounded once each), rays x agents by brute force in blocks of
rays, the answer of a ray the lexicographic minimum of (t, id) in two passes.  It knows nothing of cells, rows or an order
of visits.  Equality with the engine is exact; there is no tolerance."""
import ctypes as C

import numpy as np

from rmf_crowdsim_amd import _abi
from rmf_crowdsim_amd.simulation import RAY_DTYPE, RAY_HIT_DTYPE, rays_array
from close_pairs_reference import SIZE_MAX, last_error, roles, takes_part

BLOCK = 256
NO_HIT = np.uint64(_abi.CS_NO_HIT)
INF = np.float64(np.inf)


def rule(x, y, rays, radius):
    """(hit, t, d2, cr, uu) for every (ray, agent): bool and float64 arrays [len(rays), len(x)], one numpy operation per
    operation of the header's rule (uu: [len(rays), 1])."""
    R2 = np.float64(radius) * np.float64(radius)
    ox, oy = rays["ox"][:, None], rays["oy"][:, None]
    ux, uy = rays["ux"][:, None], rays["uy"][:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        uu = ux * ux + uy * uy
        rx = x[None, :] - ox
        ry = y[None, :] - oy
        d2 = rx * rx + ry * ry
        inside = d2 < R2
        b = rx * ux + ry * uy
        cr = rx * uy - ry * ux
        h2 = R2 * uu - cr * cr
        ahead = (b > 0) & (h2 > 0)
        t = (b - np.sqrt(h2)) / uu
        t = np.where(t < 0, np.float64(0.0), t)
        t = np.where(inside, np.float64(0.0), t)
        hit = (inside | ahead) & (t < rays["t_max"][:, None])
    return hit, t, d2, cr, uu


def cast(records, grid, rays, radius, targets=None, stats=None):
    """-> RAY_HIT_DTYPE[len(rays)]: per ray the lexicographic minimum of (t, id) over its hits, or (CS_NO_HIT, +inf).
    targets: a bool mask over records (None: everyone).  stats (a dict): gets "not_nearest", the number of rays whose
    winner is not the candidate (a participant among the targets that the ray does not ignore) with the smallest d2 to the
    origin, and "cr", "uu" of the winners (NaN for a miss)."""
    rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    part = takes_part(records, grid)
    if targets is not None:
        part = part & np.asarray(targets, dtype=bool)
    ids = records["id"][part].astype(np.uint64)
    x, y = records["x"][part].astype(np.float64), records["y"][part].astype(np.float64)
    out = np.zeros(len(rays), dtype=RAY_HIT_DTYPE)
    out["id"], out["t"] = NO_HIT, INF
    not_nearest, win_cr, win_uu = 0, np.full(len(rays), np.nan), np.full(len(rays), np.nan)
    for lo in range(0, len(rays) if len(ids) else 0, BLOCK):
        block = rays[lo:lo + BLOCK]
        hit, t, d2, cr, uu = rule(x, y, block, radius)
        hit &= ids[None, :] != block["ignore"][:, None]
        t_hit = np.where(hit, t, INF)
        t_min = t_hit.min(axis=1)
        first = hit & (t_hit == t_min[:, None])  # pass two: the smallest id among the hits at the smallest t
        id_min = np.where(first, ids[None, :], NO_HIT).min(axis=1)
        some = hit.any(axis=1)
        out["id"][lo:lo + BLOCK] = np.where(some, id_min, NO_HIT)
        out["t"][lo:lo + BLOCK] = np.where(some, t_min, INF)
        if stats is not None:
            col = np.argmax(first & (ids[None, :] == id_min[:, None]), axis=1)
            with np.errstate(invalid="ignore"):
                nearest = np.argmin(np.where((ids[None, :] != block["ignore"][:, None]) & (d2 == d2), d2, INF), axis=1)
            not_nearest += int((some & (col != nearest)).sum())
            k = np.arange(len(block))
            win_cr[lo:lo + BLOCK] = np.where(some, cr[k, col], np.nan)
            win_uu[lo:lo + BLOCK] = np.where(some, uu[k, 0], np.nan)
    if stats is not None:
        stats["not_nearest"], stats["cr"], stats["uu"] = not_nearest, win_cr, win_uu
    return out


def classes(rows):
    """(hits with t > 0, hits with t == 0, misses)"""
    hit = rows["id"] != NO_HIT
    return int((hit & (rows["t"] > 0.0)).sum()), int((hit & (rows["t"] == 0.0)).sum()), int((~hit).sum())


def call(sim, rays, radius, sel=None, rows=True, fill=0xAB, n=None):
    """cs_cast_rays / cs_mesh_cast_rays on a Simulation or a NativeTileMesh by the C entry point -> (the returned count,
    RAY_HIT_DTYPE[len(rays)] filled with `fill` before the call, or None with rows=False: the null array).  n: the number
    of rays passed, where it is not len(rays)."""
    mesh = not hasattr(sim, "_engine")
    fn = sim._lib.cs_mesh_cast_rays if mesh else sim._lib.cs_cast_rays
    handle = sim._mesh if mesh else sim._engine
    rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    out = None
    if rows:
        out = np.zeros(max(len(rays), 1), dtype=RAY_HIT_DTYPE)
        out.view(np.uint8)[...] = fill
    got = fn(handle, rays.ctypes.data_as(C.POINTER(_abi.Ray)), len(rays) if n is None else n, float(radius),
             C.byref(sel) if sel is not None else None, out.ctypes.data_as(C.POINTER(_abi.RayHit)) if rows else None)
    return got, out


def agree(sim, records, grid, rays, radius, sel=None, cols=(None, None, None), name="", stats=None, want=None):
    """The engine's (or mesh's) rows equal the restatement on `records` byte for byte, the returned count is the number
    of rays that hit, with rows and without.  Returns the restatement's rows.  want: the restatement's rows for these very
    arguments, where a test has them already (a mesh after the single engine)."""
    if want is None:
        mask = None if sel is None else roles(sel, None, records, *cols)[0]
        want = cast(records, grid, rays, radius, mask, stats=stats)
    hits = int((want["id"] != NO_HIT).sum())
    n, got = call(sim, rays, radius, sel)
    print(f"  {name}: {len(rays)} rays, restatement {classes(want)} (t > 0, t == 0, miss), engine {n} hits")
    assert n == hits, (name, last_error(sim) if n == SIZE_MAX else n)
    bad = np.nonzero((got["id"][:len(want)] != want["id"]) | (got["t"][:len(want)].view(np.uint64) != want["t"].view(np.uint64)))[0]
    assert len(bad) == 0, (name, len(bad), [(int(k), got[k].tolist(), want[k].tolist(), rays[k].tolist()) for k in bad[:4]])
    assert got[:len(want)].tobytes() == want.tobytes(), name
    n, none = call(sim, rays, radius, sel, rows=False)
    assert n == hits and none is None, name
    return want


__all__ = ["RAY_DTYPE", "RAY_HIT_DTYPE", "rays_array", "rule", "cast", "classes", "call", "agree", "NO_HIT", "SIZE_MAX",
           "last_error"]
