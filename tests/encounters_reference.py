"""The rule of cs_encounters (include/crowdstep_state.h, "Encounters between steps") restated in numpy, and what the
encounter tests share.

`encounters` is the definition the engine is compared with, applied to the engine's OWN read_agents(): who takes part by
the rectangle rule of the pairs (close_pairs_reference.takes_part), the velocities cast through float32 and widened, the
rule in f64 with every difference, product, sum and the division a separate numpy operation (rounded once each), the
roles through close_pairs_reference.roles, the rows sorted by (a, b).  It is brute force over all participants, O(n^2) in
blocks of rows, and knows nothing of cells.  Equality with the engine is exact; there is no tolerance."""
import ctypes as C

import numpy as np

from rmf_crowdsim_amd import _abi
from rmf_crowdsim_amd.simulation import ENCOUNTER_DTYPE
from close_pairs_reference import SIZE_MAX, last_error, roles, takes_part

BLOCK = 512


def products(rx, ry, wx, wy):
    """(d2, ww, rw): the sums of products of the rule that no parameter enters."""
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = rx * rx + ry * ry
        ww = wx * wx + wy * wy
        rw = rx * wx + ry * wy
    return d2, ww, rw


def approach(rx, ry, wx, wy, ww, rw, horizon):
    """(t, m2) of the rule: the time of closest approach within the horizon and the squared distance then."""
    horizon = np.float64(horizon)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        approaching = rw < 0
        free = (-rw) / ww
        free = np.where(free < horizon, free, horizon)
        t = np.where(approaching, free, np.float64(0.0))
        cx = rx + wx * t
        cy = ry + wy * t
        m2 = cx * cx + cy * cy
    return t, m2


def rule(rx, ry, wx, wy, horizon):
    """(d2, t, m2) of the header's rule for r = q - p and w = v_q - v_p (float64 arrays), one numpy operation each."""
    d2, ww, rw = products(rx, ry, wx, wy)
    t, m2 = approach(rx, ry, wx, wy, ww, rw, horizon)
    return d2, t, m2


def encounters(records, grid, distance, horizon, range_, role_a=None, role_b=None, count_only=False, stats=None,
               cache=None):
    """-> the rows (ENCOUNTER_DTYPE: a < b, t, d2 = m2), ascending by (a, b), or with count_only their number alone.
    role_a / role_b: bool masks over records (None: everyone).  stats (a dict): gets "in_range", the number of pairs with
    d2 < range^2 whose roles allow them.  cache: a dict a test keeps for ONE `records` array, so that what no parameter
    enters (the differences and the sums of products, per block of rows) is computed once and shared among its queries."""
    part = takes_part(records, grid)
    a_all = np.ones(len(records), dtype=bool) if role_a is None else np.asarray(role_a, dtype=bool)
    b_all = np.ones(len(records), dtype=bool) if role_b is None else np.asarray(role_b, dtype=bool)
    order = np.argsort(records["id"][part], kind="stable")
    ids = records["id"][part][order].astype(np.uint64)
    x, y = records["x"][part][order].astype(np.float64), records["y"][part][order].astype(np.float64)
    vx = records["vx"][part][order].astype(np.float32).astype(np.float64)
    vy = records["vy"][part][order].astype(np.float32).astype(np.float64)
    ra, rb = a_all[part][order], b_all[part][order]
    range2 = np.float64(range_) * np.float64(range_)
    lim2 = np.float64(distance) * np.float64(distance)
    n, total, in_range, out = len(ids), 0, 0, []
    for lo in range(0, n, BLOCK):
        hi = min(lo + BLOCK, n)
        kept = None if cache is None else cache.get(lo)
        if kept is None:
            with np.errstate(invalid="ignore", over="ignore"):
                rx = x[None, :] - x[lo:hi, None]  # p: the row (the smaller id where it counts), q: the column
                ry = y[None, :] - y[lo:hi, None]
                wx = vx[None, :] - vx[lo:hi, None]
                wy = vy[None, :] - vy[lo:hi, None]
            kept = (rx, ry, wx, wy) + products(rx, ry, wx, wy)
            if cache is not None:
                cache[lo] = kept
        rx, ry, wx, wy, d2, ww, rw = kept
        with np.errstate(invalid="ignore"):
            near = d2 < range2
        near &= np.arange(lo, hi)[:, None] < np.arange(n)[None, :]  # every unordered pair once, the smaller id first
        near &= (ra[lo:hi, None] & rb[None, :]) | (ra[None, :] & rb[lo:hi, None])
        p, q = np.nonzero(near)  # (row-major: ascending p, then ascending q); the rest of the rule on these pairs only
        in_range += len(p)
        t, m2 = approach(rx[p, q], ry[p, q], wx[p, q], wy[p, q], ww[p, q], rw[p, q], horizon)
        with np.errstate(invalid="ignore"):
            hit = m2 < lim2
        if count_only:
            total += int(hit.sum())
            continue
        rows = np.zeros(int(hit.sum()), dtype=ENCOUNTER_DTYPE)
        rows["a"], rows["b"], rows["t"], rows["d2"] = ids[lo + p[hit]], ids[q[hit]], t[hit], m2[hit]
        out.append(rows)
    if stats is not None:
        stats["in_range"] = in_range
    if count_only:
        return total
    return np.concatenate(out) if out else np.zeros(0, dtype=ENCOUNTER_DTYPE)


def call(sim, distance, horizon, range_, sel_a=None, sel_b=None, cap=None, fill=None):
    """cs_encounters / cs_mesh_encounters on a Simulation or a NativeTileMesh by the C entry point -> (the returned count,
    ENCOUNTER_DTYPE[cap] rows): the whole array given, so a test sees what was written.  cap None: the count-only form (a
    null array)."""
    mesh = not hasattr(sim, "_engine")
    fn = sim._lib.cs_mesh_encounters if mesh else sim._lib.cs_encounters
    handle = sim._mesh if mesh else sim._engine
    a = C.byref(sel_a) if sel_a is not None else None
    b = C.byref(sel_b) if sel_b is not None else None
    if cap is None:
        return fn(handle, float(distance), float(horizon), float(range_), a, b, None, 0), None
    out = np.zeros(max(cap, 1), dtype=ENCOUNTER_DTYPE)
    if fill is not None:
        out.view(np.uint8)[...] = fill
    n = fn(handle, float(distance), float(horizon), float(range_), a, b, out.ctypes.data_as(C.POINTER(_abi.Encounter)), cap)
    return n, out


def agree(sim, records, grid, distance, horizon, range_, sel_a=None, sel_b=None, cols=(None, None, None), name="",
          capped=True, stats=None, cache=None, want=None):
    """The engine's (or mesh's) count, rows, order and the bits of t and d2 equal the restatement on `records`, in the
    listing form (nothing written beyond the rows), the count-only form and (capped) under a cap of half the count.
    Returns the restatement's rows.  cache: see encounters().  want: the restatement's rows for these very arguments, where
    a test has them already (a mesh after the single engine)."""
    if want is None:
        ra, rb = roles(sel_a, sel_b, records, *cols)
        want = encounters(records, grid, distance, horizon, range_, None if sel_a is None else ra,
                          None if sel_b is None else rb, stats=stats, cache=cache)
    n, _ = call(sim, distance, horizon, range_, sel_a, sel_b)
    print(f"  {name}: restatement {len(want)} encounters, engine {n}")
    assert n == len(want), (name, last_error(sim) if n == SIZE_MAX else n)
    n, got = call(sim, distance, horizon, range_, sel_a, sel_b, cap=len(want) + 3, fill=0xAB)
    assert n == len(want), name
    assert np.array_equal(got["a"][:n], want["a"]) and np.array_equal(got["b"][:n], want["b"]), name
    assert got[:n].tobytes() == want.tobytes(), name  # t and d2 to the bit
    assert (got[n:].view(np.uint8) == 0xAB).all(), name  # nothing beyond
    if capped and len(want) > 1:
        cap = len(want) // 2
        n, few = call(sim, distance, horizon, range_, sel_a, sel_b, cap=cap, fill=0xAB)
        assert n == len(want) and few.tobytes() == want[:cap].tobytes(), name
    return want
