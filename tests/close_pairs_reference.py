"""The rules of cs_close_pairs (include/crowdstep_state.h, "Pairs of agents between steps") restated in numpy, and what the
pair tests share.

`pairs` is the definition the engine is compared with, applied to the engine's OWN read_agents(): who takes part by the
rectangle rule, the predicate in f64 with every difference, product and sum a separate numpy operation (rounded once each),
the roles through select_reference.pred, the pairs sorted by (a, b), and d2.  It is brute force over all participants,
O(n^2) in blocks of rows, and knows nothing of cells.  Equality with the engine is exact; there is no tolerance."""
import ctypes as C

import numpy as np

from rmf_crowdsim_amd import _abi
from select_reference import pred

SIZE_MAX = C.c_size_t(-1).value
BLOCK = 512


def rectangle(grid):
    """(gx0, gx1, gy0, gy1) of a grid description (the keywords of LocationHash2D): the f64 values read_agents() would
    report for the low corner of cell (0, 0) and of the cell one beyond the last row and column.  x runs over
    (size_t)(height / cell_size) rows, y over (size_t)(width / cell_size) columns (the row stride)."""
    cell = np.float64(grid["cell_size"])
    off_x, off_y = (np.float64(v) for v in grid["offset"])
    rows, stride = int(np.float64(grid["height"]) / cell), int(np.float64(grid["width"]) / cell)
    zero = np.float64(0.0)
    return (off_x + (zero * cell + zero), off_x + (np.float64(rows) * cell + zero),
            off_y + (zero * cell + zero), off_y + (np.float64(stride) * cell + zero))


def takes_part(records, grid):
    """Bool mask: the records whose position is finite and inside the grid's own rectangle."""
    gx0, gx1, gy0, gy1 = rectangle(grid)
    x, y = records["x"].astype(np.float64), records["y"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (gx0 <= x) & (x < gx1) & (gy0 <= y) & (y < gy1)


def roles(sel_a, sel_b, records, owner=None, hlp=None, lp=None):
    """(A, B) bool masks over records; a selection that is None: everyone."""
    none = np.zeros(len(records))
    cols = (none if owner is None else owner, none if hlp is None else hlp, none if lp is None else lp)
    everyone = np.ones(len(records), dtype=bool)
    return (everyone if sel_a is None else pred(sel_a, records, *cols),
            everyone if sel_b is None else pred(sel_b, records, *cols))


def pairs(records, grid, distance, role_a=None, role_b=None, count_only=False, cache=None):
    """-> (uint64[n, 2] pairs (a, b) with a < b, ascending; float64[n] d2), or with count_only the number n alone.
    role_a / role_b: bool masks over records (None: everyone).  cache: a dict a test keeps for ONE `records` array, so
    that the left-hand sides are computed once and shared among its distances (it holds the blocks of d2)."""
    part = takes_part(records, grid)
    a_all = np.ones(len(records), dtype=bool) if role_a is None else np.asarray(role_a, dtype=bool)
    b_all = np.ones(len(records), dtype=bool) if role_b is None else np.asarray(role_b, dtype=bool)
    order = np.argsort(records["id"][part], kind="stable")
    ids = records["id"][part][order].astype(np.uint64)
    x, y = records["x"][part][order].astype(np.float64), records["y"][part][order].astype(np.float64)
    ra, rb = a_all[part][order], b_all[part][order]
    dist2 = np.float64(distance) * np.float64(distance)
    n, total, out_pairs, out_d2 = len(ids), 0, [], []
    for lo in range(0, n, BLOCK):
        hi = min(lo + BLOCK, n)
        d2 = None if cache is None else cache.get(lo)
        if d2 is None:
            with np.errstate(invalid="ignore", over="ignore"):
                dx = x[lo:hi, None] - x[None, :]
                dy = y[lo:hi, None] - y[None, :]
                d2 = dx * dx + dy * dy
            if cache is not None:
                cache[lo] = d2
        with np.errstate(invalid="ignore"):
            hit = d2 < dist2
        hit &= np.arange(lo, hi)[:, None] < np.arange(n)[None, :]  # every unordered pair once, the smaller id first
        hit &= (ra[lo:hi, None] & rb[None, :]) | (ra[None, :] & rb[lo:hi, None])
        if count_only:
            total += int(hit.sum())
            continue
        p, q = np.nonzero(hit)  # (row-major: ascending p, then ascending q)
        out_pairs.append(np.stack([ids[lo + p], ids[q]], axis=1))
        out_d2.append(d2[p, q])
    if count_only:
        return total
    if not out_pairs:
        return np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.float64)
    return np.concatenate(out_pairs).astype(np.uint64), np.concatenate(out_d2).astype(np.float64)


def close_pairs(sim, distance, sel_a=None, sel_b=None, cap=None, want_d2=True, fill=None):
    """cs_close_pairs / cs_mesh_close_pairs on a Simulation or a NativeTileMesh by the C entry point -> (the returned
    count, uint64[cap, 2] pairs, float64[cap] d2 or None): the whole arrays given, so a test sees what was written.
    cap None: the count-only form (null arrays)."""
    mesh = not hasattr(sim, "_engine")
    fn = sim._lib.cs_mesh_close_pairs if mesh else sim._lib.cs_close_pairs
    handle = sim._mesh if mesh else sim._engine
    a = C.byref(sel_a) if sel_a is not None else None
    b = C.byref(sel_b) if sel_b is not None else None
    if cap is None:
        return fn(handle, float(distance), a, b, None, None, 0), None, None
    out = np.zeros((max(cap, 1), 2), dtype=np.uint64)
    d2 = np.zeros(max(cap, 1), dtype=np.float64) if want_d2 else None
    if fill is not None:
        out.view(np.uint8)[...] = fill
        if d2 is not None:
            d2.view(np.uint8)[...] = fill
    n = fn(handle, float(distance), a, b, out.ctypes.data_as(C.POINTER(_abi.IdPair)),
           d2.ctypes.data_as(C.POINTER(C.c_double)) if want_d2 else None, cap)
    return n, out, d2


def last_error(sim):
    if hasattr(sim, "_engine"):
        return sim._lib.cs_last_error(sim._engine).decode()
    return sim._lib.cs_mesh_last_error(sim._mesh).decode()


def agree(sim, records, grid, distance, sel_a=None, sel_b=None, cols=(None, None, None), name="", cache=None, capped=True):
    """The engine's (or mesh's) pairs, order, count and d2 bits equal the restatement on `records`, in the listing form,
    the count-only form and (capped) under a cap of half the count, with and without distances.  Returns the
    restatement's (pairs, d2).  cache: see pairs()."""
    ra, rb = roles(sel_a, sel_b, records, *cols)
    want, want_d2 = pairs(records, grid, distance, None if sel_a is None else ra, None if sel_b is None else rb, cache=cache)
    n, _, _ = close_pairs(sim, distance, sel_a, sel_b)
    print(f"  {name}: restatement {len(want)} pairs, engine {n}")
    assert n == len(want), (name, last_error(sim) if n == SIZE_MAX else n)
    n, got, got_d2 = close_pairs(sim, distance, sel_a, sel_b, cap=len(want) + 3, fill=0xAB)
    assert n == len(want), name
    assert np.array_equal(got[:n], want), name
    assert got_d2[:n].tobytes() == want_d2.tobytes(), name
    assert (got[n:].view(np.uint8) == 0xAB).all() and (got_d2[n:].view(np.uint8) == 0xAB).all(), name  # nothing beyond
    if capped and len(want) > 1:
        cap = len(want) // 2
        n, few, few_d2 = close_pairs(sim, distance, sel_a, sel_b, cap=cap, fill=0xAB)
        assert n == len(want) and np.array_equal(few, want[:cap]) and few_d2.tobytes() == want_d2[:cap].tobytes(), name
        n, few, none = close_pairs(sim, distance, sel_a, sel_b, cap=cap, want_d2=False)  # pairs without distances
        assert n == len(want) and none is None and np.array_equal(few, want[:cap]), name
    return want, want_d2
