"""The rule of cs_leg_intervals (include/crowdstep_state.h, "Every agent that enters a leg") restated in numpy, and what
the leg-interval tests share.

`intervals` is the definition the engine is compared with, applied to the engine's OWN read_agents(): who takes part by
the rectangle rule of the pairs (close_pairs_reference.takes_part), who is a row and its s_in by legs_reference.rule (the
rule of cs_leg_conflicts), s_out with every product, sum, difference, the square root and the division a separate numpy
operation (rounded once each), legs x agents by brute force in blocks of legs, the rows in (leg, id) order.  It knows
nothing of cells, rows, reaches or an order of visits.  Equality with the engine is exact, on the ids and on the bits of
s_in and s_out; there is no tolerance."""
import ctypes as C

import numpy as np

from rmf_crowdsim_amd import _abi
from rmf_crowdsim_amd.simulation import LEG_DTYPE, LEG_INTERVAL_DTYPE, legs_array
from close_pairs_reference import SIZE_MAX, last_error, roles, takes_part
from legs_reference import block_of, rule


def leaves(x, y, vx, vy, legs, distance, s_in):
    """(s_out, ww) for every (leg, agent), float64 [len(legs), len(x)]: one numpy operation per operation of the header's
    rule; s_in: the s of legs_reference.rule.  Meaningful where that rule says conflict."""
    D2 = np.float64(distance) * np.float64(distance)
    x0, y0 = legs["x0"][:, None], legs["y0"][:, None]
    lvx, lvy = legs["vx"][:, None], legs["vy"][:, None]
    t0 = legs["t0"][:, None]
    T = np.broadcast_to((legs["t1"] - legs["t0"])[:, None], s_in.shape)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        px = x[None, :] + vx[None, :] * t0
        py = y[None, :] + vy[None, :] * t0
        rx = px - x0
        ry = py - y0
        wx = vx[None, :] - lvx
        wy = vy[None, :] - lvy
        a = rx * wx + ry * wy
        ww = wx * wx + wy * wy
        cr = rx * wy - ry * wx
        h2 = D2 * ww - cr * cr
        e = (-a + np.sqrt(h2)) / ww
        e = np.where(e > s_in, e, s_in)
        e = np.where(e < T, e, T)
        s_out = np.where(h2 > 0, e, np.where(ww == 0, T, s_in))
    return s_out, ww


def intervals(records, grid, legs, distance, speed_max, targets=None, stats=None):
    """-> (LEG_INTERVAL_DTYPE rows ascending by (leg, id), uint64 counts per leg).  targets: a bool mask over records
    (None: everyone).  stats (a dict): gets the class counts of `classes`, and "same_velocity", the rows with ww == 0."""
    legs = np.ascontiguousarray(legs, dtype=LEG_DTYPE)
    part = takes_part(records, grid)
    if targets is not None:
        part = part & np.asarray(targets, dtype=bool)
    ids = records["id"][part].astype(np.uint64)
    order = np.argsort(ids, kind="stable")
    ids = ids[order]
    x, y = records["x"][part].astype(np.float64)[order], records["y"][part].astype(np.float64)[order]
    vx = records["vx"][part].astype(np.float32).astype(np.float64)[order]
    vy = records["vy"][part].astype(np.float32).astype(np.float64)[order]
    counts = np.zeros(len(legs), dtype=np.uint64)
    out, same = [], 0
    BLOCK = block_of(len(ids))
    for lo in range(0, len(legs) if len(ids) else 0, BLOCK):
        block = legs[lo:lo + BLOCK]
        hit, s_in, _ = rule(x, y, vx, vy, block, distance, speed_max)
        hit &= ids[None, :] != block["ignore"][:, None]
        s_out, ww = leaves(x, y, vx, vy, block, distance, s_in)
        k, q = np.nonzero(hit)  # (row-major: ascending leg, then ascending id)
        rows = np.zeros(len(k), dtype=LEG_INTERVAL_DTYPE)
        rows["leg"], rows["id"], rows["s_in"], rows["s_out"] = k + lo, ids[q], s_in[k, q], s_out[k, q]
        out.append(rows)
        counts[lo:lo + BLOCK] = hit.sum(axis=1)
        same += int((ww[k, q] == 0).sum())
    rows = np.concatenate(out) if out else np.zeros(0, dtype=LEG_INTERVAL_DTYPE)
    if stats is not None:
        stats.update(classes(rows, counts, legs))
        stats["same_velocity"] = same
    return rows, counts


def classes(rows, counts, legs):
    T = (legs["t1"] - legs["t0"])[rows["leg"].astype(np.int64)]
    return dict(at_start=int((rows["s_in"] == 0.0).sum()), later=int((rows["s_in"] > 0.0).sum()),
                leaves=int((rows["s_out"] < T).sum()), stays=int((rows["s_out"] == T).sum()),
                crowded_legs=int((counts >= 2).sum()), free_legs=int((counts == 0).sum()))


def call(sim, legs, distance, speed_max, sel=None, cap=0, rows=True, counts=True, fill=0xAB, n=None):
    """cs_leg_intervals / cs_mesh_leg_intervals on a Simulation or a NativeTileMesh by the C entry point -> (the returned
    count, the uint64 counts buffer or None, the LEG_INTERVAL_DTYPE buffer of cap + 2 rows or None), both buffers filled
    with `fill` before the call.  rows=False passes the null array with `cap` as given; n: the number of legs passed,
    where it is not len(legs)."""
    mesh = not hasattr(sim, "_engine")
    fn = sim._lib.cs_mesh_leg_intervals if mesh else sim._lib.cs_leg_intervals
    handle = sim._mesh if mesh else sim._engine
    legs = np.ascontiguousarray(legs, dtype=LEG_DTYPE)
    out = per_leg = None
    if rows:
        out = np.zeros(cap + 2, dtype=LEG_INTERVAL_DTYPE)
        out.view(np.uint8)[...] = fill
    if counts:
        per_leg = np.zeros(max(len(legs), 1), dtype=np.uint64)
        per_leg.view(np.uint8)[...] = fill
    got = fn(handle, legs.ctypes.data_as(C.POINTER(_abi.Leg)), len(legs) if n is None else n, float(distance),
             float(speed_max), C.byref(sel) if sel is not None else None,
             per_leg.ctypes.data_as(C.POINTER(C.c_uint64)) if counts else None,
             out.ctypes.data_as(C.POINTER(_abi.LegInterval)) if rows else None, cap)
    return got, per_leg, out


def agree(sim, records, grid, legs, distance, speed_max, sel=None, cols=(None, None, None), name="", stats=None, want=None):
    """The engine's (or mesh's) rows and per-leg counts equal the restatement on `records` byte for byte: listing with
    room for every row (nothing is written behind them), and counting only (a null array; an array with cap == 0, left
    alone; with and without the counts).  Returns the restatement's (rows, counts).  want: the restatement's answer for
    these very arguments, where a test has it already (a mesh after the single engine)."""
    if want is None:
        mask = None if sel is None else roles(sel, None, records, *cols)[0]
        want = intervals(records, grid, legs, distance, speed_max, mask, stats=stats)
    rows, counts = want
    total = len(rows)
    assert int(counts.sum()) == total
    n, per_leg, got = call(sim, legs, distance, speed_max, sel, cap=total)
    print(f"  {name}: {len(legs)} legs, restatement {total} rows, engine {n}")
    assert n == total, (name, last_error(sim) if n == SIZE_MAX else n)
    assert per_leg[:len(legs)].tobytes() == counts.tobytes(), name
    bad = np.nonzero((got[:total]["leg"] != rows["leg"]) | (got[:total]["id"] != rows["id"]) |
                     (got[:total]["s_in"].view(np.uint64) != rows["s_in"].view(np.uint64)) |
                     (got[:total]["s_out"].view(np.uint64) != rows["s_out"].view(np.uint64)))[0]
    assert len(bad) == 0, (name, len(bad), [(got[k].tolist(), rows[k].tolist(), legs[int(rows["leg"][k])].tolist()) for k in bad[:4]])
    assert got[:total].tobytes() == rows.tobytes() and (got[total:].view(np.uint8) == 0xAB).all(), name
    n, per_leg, none = call(sim, legs, distance, speed_max, sel, cap=total + 5, rows=False)
    assert n == total and none is None and per_leg[:len(legs)].tobytes() == counts.tobytes(), name
    n, per_leg, kept = call(sim, legs, distance, speed_max, sel, cap=0, counts=False)
    assert n == total and per_leg is None and (kept.view(np.uint8) == 0xAB).all(), name
    return want


__all__ = ["LEG_DTYPE", "LEG_INTERVAL_DTYPE", "legs_array", "leaves", "intervals", "classes", "call", "agree", "SIZE_MAX",
           "last_error"]
