"""The rule of cs_gate_crossings (include/crowdstep_state.h, "Who crosses a line") restated in numpy, and what the
gate-crossing tests share.

`crossings` is the definition the engine is compared with, applied to the engine's OWN read_agents(): who takes part by
the rectangle rule of the pairs (close_pairs_reference.takes_part), the rule with every product, sum, difference and
division a separate numpy operation (rounded once each), gates x agents by brute force in blocks of gates, the rows in
(gate, id) order.  It knows nothing of cells, rows, reaches or an order of visits.  Equality with the engine is exact, on
the ids, on dir and on the bits of s and u; there is no tolerance."""
import ctypes as C

import numpy as np

from rmf_crowdsim_amd import _abi
from rmf_crowdsim_amd.simulation import GATE_CROSSING_DTYPE, GATE_DTYPE, gates_array, path_gates
from close_pairs_reference import SIZE_MAX, last_error, roles, takes_part
from legs_reference import block_of


def rule(x, y, vx, vy, gates, speed_max):
    """(crossing, dir, s, u) for every (gate, agent): bool, int32 and float64 arrays [len(gates), len(x)], one numpy
    operation per operation of the header's rule.  x, y, vx, vy: float64 (the velocity the f32 of the record, widened)."""
    with np.errstate(over="ignore"):
        S2 = np.float64(speed_max) * np.float64(speed_max)
    ax, ay = gates["ax"][:, None], gates["ay"][:, None]
    bx, by = gates["bx"][:, None], gates["by"][:, None]
    t0 = gates["t0"][:, None]
    T = (gates["t1"] - gates["t0"])[:, None]
    x, y, vx, vy = x[None, :], y[None, :], vx[None, :], vy[None, :]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ss = vx * vx + vy * vy
        slow = ss < S2
        px = x + vx * t0
        py = y + vy * t0
        ex = bx - ax
        ey = by - ay
        rx = px - ax
        ry = py - ay
        c0 = ex * ry - ey * rx
        cv = ex * vy - ey * vx
        cu = rx * vy - ry * vx
        towards = ((cv > 0) & (c0 <= 0)) | ((cv < 0) & (c0 >= 0))
        s = (-c0) / cv
        s = np.where(s > 0, s, np.float64(0.0))
        u = cu / cv
        hit = slow & towards & (s < T) & (u >= 0) & (u < 1)
    return hit, np.where(cv > 0, 1, -1).astype(np.int32), s, u


def crossings(records, grid, gates, speed_max, mask=None, stats=None):
    """-> (GATE_CROSSING_DTYPE rows ascending by (gate, id), uint64 counts [len(gates), 2]: dir +1, dir -1).  mask: a bool
    mask over records, the filter (None: everyone).  stats (a dict): gets the class counts of `classes`."""
    gates = np.ascontiguousarray(gates, dtype=GATE_DTYPE)
    part = takes_part(records, grid)
    if mask is not None:
        part = part & np.asarray(mask, dtype=bool)
    ids = records["id"][part].astype(np.uint64)
    order = np.argsort(ids, kind="stable")
    ids = ids[order]
    x, y = records["x"][part].astype(np.float64)[order], records["y"][part].astype(np.float64)[order]
    vx = records["vx"][part].astype(np.float32).astype(np.float64)[order]
    vy = records["vy"][part].astype(np.float32).astype(np.float64)[order]
    counts = np.zeros((len(gates), 2), dtype=np.uint64)
    out = []
    BLOCK = block_of(len(ids))
    for lo in range(0, len(gates) if len(ids) else 0, BLOCK):
        block = gates[lo:lo + BLOCK]
        hit, dirs, s, u = rule(x, y, vx, vy, block, speed_max)
        k, q = np.nonzero(hit)  # (row-major: ascending gate, then ascending id)
        rows = np.zeros(len(k), dtype=GATE_CROSSING_DTYPE)
        rows["gate"], rows["dir"], rows["id"], rows["s"], rows["u"] = k + lo, dirs[k, q], ids[q], s[k, q], u[k, q]
        out.append(rows)
        counts[lo:lo + BLOCK, 0] = (hit & (dirs > 0)).sum(axis=1)
        counts[lo:lo + BLOCK, 1] = (hit & (dirs < 0)).sum(axis=1)
    rows = np.concatenate(out) if out else np.zeros(0, dtype=GATE_CROSSING_DTYPE)
    if stats is not None:
        stats.update(classes(rows, counts))
    return rows, counts


def classes(rows, counts):
    per_gate = counts.sum(axis=1)
    return dict(left=int((rows["dir"] == 1).sum()), right=int((rows["dir"] == -1).sum()),
                at_start=int((rows["s"] == 0.0).sum()), later=int((rows["s"] > 0.0).sum()),
                empty_gates=int((per_gate == 0).sum()), crowded_gates=int((per_gate >= 2).sum()))


def call(sim, gates, speed_max, sel=None, cap=0, rows=True, counts=True, fill=0xAB, n=None, null_gates=False):
    """cs_gate_crossings / cs_mesh_gate_crossings on a Simulation or a NativeTileMesh by the C entry point -> (the
    returned count, the uint64 counts buffer [n, 2] or None, the GATE_CROSSING_DTYPE buffer of cap + 2 rows or None), both
    buffers filled with `fill` before the call.  rows=False passes the null array with `cap` as given; n: the number of
    gates passed, where it is not len(gates)."""
    mesh = not hasattr(sim, "_engine")
    fn = sim._lib.cs_mesh_gate_crossings if mesh else sim._lib.cs_gate_crossings
    handle = sim._mesh if mesh else sim._engine
    gates = np.ascontiguousarray(gates, dtype=GATE_DTYPE)
    out = per_gate = None
    if rows:
        out = np.zeros(cap + 2, dtype=GATE_CROSSING_DTYPE)
        out.view(np.uint8)[...] = fill
    if counts:
        per_gate = np.zeros((max(len(gates), 1), 2), dtype=np.uint64)
        per_gate.view(np.uint8)[...] = fill
    got = fn(handle, None if null_gates else gates.ctypes.data_as(C.POINTER(_abi.Gate)), len(gates) if n is None else n,
             float(speed_max), C.byref(sel) if sel is not None else None,
             per_gate.ctypes.data_as(C.POINTER(C.c_uint64)) if counts else None,
             out.ctypes.data_as(C.POINTER(_abi.GateCrossing)) if rows else None, cap)
    return got, per_gate, out


def agree(sim, records, grid, gates, speed_max, sel=None, cols=(None, None, None), name="", stats=None, want=None):
    """The engine's (or mesh's) rows and counts equal the restatement on `records` byte for byte: listing with room for
    every row (nothing is written behind them), and counting only (a null array; an array with cap == 0, left alone; with
    and without the counts).  Returns the restatement's (rows, counts).  want: the restatement's answer for these very
    arguments, where a test has it already (a mesh after the single engine)."""
    if want is None:
        mask = None if sel is None else roles(sel, None, records, *cols)[0]
        want = crossings(records, grid, gates, speed_max, mask, stats=stats)
    rows, counts = want
    total = len(rows)
    assert int(counts.sum()) == total
    n, per_gate, got = call(sim, gates, speed_max, sel, cap=total)
    print(f"  {name}: {len(gates)} gates, restatement {total} rows, engine {n}")
    assert n == total, (name, last_error(sim) if n == SIZE_MAX else n)
    assert per_gate[:len(gates)].tobytes() == counts.tobytes(), name
    bad = np.nonzero((got[:total]["gate"] != rows["gate"]) | (got[:total]["id"] != rows["id"]) |
                     (got[:total]["dir"] != rows["dir"]) |
                     (got[:total]["s"].view(np.uint64) != rows["s"].view(np.uint64)) |
                     (got[:total]["u"].view(np.uint64) != rows["u"].view(np.uint64)))[0]
    assert len(bad) == 0, (name, len(bad), [(got[k].tolist(), rows[k].tolist(), gates[int(rows["gate"][k])].tolist()) for k in bad[:4]])
    assert got[:total].tobytes() == rows.tobytes() and (got[total:].view(np.uint8) == 0xAB).all(), name
    n, per_gate, none = call(sim, gates, speed_max, sel, cap=total + 5, rows=False)
    assert n == total and none is None and per_gate[:len(gates)].tobytes() == counts.tobytes(), name
    n, per_gate, kept = call(sim, gates, speed_max, sel, cap=0, counts=False)
    assert n == total and per_gate is None and (kept.view(np.uint8) == 0xAB).all(), name
    return want


__all__ = ["GATE_DTYPE", "GATE_CROSSING_DTYPE", "gates_array", "path_gates", "rule", "crossings", "classes", "call", "agree",
           "SIZE_MAX", "last_error"]
