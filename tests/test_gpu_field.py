"""Rasterising the crowd on one engine (include/crowdstep_state.h, cs_agent_field; Simulation.agent_field): the engine
against the numpy restatement of the rules (tests/field_reference.py) applied to its OWN read_agents().  Counts are equal,
every bin of every raster; sums lie within n * 2^-52 * sum|v| of the exactly rounded sum and are equal where a bin holds
one agent or none ("Rasterising the crowd between steps")."""
import ctypes as C

import numpy as np
import pytest

from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, LocationHash2D,
                              NoLocalPlan, Selection, Simulation, StubHighLevelPlan, Zanlungo, _abi, scenes)
from field_reference import bins_of, check, desc, field, last_error, raster
from select_reference import Ledger, add_three_sinks, drain, keep_events, selection, selections_for
from test_gpu_agent_write import _add_crossing, _crossing, _steps

pytestmark = pytest.mark.gpu
FLAGS = [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER]
FILTERS = ("term 4", "term 8", "term 32", "term 64", "terms 1+2")  # owner, planner, waypoint, speed, rect AND circle


def _scene(flags, twins=1, n=4096):
    """Twins of the crossing crowd plus three source-sinks, each with the ledger of who owns whom."""
    pts, pref, group, grid, extent = _crossing(n)
    sims, ledgers, sinks = [], [], None
    for _ in range(twins):
        s = Simulation(LocationHash2D(**grid), flags=flags)
        ledgers.append(Ledger(s).watch())
        keep_events(s)
        _add_crossing(s, pts, group)
        sinks = add_three_sinks(s, extent)
        sims.append(s)
    return sims, ledgers, sinks, grid


def _advance(sims, ledgers, k):
    for s, led in zip(sims, ledgers):
        for _ in range(k):
            s.step(0.05)
        led.hear(drain(s))


def _edge_pair(rec, axis, rng):
    """Two agents a, b with rec[axis][a] < rec[axis][b] and a quarter of their distance a normal number"""
    while True:
        a, b = (int(v) for v in rng.choice(len(rec), 2, replace=False))
        if rec[axis][a] > rec[axis][b]:
            a, b = b, a
        if rec[axis][b] - rec[axis][a] > 1.0:
            return a, b


def _rasters(rec, grid, rng):
    """(name, desc) around the crowd in `rec`"""
    x, y = rec["x"], rec["y"]
    lo_x, lo_y, hi_x, hi_y = float(x.min()), float(y.min()), float(x.max()), float(y.max())
    span = max(hi_x - lo_x, hi_y - lo_y) * 1.001
    cell = grid["cell_size"]
    off = grid["offset"]
    out = [("1 x 1", desc(lo_x - 1.0, lo_y - 1.0, span + 2.0, span + 2.0, 1, 1)),
           ("37 x 1", desc(lo_x, lo_y - 1.0, span / 37, span + 2.0, 37, 1)),
           ("1 x 37", desc(lo_x - 1.0, lo_y, span + 2.0, span / 37, 1, 37)),
           ("8 x 8 over the crowd", desc(lo_x, lo_y, span / 8, span / 8, 8, 8)),
           ("the simulation's cells", desc(off[0], off[1], cell, cell, int(np.ceil(grid["width"] / cell)),
                                           int(np.ceil(grid["height"] / cell)))),
           ("512 x 512, a tenth of a cell", desc(float(np.median(x)) - 25.6 * cell, float(np.median(y)) - 25.6 * cell,
                                                 cell / 10, cell / 10, 512, 512)),
           ("half outside the crowd", desc(float(np.median(x)), float(np.median(y)), 1.0, 1.0, 200, 200)),
           ("wholly outside the crowd", desc(lo_x - 500.0, lo_y - 500.0, 1.0, 1.0, 64, 64)),
           ("non-square bins", desc(lo_x + 3.0, lo_y + 1.0, 1.7, 0.6, 45, 150))]
    # rasters built from read-back coordinates: agent a exactly on the low edge, agent b exactly on bin edge 4 (cell_w =
    # (x_b - x_a) / 4 is exact, so (x_b - x_a) / cell_w == 4.0): outside a raster of 4 bins, in bin 4 of one of 8; the
    # other axis is one bin that holds everybody
    for axis in ("x", "y"):
        a, b = _edge_pair(rec, axis, rng)
        lo, quarter = float(rec[axis][a]), float((rec[axis][b] - rec[axis][a]) / 4)
        assert (np.float64(rec[axis][b]) - np.float64(lo)) / np.float64(quarter) == 4.0
        for n_bins in (4, 8):
            d = (desc(lo, lo_y - 1.0, quarter, span + 2.0, n_bins, 1) if axis == "x" else
                 desc(lo_x - 1.0, lo, span + 2.0, quarter, 1, n_bins))
            out.append((f"{axis} edges on agents {rec['id'][a]}, {rec['id'][b]}, {n_bins} bins", d))
    return out


@pytest.mark.parametrize("flags", FLAGS)
def test_every_raster_with_and_without_a_filter_equals_the_restatement(flags):
    (a,), (led,), sinks, grid = _scene(flags)
    rng = np.random.default_rng(17)
    for steps, total in ((10, 10), (30, 40)):
        _advance((a,), (led,), steps)
        rec = a.read_agents()
        cols = led.columns(rec)
        sels = dict(selections_for(rec, led, sinks))
        filters = [("no filter", None)] + [(n, sels[n]) for n in FILTERS]
        many = {}
        for name, d in _rasters(rec, grid, rng):
            for f_name, sel in filters:
                want = raster(d, rec, sel, *cols)
                rc, count, sums = field(a, d, sel)
                assert rc == 0, (name, f_name, last_error(a))
                print(f"flags {flags}, {total} steps, {name}, {f_name}: {int(want[0].sum())} agents in "
                      f"{int((want[0] > 0).sum())} of {want[0].size} bins, fullest {int(want[0].max())}")
                crowded, single = check(f"{name}, {f_name}", count, sums, want)
                many[(name, f_name)] = (crowded, single, int(want[0].sum()))
            inside, flat = bins_of(d, rec["x"], rec["y"])
            if " edges on agents " in name:  # who sits exactly on an edge falls the way the rule says
                at = {int(i): k for k, i in enumerate(rec["id"])}
                ka, kb = (at[int(v)] for v in name.split("agents ")[1].split(", ")[:2])
                assert inside[ka] and flat[ka] == 0
                assert (not inside[kb]) if max(d.nx, d.ny) == 4 else (inside[kb] and flat[kb] == 4)
        # the scenes exercise what they are meant to
        assert many[("1 x 1", "no filter")][2] == len(rec)
        assert many[("wholly outside the crowd", "no filter")][2] == 0
        assert 0 < many[("half outside the crowd", "no filter")][2] < len(rec)
        assert many[("8 x 8 over the crowd", "no filter")][0] >= 32 and many[("the simulation's cells", "no filter")][0] > 200
        assert many[("512 x 512, a tenth of a cell", "no filter")][1] > 1000  # single-agent bins in the fine raster
        for f_name in FILTERS:  # every filter lets somebody through, and not everybody
            assert 0 < many[("1 x 1", f_name)][2] < len(rec), f_name
        assert a.read_agents().tobytes() == rec.tobytes()


def test_counts_only_sums_only_and_both_and_the_python_surface():
    (a,), (led,), sinks, grid = _scene(0)
    _advance((a,), (led,), 15)
    rec = a.read_agents()
    rng = np.random.default_rng(2)
    fast = selection(_abi.CS_SEL_SPEED, speed_lo=1.0, speed_hi=float("inf"))
    for name, d in _rasters(rec, grid, rng)[3:6]:
        for sel in (None, fast):
            want = raster(d, rec, sel, *led.columns(rec))
            rc, count, none = field(a, d, sel, want="count")
            assert rc == 0 and none is None
            check(name + " (counts only)", count, None, want)
            rc, none, sums = field(a, d, sel, want="sums")
            assert rc == 0 and none is None
            check(name + " (sums only)", None, sums, want)
            rc, both_count, both_sums = field(a, d, sel, want="both")
            assert rc == 0 and np.array_equal(both_count, count)
            check(name + " (both)", both_count, both_sums, want)
            few = want[0] <= 1  # (sums of several agents may differ in their last bits from call to call: any order)
            assert np.array_equal(both_sums[few], sums[few])
    # Simulation.agent_field: shape is (ny, nx), cell a scalar or a pair, selection what count_agents accepts
    d = desc(float(np.median(rec["x"])) - 20.0, float(np.median(rec["y"])) - 10.0, 2.5, 0.8, 16, 25)
    count = a.agent_field((d.x0, d.y0), (2.5, 0.8), (25, 16))
    assert isinstance(count, np.ndarray) and count.dtype == np.uint32 and count.shape == (25, 16)
    check("agent_field", count, None, raster(d, rec))
    count, sum_v = a.agent_field((d.x0, d.y0), (2.5, 0.8), (25, 16), velocity=True)
    assert sum_v.dtype == np.float64 and sum_v.shape == (25, 16, 2)
    check("agent_field with velocity", count, sum_v, raster(d, rec))
    square = desc(d.x0, d.y0, 2.5, 2.5, 16, 25)
    rect = (d.x0 + 5.0, d.y0 + 5.0, d.x0 + 30.0, d.y0 + 40.0)
    want = raster(square, rec, selection(_abi.CS_SEL_RECT, x0=rect[0], y0=rect[1], x1=rect[2], y1=rect[3]), *led.columns(rec))
    for sel in (Selection(rect=rect), dict(rect=rect)):
        count, sum_v = a.agent_field((d.x0, d.y0), 2.5, (25, 16), selection=sel, velocity=True)
        check("agent_field with a selection", count, sum_v, want)
    assert 0 < int(want[0].sum()) < len(rec)
    with pytest.raises(CrowdSimError, match="agent_field"):
        a.agent_field((0.0, 0.0), -1.0, (4, 4))
    assert a.read_agents().tobytes() == rec.tobytes()


def test_both_forms_of_the_kernel_give_the_same_raster(monkeypatch):
    """Rasters small enough for the LDS-privatised form, rasterised by it and (CS_FIELD_LDS_BYTES=0) by the form that
    adds to global memory; and a crowd whose slots are not in cell order (positions written between steps)."""
    (a,), (led,), sinks, grid = _scene(0)
    _advance((a,), (led,), 12)
    rng = np.random.default_rng(8)
    rows = a.read_agents()
    rows = rows[rng.choice(len(rows), 1500, replace=False)].copy()
    rows["x"] = rng.uniform(rows["x"].min(), rows["x"].max(), len(rows))
    rows["y"] = rng.uniform(rows["y"].min(), rows["y"].max(), len(rows))
    for shuffled in (False, True):
        if shuffled:
            a.write_agents(rows, "position")  # (no step since: the slots are where they were, the agents are not)
        rec = a.read_agents()
        for name, d in _rasters(rec, grid, rng)[:5]:
            want = raster(d, rec)
            got = {}
            for limit in (None, "0"):
                if limit is None:
                    monkeypatch.delenv("CS_FIELD_LDS_BYTES", raising=False)
                else:
                    monkeypatch.setenv("CS_FIELD_LDS_BYTES", limit)
                rc, count, sums = field(a, d)
                assert rc == 0
                check(f"{name}, shuffled {shuffled}, LDS limit {limit}", count, sums, want)
                got[limit] = count
            assert np.array_equal(got[None], got["0"])
    monkeypatch.delenv("CS_FIELD_LDS_BYTES", raising=False)


def test_refused_rasters_leave_the_outputs_and_the_engine_as_they_were():
    (a,), (led,), sinks, grid = _scene(0)
    _advance((a,), (led,), 12)
    rec = a.read_agents()
    nan, inf = float("nan"), float("inf")
    good = desc(40.0, 40.0, 3.0, 3.0, 20, 20)
    bad = [("NaN x0", desc(nan, 0.0, 1.0, 1.0, 4, 4)), ("inf x0", desc(inf, 0.0, 1.0, 1.0, 4, 4)),
           ("NaN y0", desc(0.0, nan, 1.0, 1.0, 4, 4)), ("-inf y0", desc(0.0, -inf, 1.0, 1.0, 4, 4)),
           ("NaN cell_w", desc(0.0, 0.0, nan, 1.0, 4, 4)), ("inf cell_w", desc(0.0, 0.0, inf, 1.0, 4, 4)),
           ("NaN cell_h", desc(0.0, 0.0, 1.0, nan, 4, 4)), ("inf cell_h", desc(0.0, 0.0, 1.0, inf, 4, 4)),
           ("cell_w == 0", desc(0.0, 0.0, 0.0, 1.0, 4, 4)), ("cell_w < 0", desc(0.0, 0.0, -1.0, 1.0, 4, 4)),
           ("cell_h == 0", desc(0.0, 0.0, 1.0, 0.0, 4, 4)), ("cell_h < 0", desc(0.0, 0.0, 1.0, -2.0, 4, 4)),
           ("nx == 0", desc(0.0, 0.0, 1.0, 1.0, 0, 4)), ("ny == 0", desc(0.0, 0.0, 1.0, 1.0, 4, 0)),
           ("one bin more than CS_FIELD_MAX_CELLS", desc(0.0, 0.0, 1.0, 1.0, 5, 838861)),
           ("nx * ny beyond 32 bits", desc(0.0, 0.0, 1.0, 1.0, 2 ** 31, 2))]
    assert 5 * 838861 == _abi.CS_FIELD_MAX_CELLS + 1

    def refused(rc, outs, name):
        assert rc == 3, name
        assert "agent_field" in last_error(a), (name, last_error(a))
        for o in outs:
            assert (o.view(np.uint8) == 0xAB).all(), name
        rc, count, sums = field(a, good)
        assert rc == 0
        check(f"after the refusal of {name}", count, sums, raster(good, rec))
    for name, d in bad:
        rc, count, sums = field(a, d, fill=0xAB)
        refused(rc, (count, sums), name)
    lib, e = a._lib, a._engine
    count = np.full(400, 0xABABABAB, dtype=np.uint32)
    vx = np.frombuffer(b"\xab" * 3200, dtype=np.float64).copy()
    vy = vx.copy()
    p_c, p_x, p_y = count.ctypes.data_as(C.POINTER(C.c_uint32)), vx.ctypes.data_as(C.POINTER(C.c_double)), \
        vy.ctypes.data_as(C.POINTER(C.c_double))
    refused(lib.cs_agent_field(e, None, None, p_c, p_x, p_y), (count, vx, vy), "a null description")
    refused(lib.cs_agent_field(e, C.byref(good), None, None, None, None), (count, vx, vy), "no output")
    refused(lib.cs_agent_field(e, C.byref(good), None, p_c, p_x, None), (count, vx, vy), "sum_vx without sum_vy")
    refused(lib.cs_agent_field(e, C.byref(good), None, None, None, p_y), (count, vx, vy), "sum_vy without sum_vx")
    for name, sel in (("unknown term bits", selection(128)), ("a NaN rectangle", selection(_abi.CS_SEL_RECT, x0=nan)),
                      ("a negative radius", selection(_abi.CS_SEL_CIRCLE, r=-1.0))):
        refused(lib.cs_agent_field(e, C.byref(good), C.byref(sel), p_c, p_x, p_y), (count, vx, vy), name)
    assert len(a) == len(rec) and a.read_agents().tobytes() == rec.tobytes() and drain(a) == []
    a.step(0.05)  # (not poisoned)


def test_an_agent_the_index_never_took_is_binned_where_it_was_created():
    pts, pref, group, grid, extent = _crossing(1024)
    a = Simulation(LocationHash2D(**grid))
    _add_crossing(a, pts, group)
    _steps((a,), 3)
    where = (grid["width"] * 5.0 + 0.75, 1.0)
    with pytest.raises(CrowdSimError):  # created, then refused by the index (lib.rs:133-149)
        a.add_agents([where], StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 1.5)
    rec = a.read_agents()
    assert len(rec) == 1025 and (float(rec["x"][-1]), float(rec["y"][-1])) == where
    round_it = desc(where[0] - 1.0, 0.0, 0.5, 0.5, 4, 4)  # fx = 2.0, fy = 2.0: bin (2, 2)
    rc, count, sums = field(a, round_it)
    assert rc == 0 and count[2, 2] == 1 and int(count.sum()) == 1 and (sums == 0.0).all()
    check("round the agent", count, sums, raster(round_it, rec))
    everything = desc(-10.0, -10.0, grid["width"] * 6.0, grid["height"] * 6.0, 2, 2)
    rc, count, sums = field(a, everything)
    assert rc == 0 and int(count.sum()) == 1025
    check("the whole plane", count, sums, raster(everything, rec))
    moving = selection(_abi.CS_SEL_SPEED, speed_lo=0.1, speed_hi=9.0)  # (at rest: the filter leaves it out)
    rc, count, _ = field(a, round_it, moving)
    assert rc == 0 and int(count.sum()) == 0
    with pytest.raises(CrowdSimError, match="Index out of bounds"):  # every step still fails on it (lib.rs:299-302)
        a.step(0.05)


@pytest.mark.parametrize("flags", FLAGS)
def test_fields_between_steps_disturb_nothing(flags):
    """Twins: one is asked for a raster between every two steps, the other never; after 40 steps they are equal to the
    byte and have fired the same events."""
    (a, b), ledgers, sinks, grid = _scene(flags, twins=2)
    rec = a.read_agents()
    assert rec.tobytes() == b.read_agents().tobytes()
    rasters = _rasters(rec, grid, np.random.default_rng(3))
    fast = selection(_abi.CS_SEL_SPEED, speed_lo=0.5, speed_hi=3.0)
    for k in range(40):
        a.step(0.05)
        b.step(0.05)
        name, d = rasters[k % len(rasters)]
        rc, count, sums = field(a, d, fast if k % 3 == 0 else None, want=("both", "count", "sums")[k % 3])
        assert rc == 0, name
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert drain(a) == drain(b)
    kept = [s.kernel_stat(_abi.CS_STAT_STEPS_ON_KEPT_WINDOWS) for s in (a, b)]
    assert kept[0] == kept[1]


def test_wide_ids_give_the_same_rasters():
    sims = []
    for flags in (0, CS_CFG_WIDE_IDS):
        (s,), (led,), sinks, grid = _scene(flags)
        _advance((s,), (led,), 20)
        sims.append(s)
    a, w = sims
    rec = a.read_agents()
    assert w.read_agents().tobytes() == rec.tobytes()
    for name, d in _rasters(rec, grid, np.random.default_rng(5))[2:7]:
        want = raster(d, rec)
        rc, count, sums = field(a, d)
        rc_w, count_w, sums_w = field(w, d)
        assert rc == 0 and rc_w == 0 and np.array_equal(count, count_w), name
        check(name + " (wide ids)", count_w, sums_w, want)
        check(name, count, sums, want)


def test_the_largest_raster_and_one_bin_more():
    (a,), (led,), sinks, grid = _scene(0)
    _advance((a,), (led,), 8)
    rec = a.read_agents()
    before = a._lib.cs_device_bytes(a._engine)
    d = desc(float(rec["x"].min()) - 1.0, float(rec["y"].min()) - 1.0, 0.07, 0.07, 2048, 2048)
    assert d.nx * d.ny == _abi.CS_FIELD_MAX_CELLS
    rc, count, sums = field(a, d)
    assert rc == 0
    crowded, single = check("2048 x 2048", count, sums, raster(d, rec))
    assert int(count.sum()) > 3000 and single > 3000
    grown = a._lib.cs_device_bytes(a._engine) - before  # the raster's scratch is the engine's, and counted
    assert grown >= d.nx * d.ny * 20
    rc, count, sums = field(a, desc(d.x0, d.y0, 0.07, 0.07, 5, 838861), fill=0xAB)
    assert rc == 3 and "agent_field" in last_error(a) and (count.view(np.uint8) == 0xAB).all()
    assert a._lib.cs_device_bytes(a._engine) - before == grown
    a.step(0.05)


def test_a_million_agents_on_a_1024_x_1024_raster_with_velocities():
    """One scene build and one call.  The sums of the restatement are np.add.at in f64 here (recursive summation in record
    order, itself within (n - 1) * 2^-53 * sum|v| of the exact sum, which the bound's factor two covers): math.fsum per
    bin over a million agents takes too long on the test machine's 16 cores."""
    pts, grid, extent, group = scenes.uniform_crowd(1_000_000, seed=5, cell_size=2.0)
    a = Simulation(LocationHash2D(**grid))
    scenes.add_counterflow(a, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    _steps((a,), 5)
    rec = a.read_agents()
    assert len(rec) == 1_000_000
    lo_x, lo_y = float(rec["x"].min()), float(rec["y"].min())
    span = max(float(rec["x"].max()) - lo_x, float(rec["y"].max()) - lo_y) * 1.0001
    d = desc(lo_x, lo_y, span / 1024, span / 1024, 1024, 1024)
    want = raster(d, rec, exact_sums=False)
    rc, count, sums = field(a, d)
    assert rc == 0
    crowded, single = check("a million agents, 1024 x 1024", count, sums, want)
    print(f"{int(count.sum())} agents in {int((count > 0).sum())} bins, {crowded} bins with two or more, {single} with one")
    assert int(count.sum()) == 1_000_000 and crowded > 10_000 and single > 10_000  # (both kinds of bins, in numbers)
