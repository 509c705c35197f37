"""Rays against the crowd on one engine (include/crowdstep_state.h, Simulation.cast_rays / count_ray_hits): the engine
against the numpy restatement of the rule (tests/rays_reference.py) applied to its OWN read_agents().  Equality is exact:
the id and the bits of t of every ray, and the returned count; there is no tolerance anywhere ("Rays
against the crowd between steps")."""
import ctypes as C

import numpy as np
import pytest

from rmf_crowdsim_amd import (CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS, CrowdSimError, LocationHash2D,
                              NoLocalPlan, Selection, Simulation, StubHighLevelPlan, Zanlungo, _abi, scenes)
from close_pairs_reference import rectangle, roles, takes_part
from rays_reference import NO_HIT, RAY_HIT_DTYPE, SIZE_MAX, agree, call, cast, classes, last_error, rays_array
from select_reference import NO_SINK, drain, selection
from test_gpu_agent_write import _steps
from test_gpu_encounters import _advance, _scene

pytestmark = pytest.mark.gpu
FLAGS = [0, CS_CFG_FORCE_TILED, CS_CFG_FORCE_GATHER]
INF = float("inf")
# (radius, reach in metres: t_max = reach / the nominal length of u).  The crossing crowd holds 0.3 agents per square
# metre, so a ray is 1 / (2 * radius * 0.3) metres from disc to disc on average: 8 m at 0.2 m.  A reach of 1 m at that radius
# leaves fewer than 20 hits with t > 0 among the rays below, so the short query has a radius of 0.4 m and reaches 2 m.
QUERIES = [(0.4, 2.0), (0.05, 3.0), (0.2, INF)]
LENGTHS = (1e-3, 1.0, 1e3)


def ray_sets(rec, grid, reach, seed=7, beams=360, casters=4, segments=500):
    """The rays of one query, from the engine's own records: fans of `beams` beams from `casters` agents' positions with
    `ignore` set to the caster, the same fans without it (each of those rays hits its caster at t == 0), and `segments`
    random rays with origins up to 10 m outside the grid's rectangle, every sixth of them parallel to an axis (ux == 0.0 or
    uy == 0.0 exactly).  Directions have length 1e-3, 1 or 1e3 in turn and t_max = reach / that length."""
    rng = np.random.default_rng(seed)
    part = rec[takes_part(rec, grid)]
    part = part[np.argsort(part["id"])]
    who = part[(np.arange(casters) * 2 + 1) * len(part) // (2 * casters)]
    phi = 2.0 * np.pi * np.arange(beams) / beams
    unit = np.column_stack([np.cos(phi), np.sin(phi)])
    o, u, ign = [], [], []
    for with_ignore in (True, False):
        for a in who:
            o.append(np.repeat([[a["x"], a["y"]]], beams, axis=0))
            u.append(unit)
            ign.append(np.full(beams, a["id"] if with_ignore else _abi.CS_NO_HIT, dtype=np.uint64))
    gx0, gx1, gy0, gy1 = rectangle(grid)
    so = np.column_stack([rng.uniform(gx0 - 10.0, gx1 + 10.0, segments), rng.uniform(gy0 - 10.0, gy1 + 10.0, segments)])
    crowd = np.column_stack([part["x"], part["y"]])
    aim = crowd[rng.integers(0, len(crowd), segments)] + rng.normal(0.0, 1.0, (segments, 2))  # most of them towards the crowd
    su = aim - so
    su /= np.hypot(su[:, 0], su[:, 1])[:, None]
    su[::4] = -su[::4]  # (a quarter look away)
    su[0::6, 0] = 0.0
    su[0::6, 1] = np.where(su[0::6, 1] < 0.0, -1.0, 1.0)
    su[3::6, 1] = 0.0
    su[3::6, 0] = np.where(su[3::6, 0] < 0.0, -1.0, 1.0)
    so[0::6, 0] = crowd[rng.integers(0, len(crowd), len(so[0::6])), 0] + 0.1  # (axis-parallel rays through the crowd)
    so[3::6, 1] = crowd[rng.integers(0, len(crowd), len(so[3::6])), 1] - 0.1
    o.append(so)
    u.append(su)
    ign.append(np.full(segments, _abi.CS_NO_HIT, dtype=np.uint64))
    o, u, ign = np.concatenate(o), np.concatenate(u), np.concatenate(ign)
    length = np.asarray(LENGTHS)[np.arange(len(o)) % len(LENGTHS)]
    rays = rays_array(o, u * length[:, None], reach / length, ign)
    assert (rays["ux"] == 0.0).sum() >= segments // 7 and (rays["uy"] == 0.0).sum() >= segments // 7
    return rays


def check_query(sim, rec, grid, radius, reach, name, sel=None, cols=(None, None, None), want_classes=True):
    """One query of QUERIES on the ray sets: the class counts by the restatement ALONE (printed, then asserted), then the
    engine against it."""
    rays = ray_sets(rec, grid, reach)
    stats = {}
    mask = None if sel is None else roles(sel, None, rec, *cols)[0]
    want = cast(rec, grid, rays, radius, mask, stats=stats)
    moving, still, miss = classes(want)
    print(f"  {name}: restatement alone: {moving} hits with t > 0, {still} with t == 0, {miss} misses, "
          f"{stats['not_nearest']} winners that are not the candidate nearest the origin")
    if want_classes:
        assert moving >= 20 and still >= 20 and miss >= 20 and stats["not_nearest"] >= 5
    agree(sim, rec, grid, rays, radius, sel, cols, name, want=want)
    return rays, want, stats


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", [1024, 4096])
def test_the_crossing_crowd_equals_the_restatement(n, flags):
    a, led, _, grid = _scene(flags, n)
    _advance(a, led, 40)
    rec = a.read_agents()
    assert len(rec) == n and takes_part(rec, grid).all()
    for radius, reach in QUERIES:
        rays, want, _ = check_query(a, rec, grid, radius, reach, f"{n} agents, flags {flags}, {(radius, reach)}")
    # the Python surface (the last query)
    o, u = np.column_stack([rays["ox"], rays["oy"]]), np.column_stack([rays["ux"], rays["uy"]])
    got = a.cast_rays(o, u, radius, t_max=rays["t_max"], ignore=rays["ignore"])
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert a.count_ray_hits(o, u, radius, t_max=rays["t_max"], ignore=rays["ignore"]) == int((want["id"] != NO_HIT).sum())
    one = a.cast_rays(o[:7], u[:7], radius, t_max=float(rays["t_max"][0]), ignore=int(rays["ignore"][0]))  # scalars
    assert one.tobytes() == cast(rec, grid, rays_array(o[:7], u[:7], rays["t_max"][0], rays["ignore"][0]), radius).tobytes()
    assert a.cast_rays(np.zeros((0, 2)), np.zeros((0, 2)), radius).shape == (0,)
    assert a.read_agents().tobytes() == rec.tobytes()


def test_targets():
    a, led, sinks, grid = _scene(sinks=True)
    _advance(a, led, 40)
    rec = a.read_agents()
    cols = led.columns(rec)
    owners = np.asarray(cols[0])
    spawned = [int(s) for s in np.unique(owners) if int(s) != NO_SINK]
    assert spawned  # (agents of a source-sink are alive)
    half = selection(_abi.CS_SEL_RECT, x0=-INF, y0=-INF, x1=float(np.median(rec["x"])), y1=INF)
    pace = float(np.median(np.hypot(rec["vx"].astype(np.float64), rec["vy"].astype(np.float64))))  # (half are slower)
    slow = selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=pace)
    of_sink = selection(_abi.CS_SEL_SOURCE_SINK, source_sink=spawned[0])
    nobody = selection(_abi.CS_SEL_LP, lp=12345)
    everyone = check_query(a, rec, grid, 0.2, INF, "no targets")[1]
    for name, sel in (("a rect", half), ("a speed", slow), ("a source-sink", of_sink)):
        _, want, _ = check_query(a, rec, grid, 0.2, INF, name, sel, cols, want_classes=False)
        hit = want["id"] != NO_HIT
        allowed = set(rec["id"][roles(sel, None, rec, *cols)[0]].tolist())
        assert set(want["id"][hit].tolist()) <= allowed and (want["t"] >= everyone["t"]).all()
        if sel is not of_sink:
            assert hit.any() and (want["id"] != everyone["id"]).any()  # (the others are transparent)
    # rays aimed at the agents of that source-sink from 3 m away, through whoever stands between
    theirs = rec[owners == spawned[0]]
    aimed = rays_array(np.column_stack([theirs["x"] - 3.0, theirs["y"]]), np.repeat([[1.0, 0.0]], len(theirs), axis=0))
    want = agree(a, rec, grid, aimed, 0.2, of_sink, cols, "aimed at the agents of a source-sink")
    assert (want["id"] != NO_HIT).all() and set(want["id"].tolist()) <= set(theirs["id"].tolist())
    _, want, _ = check_query(a, rec, grid, 0.2, INF, "nobody", nobody, cols, want_classes=False)
    assert (want["id"] == NO_HIT).all() and np.isinf(want["t"]).all()
    # the Python surface: dicts and Selections
    rays = ray_sets(rec, grid, 3.0)
    o, u = np.column_stack([rays["ox"], rays["oy"]]), np.column_stack([rays["ux"], rays["uy"]])
    want = cast(rec, grid, rays, 0.2, roles(slow, None, rec, *cols)[0])
    assert a.cast_rays(o, u, 0.2, t_max=rays["t_max"], ignore=rays["ignore"], targets=dict(speed=(0.0, pace))).tobytes() == want.tobytes()
    assert a.count_ray_hits(o, u, 0.2, t_max=rays["t_max"], ignore=rays["ignore"], targets=Selection(speed=(0.0, pace))) == \
        int((want["id"] != NO_HIT).sum())
    assert a.read_agents().tobytes() == rec.tobytes()


def test_edges_to_the_bit():
    """For 40 sampled hits with t > 0: t_max at t and at its two f64 neighbours, radius at sqrt(cr * cr / uu) (where the
    winner grazes) and at its two neighbours.  The engine and the restatement agree whichever way each case falls (a fused
    multiply-add, a reciprocal or an f32 shortcut would not)."""
    a, led, _, grid = _scene()
    _advance(a, led, 40)
    rec = a.read_agents()
    radius = 0.2
    rays, base, stats = check_query(a, rec, grid, radius, 3.0, "the base query")
    inner = np.nonzero((base["id"] != NO_HIT) & (base["t"] > 0.0))[0]
    assert len(inner) >= 40
    rng = np.random.default_rng(19)
    fell = {True: 0, False: 0}
    for k in rng.choice(inner, 40, replace=False):
        t = base["t"][k]
        three = np.repeat(rays[k:k + 1], 3)
        three["t_max"] = [np.nextafter(t, 0.0), t, np.nextafter(t, INF)]
        want = agree(a, rec, grid, three, radius, name=f"ray {k}, t_max around {float(t).hex()}")
        assert want["id"][:2].tolist() == [NO_HIT, NO_HIT] and want[2].tobytes() == base[k].tobytes()  # (strict, then itself)
        fell[False] += 2
        fell[True] += 1
        with np.errstate(invalid="ignore"):
            graze = np.sqrt(stats["cr"][k] * stats["cr"][k] / stats["uu"][k])
        assert 0.0 <= graze <= radius
        one = rays[k:k + 1].copy()
        one["t_max"] = INF
        for r in (np.nextafter(graze, 0.0), graze, np.nextafter(graze, INF)):
            want = agree(a, rec, grid, one, float(r), name=f"ray {k}, radius {float(r).hex()}")
            fell[bool(want["id"][0] == base["id"][k])] += 1
    print(f"the sampled winner was hit {fell[True]} times and not {fell[False]} times")
    assert fell[True] >= 40 and fell[False] >= 40
    assert a.read_agents().tobytes() == rec.tobytes()


def test_degenerate_queries_far_origins_and_an_offset_grid():
    """A grid that is not square and does not start at 0 (30 rows of x from -3, 20 columns of y from 1.5), agents written
    up to its very edges and outside it; t_max == 0, radius == 0, a radius wider than the grid, +inf everywhere, origins
    so far away that the walk takes no clip at all, and directions at the ends of the admitted range."""
    grid = dict(width=40.0, height=60.0, cell_size=2.0, offset=(-3.0, 1.5))
    rng = np.random.default_rng(3)
    a = Simulation(LocationHash2D(**grid))
    assert a.cast_rays([(0.0, 5.0)], [(1.0, 0.0)], 0.5).tolist() == [(_abi.CS_NO_HIT, INF)]  # an empty crowd
    pts = np.column_stack([rng.uniform(-3.0, 57.0, 700), rng.uniform(1.5, 41.5, 700)])
    pts[:8] = [(-3.0, 1.5), (56.99, 41.49), (-3.0, 41.4), (56.9, 1.5), (-3.5, 20.0), (20.0, 43.0), (20.0, 1.0), (20.0, 41.5)]
    a.add_agents(pts, StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 2.0)
    a.step(0.05)
    rec = a.read_agents()
    part = takes_part(rec, grid)
    assert 690 <= part.sum() < 700  # (the outsiders are never hit)
    for reach in (0.0, 2.0, INF):
        rays = ray_sets(rec, grid, reach, seed=11, beams=90)
        for radius in (0.0, 0.15, 0.5, 7.0, 100.0, INF):
            want = agree(a, rec, grid, rays, radius, name=f"offset grid, radius {radius}, reach {reach}")
            if reach == 0.0 or radius == 0.0:
                assert (want["id"] == NO_HIT).all()
            assert not np.isin(want["id"], rec["id"][~part]).any()
    # far origins: beyond 2^32 cells, and merely far; towards the crowd and along an axis through it
    o, u = [], []
    for far in (1e5, 1e8, 1e10, 1e12, 1e300):
        for k in range(12):
            target = pts[20 + k]
            o += [(target[0] - far, target[1]), (target[0], target[1] + far), (target[0] - far, target[1] - far)]
            u += [(1.0, 0.0), (0.0, -1.0), (1.0, 1.0)]
    rays = rays_array(o, u)
    for radius in (0.3, 3.0):
        want = agree(a, rec, grid, rays, radius, name=f"far origins, radius {radius}")
    assert (want["id"][:36] != NO_HIT).sum() >= 24
    # directions at the ends of the admitted range, and a t_max that is +inf in every one of them
    o = pts[40:100]
    phi = rng.uniform(0.0, 2.0 * np.pi, len(o))
    unit = np.column_stack([np.cos(phi), np.sin(phi)])
    for length in (2.0 ** -49.5, 2.0 ** 49.5):
        rays = rays_array(o + 0.7 * unit, unit * length)
        want = agree(a, rec, grid, rays, 0.25, name=f"directions of length {length}")
        assert (want["id"] != NO_HIT).sum() >= 20
    assert a.read_agents().tobytes() == rec.tobytes()


def test_refusals():
    grid = dict(width=40.0, height=40.0, cell_size=2.0, offset=(0.0, 0.0))
    a = Simulation(LocationHash2D(**grid))
    a.add_agents([(3.0, 4.0), (8.0, 4.0), (30.0, 30.0)], StubHighLevelPlan((0.1, 0.0)), NoLocalPlan(), 2.0)
    a.step(0.05)
    rec = a.read_agents()
    good = rays_array([(1.0, 4.0)] * 6, [(1.0, 0.0)] * 6)
    usable = cast(rec, grid, good, 0.5)
    assert usable["id"].tolist() == [0] * 6 and agree(a, rec, grid, good, 0.5, name="three agents").tobytes() == usable.tobytes()
    nan = float("nan")

    def bad(field, value, k=3):
        rays = good.copy()
        rays[field][k] = value
        return rays

    bad_terms = selection(1 << 9)
    nan_rect = selection(_abi.CS_SEL_RECT, x0=nan, y0=0.0, x1=1.0, y1=1.0)
    zero = bad("ux", 0.0)
    cases = [("NaN radius", good, nan, None, None), ("negative radius", good, -0.5, None, None),
             ("too many rays", good, 0.5, None, _abi.CS_RAYS_MAX + 1),
             ("unknown terms", good, 0.5, bad_terms, None), ("a NaN in the selection", good, 0.5, nan_rect, None),
             ("a zero direction", zero, 0.5, None, None)]
    for field in ("ox", "oy", "ux", "uy"):
        cases += [(f"{field} {v}", bad(field, v), 0.5, None, None) for v in (nan, INF, -INF)]
    cases += [("a short direction", bad("ux", 2.0 ** -51), 0.5, None, None),
              ("a long direction", bad("ux", 2.0 ** 51), 0.5, None, None),
              ("NaN t_max", bad("t_max", nan), 0.5, None, None), ("negative t_max", bad("t_max", -1e-300), 0.5, None, None)]
    for name, rays, radius, sel, n in cases:
        for rows in (True, False):
            got, out = call(a, rays, radius, sel, rows=rows, fill=0xAB, n=n)
            assert got == SIZE_MAX and "cast_rays" in last_error(a), name
            if rows:
                assert (out.view(np.uint8) == 0xAB).all(), name
        if rays is not good:
            assert "ray 3" in last_error(a), (name, last_error(a))  # the first bad ray, by its index
        assert a.read_agents().tobytes() == rec.tobytes(), name
        assert call(a, good, 0.5)[1].tobytes() == usable.tobytes(), name
    two = bad("ux", nan, 5)
    two["t_max"][2] = -1.0
    assert call(a, two, 0.5)[0] == SIZE_MAX and "ray 2" in last_error(a)
    out = np.zeros(4, dtype=RAY_HIT_DTYPE)
    assert a._lib.cs_cast_rays(a._engine, None, 4, 0.5, None, out.ctypes.data_as(C.POINTER(_abi.RayHit))) == SIZE_MAX
    assert "cast_rays" in last_error(a) and not out.view(np.uint8).any()
    assert a._lib.cs_cast_rays(a._engine, None, 0, 0.5, None, None) == 0  # no rays: nothing to do
    short, long_ = bad("ux", 2.0 ** -50), bad("ux", 2.0 ** 50)  # (uu == 2^-100 and 2^100 are admitted)
    agree(a, rec, grid, short, 0.5, name="uu == 2^-100")
    agree(a, rec, grid, long_, 0.5, name="uu == 2^100")
    with pytest.raises(CrowdSimError, match="cast_rays"):
        a.cast_rays([(1.0, 4.0)], [(0.0, 0.0)], 0.5)
    with pytest.raises(CrowdSimError, match="cast_rays"):
        a.count_ray_hits([(1.0, 4.0)], [(1.0, 0.0)], 0.5, targets=dict(circle=(0.0, 0.0, -2.0)))
    assert a.read_agents().tobytes() == rec.tobytes()
    a.step(0.05)
    assert a.cast_rays([(1.0, 4.0)], [(1.0, 0.0)], 0.5)["id"].tolist() == [0]


def test_wide_ids_by_external_id(monkeypatch):
    """Ids above 2^32 come back, and `ignore` is taken in external ids, before and after a renumbering."""
    monkeypatch.setenv("CS_FIRST_AGENT_ID", str(2 ** 40 + 1))
    monkeypatch.setenv("CS_DEVICE_ID_LIMIT", "4096")
    pts, grid, extent, group = scenes.uniform_crowd(600, seed=9, cell_size=2.0, room=20.0)
    a = Simulation(LocationHash2D(**grid), flags=CS_CFG_WIDE_IDS)
    monkeypatch.delenv("CS_DEVICE_ID_LIMIT")
    monkeypatch.delenv("CS_FIRST_AGENT_ID")
    ids = scenes.add_counterflow(a, pts, group, scenes.CREEP_SPEED, Zanlungo(*scenes.METRIC_ZANLUNGO), 2.0)
    assert min(ids) > 2 ** 40
    spot = np.array([[extent + 15.0, extent + 15.0]])
    still, nolp = StubHighLevelPlan((0.0, 0.0)), NoLocalPlan()

    def check(when):
        rec = a.read_agents()
        rays = ray_sets(rec, grid, 4.0, beams=90)
        want = agree(a, rec, grid, rays, 0.2, name=when)
        hit = want["id"] != NO_HIT
        assert hit.sum() >= 90 and int(want["id"][hit].min()) > 2 ** 32
        fans = rays["ignore"] != _abi.CS_NO_HIT
        assert fans.sum() == 360 and (want["id"][fans] != rays["ignore"][fans]).all() and int(rays["ignore"][fans].min()) > 2 ** 32
        assert (want["t"][360:720] == 0.0).all() and (want["id"][360:720] <= rays["ignore"][:360]).all()  # (no ignore: the
        # caster itself, or one with a smaller id on the same spot)

    for r in range(6):
        more = a.add_agents(np.repeat(spot, 600, axis=0) + np.arange(600)[:, None] * 0.01, still, nolp, 1.0)
        a.step(0.05)
        if r in (0, 5):
            n_before = a.kernel_stat(_abi.CS_STAT_RENUMBERINGS)
            check(f"round {r}, {n_before} renumberings")
            assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) == n_before
        a.remove_agents_by_id(more[:-1])
    assert a.kernel_stat(_abi.CS_STAT_RENUMBERINGS) >= 1
    check("at the end")


@pytest.mark.parametrize("flags", [0, CS_CFG_FORCE_TILED])
def test_twins_one_of_which_asks_between_steps(flags):
    """One twin casts rays after every step from 20 to 30, the other never does: the same bytes, events and report."""
    twins = [_scene(flags, 4096, sinks=True) for _ in range(2)]
    (a, led_a, _, grid), (b, led_b, _, _) = twins
    for s, led, _, _ in twins:
        _advance(s, led, 20)
    rec = a.read_agents()
    assert rec.tobytes() == b.read_agents().tobytes()
    rays = ray_sets(rec, grid, 5.0, beams=90)
    o, u = np.column_stack([rays["ox"], rays["oy"]]), np.column_stack([rays["ux"], rays["uy"]])
    for _ in range(10):
        hits = a.count_ray_hits(o, u, 0.2, t_max=rays["t_max"], ignore=rays["ignore"])
        assert 0 < hits < len(rays)
        a.cast_rays(o, u, 0.3, targets=dict(source_sink=0))
        _steps((a, b), 1)
    assert a.read_agents().tobytes() == b.read_agents().tobytes()
    assert drain(a) == drain(b)
    assert a.last_report == b.last_report
