"""The scenes of the set_targets parity tests, each runnable on the engine (RouteFollower + Simulation.set_targets) and
as the REFERENCE: the oracle with a HostFollower (tests/host_follower.py) on which set_target is called agent by agent,
in batch order, with the agent as read_agents() shows it, as a reference host does (rmf/mod.rs:217-236)."""
import math

import numpy as np

from host_follower import HostFollower
from rmf_crowdsim_amd import (LocationHash2D, NoLocalPlan, RouteFollower, SeededPoissonCrowd, SourceSink, Zanlungo)
from rmf_crowdsim_amd.simulation import Agent
from test_oracle_reference_kats import DoglegRoutes, MockEventListener

EXITS = [(20.0, 20.0), (140.0, 20.0), (140.0, 140.0), (20.0, 140.0)]


class Host:
    """One side of a comparison: a simulation, its follower and a uniform `send(ids, goals)` -> statuses."""

    def __init__(self, sim_cls, reference, scale, arrive=0.1, speed=1.2, grid=(160.0, 160.0, 2.0, (0.0, 0.0)), **kw):
        self.routes = DoglegRoutes()
        self.reference = reference
        self.sim = sim_cls(LocationHash2D(*grid), **kw)
        self.hlp = (HostFollower if reference else RouteFollower)(self.routes, scale=scale, arrive=arrive, speed=speed)
        self.statuses = []  # of every entry sent so far, in order
        self.marks = []     # the length of the plan_route log after every batch

    def send(self, ids, goals):
        ids = [int(i) for i in ids]
        goals = np.asarray(goals, dtype=np.float64).reshape(-1, 2)
        if not self.reference:
            st = [int(s) for s in self.sim.set_targets(ids, goals)]
        else:
            arr = self.sim.read_agents()
            at = np.searchsorted(arr["id"], np.asarray(ids, dtype=np.uint64))
            assert (arr["id"][at] == np.asarray(ids, dtype=np.uint64)).all()
            first = len(self.hlp.statuses)
            for k, i in enumerate(ids):
                r = arr[at[k]]
                agent = Agent(i, np.array([r["x"], r["y"]]), np.array([r["vx"], r["vy"]]), int(r["next_waypoint"]),
                              float(r["eyesight_range"]))
                self.hlp.set_target(agent, goals[k], np.zeros(2))
            st = self.hlp.statuses[first:]
        self.statuses += st
        self.marks.append(len(self.routes.calls))
        return st

    def calls(self):
        """the plan_route log: (start, goal) pairs in call order"""
        return [(tuple(s), tuple(g)) for s, g in self.routes.calls]


def same_calls(got, want, goals_exact=True, within=5e-4):
    """Two plan_route logs name the same calls in the same order: starts to 3 decimals (f32 cell-relative positions on
    the device, f64 in the reference; compared by distance, since rounding both to 3 decimals splits values that
    straddle a rounding boundary), goals exactly unless they were derived from each side's own positions."""
    if len(got) != len(want):
        return False
    for (sa, ga), (sb, gb) in zip(got, want):
        if max(abs(sa[0] - sb[0]), abs(sa[1] - sb[1])) > within:
            return False
        if (ga != gb) if goals_exact else (max(abs(ga[0] - gb[0]), abs(ga[1] - gb[1])) > within):
            return False
    return True


def lattice(nx, ny, spacing, origin, jitter, seed):
    rng = np.random.default_rng(seed)
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    pts = np.stack([origin[0] + spacing * ix.ravel(), origin[1] + spacing * iy.ravel()], axis=1).astype(np.float64)
    if jitter:
        pts += rng.uniform(-jitter, jitter, pts.shape)
    return pts


def run_dispatch(sim_cls, reference, steps=180, side=40, **kw):
    """Dispatch, NoLocalPlan: side x side agents 1.6 m apart sent to four exits three times."""
    h = Host(sim_cls, reference, scale=4.0, **kw)
    ids = h.sim.add_agents(lattice(side, side, 1.6, (40.0, 40.0), 0.15, 5), h.hlp, NoLocalPlan(), 2.0)
    rng = np.random.default_rng(23)  # (the same draws on both sides)
    for step in range(steps):
        if step == 0:
            h.send(ids, [EXITS[i % 4] for i in ids])
        if step == 60:
            some = sorted(rng.choice(ids, (2 * len(ids)) // 3, replace=False).tolist())
            h.send(some, [EXITS[(i + 1) % 4] for i in some])
        if step == 120:
            some = rng.choice(ids, (2 * len(ids)) // 3, replace=False).tolist()  # (in a random order)
            h.send(some, [EXITS[int(e)] for e in rng.integers(0, 4, len(some))])
        h.sim.step(0.1)
    return h


def run_swirl(sim_cls, reference, side=32, steps=25, **kw):
    """Dispatch under Zanlungo: everybody walks a private dogleg to their own place turned by 60 degrees about the
    crowd's centre, two thirds turn back at step 12.  The same scene has its first NaN in the reference at step 39."""
    h = Host(sim_cls, reference, scale=0.5, **kw)
    half = 0.5 * 2.4 * (side - 1)
    pts = lattice(side, side, 2.4, (80.0 - half, 80.0 - half), 0.0, 0)
    ids = h.sim.add_agents(pts, h.hlp, Zanlungo(0.3, 1.0, 0.0, 0.4, 2.0, 0.2), 2.0)
    rng = np.random.default_rng(7)

    def turned(xy, deg):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        d = np.asarray(xy) - 80.0
        return np.stack([80.0 + c * d[:, 0] - s * d[:, 1], 80.0 + s * d[:, 0] + c * d[:, 1]], axis=1)

    for step in range(steps):
        if step == 0:
            h.send(ids, turned(pts, 60.0))
        if step == 12:
            some = sorted(rng.choice(ids, (2 * len(ids)) // 3, replace=False).tolist())
            # (goals from the lattice, not from the f32 / f64 positions: the same numbers on both sides)
            h.send(some, turned(pts[[ids.index(i) for i in some]], -60.0))
        h.sim.step(0.1)
    return h


def add_dogleg_stream(sim, hlp, lp, rate=1.5):
    """the 16-sink stream of test_route_follower_stream_matches_oracle"""
    for k in range(16):
        y = 20.0 + 7.5 * k
        left = k % 2 == 0
        src = (20.0, y) if left else (140.0, y)
        mid = (70.0, y + 3.0) if left else (90.0, y - 3.0)
        dst = (120.0, y) if left else (40.0, y)
        sim.add_source_sink(SourceSink(src, 1.0, SeededPoissonCrowd(rate, 40 + k), hlp, lp, [mid, dst], False, 2.0))


def run_stream(sim_cls, reference, steps=1000, resend=(50, 120, 500), follower=None, **kw):
    """Source-sink agents re-sent mid-leg: at the `resend` steps every third live agent goes 30 m on and 5 m aside;
    afterwards the sink's own set_target at its waypoint takes over.  `follower`: another planner class to run the same
    stream with (the pin of HostFollower against RouteFollower)."""
    h = Host(sim_cls, reference, scale=4.0, **kw)
    if follower is not None:
        h.hlp = follower(h.routes, scale=4.0, arrive=0.1, speed=1.2)
    h.listener = MockEventListener()
    h.sim.add_event_listener(h.listener)
    add_dogleg_stream(h.sim, h.hlp, NoLocalPlan())
    h.counts = []
    for step in range(steps):
        if step in resend:
            some = h.sim.read_agents()[::3]
            goals = np.stack([np.where(some["vx"] >= 0, some["x"] + 30.0, some["x"] - 30.0), some["y"] + 5.0], axis=1)
            h.send(some["id"], goals)
        h.sim.step(0.1)
        r = h.sim.last_report
        h.counts.append((len(h.sim), r["n_spawned"], r["n_destroyed"], r["n_waypoint_hits"]))
    return h
