"""Host-side mirror of the reference's trait surface for the `Simulation::step` path.

Same names and argument meaning as rmf_crowdsim (paths relative to
rmf_crowdsim/src in the reference tree):

    Simulation            lib.rs:69-383      new / add_agents / add_source_sink /
                                             remove_source_sink / add_event_listener /
                                             remove_agents / step / agents
    EventListener         lib.rs:22-33
    Agent                 lib.rs:46-65
    HighLevelPlanner      highlevel_planners/highlevel_planners.rs:8-16
    LocalPlanner          local_planners/local_planner.rs:7-18
    Zanlungo / NoLocalPlan  local_planners/zanlungo.rs:31-48, no_local_plan.rs:7-18
    LocationHash2D        spatial_index/location_hash_2d.rs:33-51
    SourceSink / CrowdGenerator / MonotonicCrowd   source_sink/source_sink.rs:30-101

Everything forwards to the C ABI (include/crowdstep.h) of the HIP engine; Rust
`Result<_, String>` becomes `CrowdSimError(message)`.
"""
import ctypes as C
import datetime
import weakref
from dataclasses import dataclass

import numpy as np

from . import _abi, _native


class CrowdSimError(RuntimeError):
    """`Err(String)` of the reference API ("Index out of bounds", ...)."""


@dataclass
class Agent:
    """pub struct Agent, lib.rs:46-65 (the fields `step` maintains)."""
    agent_id: int
    position: np.ndarray
    velocity: np.ndarray
    next_waypoint: int
    eyesight_range: float
    orientation: float = 0.0   # never written after creation (lib.rs:138)
    angular_vel: float = 0.0   # never written after creation (lib.rs:141)
    preferred_vel: object = None  # set on the clone a LocalPlanner sees (lib.rs:271); (0, 0) on its neighbours


# ---- spatial index ---------------------------------------------------------
class SpatialIndex:
    """trait SpatialIndex, spatial_index.rs:4-14: what `Simulation<T: SpatialIndex>` (lib.rs:69) is generic over.

    On this backend the index IS the neighbour kernel: the engine keeps the agents in the cell order of a
    `LocationHash2D` and answers `get_neighbours_in_radius` / `get_nearest_neighbours` / `add_or_update` /
    `remove_agent` itself (`Simulation.get_neighbours_in_radius`, `.get_nearest_neighbours`, the step's re-binning,
    `.remove_agents`).  An index therefore has to describe itself as such a grid: `device_form()` returns the
    `LocationHash2D` it is equivalent to (the one provided method this mirror adds to the trait, like the planners'), or
    None, in which case `Simulation(index)` refuses it with an error that says so.  There is no host-side slow path
    for a foreign index (unlike the planners: a per-agent host query per step would put the hot path on the CPU)."""

    def add_or_update(self, index, position):           # spatial_index.rs:6
        raise NotImplementedError

    def get_nearest_neighbours(self, n, position):       # spatial_index.rs:8
        raise NotImplementedError

    def get_neighbours_in_radius(self, radius, position):  # spatial_index.rs:10
        raise NotImplementedError

    def remove_agent(self, index):                       # spatial_index.rs:12
        raise NotImplementedError

    def device_form(self):
        return None


class LocationHash2D(SpatialIndex):
    """LocationHash2D::new(width, height, cell_size, offset); location_hash_2d.rs:33."""

    def device_form(self):
        return self

    def __init__(self, width, height, cell_size, offset):
        self.width = float(width)
        self.height = float(height)
        self.cell_size = float(cell_size)
        self.offset = (float(offset[0]), float(offset[1]))

    def _desc(self):
        return _abi.GridDesc(self.width, self.height, self.cell_size, *self.offset)


# ---- local planners --------------------------------------------------------
class LocalPlanner:
    """trait LocalPlanner, local_planner.rs:7-18.

    The two planners the reference ships (Zanlungo, NoLocalPlan) run on the device; they are passed
    as data.  Any other subclass is host code: override `get_desired_velocity`, and the engine
    evaluates it through the batched callback each step (cs_register_lp_callback: the slow path of
    SURVEY.md section 8b), with the agent and its neighbours as they were at the start of the step.
    """

    def get_desired_velocity(self, agent, nearby_agents, recommended_velocity):
        """-> (vx, vy).  `agent.preferred_vel` is the recommended velocity too (lib.rs:271); the
        neighbours' is (0, 0), as in the reference (lib.rs:140)."""
        raise NotImplementedError

    def add_agent(self, agent_id):       # local_planner.rs:14 (the reference never calls it: lib.rs:127-131 only
        pass                             # stores the planner per agent)

    def remove_agent(self, agent_id):    # local_planner.rs:16, called by remove_agents (lib.rs:181-184)
        pass

    _host_code = True  # the facade tells such a planner when one of its agents is removed

    def _register(self, lib, engine):
        if type(self).get_desired_velocity is LocalPlanner.get_desired_velocity:
            raise CrowdSimError("a LocalPlanner must be Zanlungo, NoLocalPlan or override get_desired_velocity")

        def batch(_user, n, agents, recommended, nb_begin, neighbours, out):
            def view(r, preferred):
                a = Agent(int(r.agent_id), np.array([r.x, r.y]), np.array([r.vx, r.vy]), int(r.next_waypoint),
                          float(r.eyesight_range))
                a.preferred_vel = preferred
                return a
            try:
                for k in range(n):
                    rec = np.array([recommended[2 * k], recommended[2 * k + 1]])
                    me = view(agents[k], rec)
                    nearby = [view(neighbours[q], np.zeros(2)) for q in range(nb_begin[k], nb_begin[k + 1])]
                    vx, vy = self.get_desired_velocity(me, nearby, rec)
                    out[2 * k], out[2 * k + 1] = float(vx), float(vy)
            except Exception as err:  # noqa: BLE001 (an exception must not cross the C frame: the step fails instead)
                self.failure = err
                return 1
            return 0

        fn = _abi.LpBatchFn(batch)
        # one thunk per engine this planner is registered with; the engines hold the raw pointer
        self._keepalive = getattr(self, "_keepalive", []) + [fn]
        handle = lib.cs_register_lp_callback(engine, fn, None)
        if handle == 0xFFFFFFFF:
            raise CrowdSimError(lib.cs_last_error(engine).decode())
        return handle


class NoLocalPlan(LocalPlanner):
    """no_local_plan.rs:7-18: returns the recommended velocity unchanged."""
    _host_code = False

    def _register(self, lib, engine):
        return lib.cs_register_no_local_plan(engine)


class Zanlungo(LocalPlanner):
    """Zanlungo::new(agent_scale, obstacle_scale, reaction_time, force_distance,
    agent_mass, agent_radius); zanlungo.rs:31-48."""

    _host_code = False

    def __init__(self, agent_scale, obstacle_scale, reaction_time, force_distance, agent_mass,
                 agent_radius):
        self.params = _abi.ZanlungoParams(agent_scale, obstacle_scale, reaction_time,
                                          force_distance, agent_mass, agent_radius)

    def _register(self, lib, engine):
        return lib.cs_register_zanlungo(engine, C.byref(self.params))


# ---- high-level planners ---------------------------------------------------
class HighLevelPlanner:
    """trait HighLevelPlanner, highlevel_planners.rs:8-16.

    Subclass and override `get_desired_velocity` for a host planner (evaluated
    through the batched callback each step: the slow path), or use the data
    planners below, which the device evaluates itself.
    """

    def get_desired_velocity(self, agent, time):
        """-> (vx, vy) or None"""
        return None

    def set_target(self, agent, point, tolerance):
        pass

    def remove_agent_id(self, agent_id):
        pass

    # -- ABI plumbing --
    def _desc(self):
        keep = []

        def velocity(_user, n, ids, pos, vel, time_s, out, some):
            for i in range(n):
                agent = Agent(int(ids[i]), np.array([pos[2 * i], pos[2 * i + 1]]),
                              np.array([vel[2 * i], vel[2 * i + 1]]), 0, 0.0)
                res = self.get_desired_velocity(agent, datetime.timedelta(seconds=time_s))
                if res is None:
                    some[i] = 0
                else:
                    some[i] = 1
                    out[2 * i], out[2 * i + 1] = float(res[0]), float(res[1])

        def set_target(_user, aid, px, py, tx, ty, tolx, toly):
            agent = Agent(int(aid), np.array([px, py]), np.zeros(2), 0, 0.0)
            self.set_target(agent, np.array([tx, ty]), np.array([tolx, toly]))

        def remove(_user, aid):
            self.remove_agent_id(int(aid))

        fv, fs, fr = _abi.HlpVelocityFn(velocity), _abi.HlpSetTargetFn(set_target), \
            _abi.HlpRemoveFn(remove)
        keep += [fv, fs, fr]
        return _abi.HlpDesc(_abi.CS_HLP_CALLBACK, 0.0, 0.0, fv, fs, fr, None, _abi.RoutePlanFn(),
                            0.0, 0.0, 0.0), keep

    def _register(self, lib, engine):
        desc, keep = self._desc()
        # one set of callback thunks per engine this planner is registered with (a tile mesh
        # registers it with every tile); the engines hold the raw pointers
        self._keepalive = getattr(self, "_keepalive", []) + list(keep)
        return lib.cs_register_hlp(engine, C.byref(desc))


class _DataPlan(HighLevelPlanner):
    _kind = _abi.CS_HLP_NONE

    def __init__(self, default_vel=(0.0, 0.0)):
        self.default_vel = (float(default_vel[0]), float(default_vel[1]))

    def _desc(self):
        return _abi.HlpDesc(self._kind, self.default_vel[0], self.default_vel[1],
                            _abi.HlpVelocityFn(), _abi.HlpSetTargetFn(), _abi.HlpRemoveFn(),
                            None, _abi.RoutePlanFn(), 0.0, 0.0, 0.0), []


class NoHighLevelPlan(_DataPlan):
    """get_desired_velocity -> None for every agent (lib.rs:263-273 leaves vel = 0)."""
    _kind = _abi.CS_HLP_NONE


class StubHighLevelPlan(_DataPlan):
    """The reference tests' stub: Some(default_vel) for every agent (lib.rs:391-420)."""
    _kind = _abi.CS_HLP_CONSTANT

    def get_desired_velocity(self, agent, time):
        return self.default_vel


class IdParityHighLevelPlan(_DataPlan):
    """The visualiser's stub: even ids get -default_vel, odd ids +default_vel
    (rmf_crowdsim_viz/src/main.rs:20-30)."""
    _kind = _abi.CS_HLP_ID_PARITY

    def get_desired_velocity(self, agent, time):
        s = -1.0 if agent.agent_id % 2 == 0 else 1.0
        return (s * self.default_vel[0], s * self.default_vel[1])


class RouteFollower(HighLevelPlanner):
    """The follower half of RMFPlanner (rmf/mod.rs:195-242) with the route search left to the
    host: `plan_route(start, goal)` returns the waypoints of a route (the goal last) or None,
    the way RMFPlanner::plan_route does with A* over its visibility graph (rmf/mod.rs:160-192).
    It is called once per set_target whose (start, goal) SpatialHash pair is new
    (route_plans_by_location, rmf/mod.rs:217-236); following the route, that is
    get_desired_velocity (unit vector to the current waypoint, next waypoint inside 0.1,
    rmf/mod.rs:197-215), runs on the device for every agent every step.
    """

    def __init__(self, plan_route, scale=1.0, arrive=0.1, speed=1.0):
        self.plan_route = plan_route
        self.scale, self.arrive, self.speed = float(scale), float(arrive), float(speed)
        self._hosts = []  # weak references to the simulations and meshes this planner is registered with

    def _registered_with(self, host):
        """Called by a Simulation or a NativeTileMesh that has registered this planner with its engine."""
        hosts = self.__dict__.setdefault("_hosts", [])  # (a subclass may have skipped __init__)
        if not any(h() is host for h in hosts):
            hosts.append(weakref.ref(host))

    def set_target(self, agent, point, tolerance=(0.0, 0.0)):
        """RMFPlanner::set_target (rmf/mod.rs:217-236) as a host calls it: forwards `agent.agent_id` to set_targets of the
        one simulation or mesh this planner is registered with.  Returns that entry's _abi.CS_TARGET_* status."""
        hosts = [h() for h in getattr(self, "_hosts", []) if h() is not None]
        if len(hosts) != 1:
            raise CrowdSimError(
                f"RouteFollower.set_target: the planner is registered with {len(hosts)} simulations; it forwards to "
                "Simulation.set_targets (or NativeTileMesh.set_targets) of exactly one: call that directly")
        return int(hosts[0].set_targets([int(agent.agent_id)], [point], tolerance)[0])

    def _desc(self):
        def plan(_user, sx, sy, gx, gy, out, cap):
            pts = self.plan_route((sx, sy), (gx, gy))
            if not pts:
                return 0
            n = min(len(pts), int(cap))
            for k in range(n):
                out[2 * k], out[2 * k + 1] = float(pts[k][0]), float(pts[k][1])
            return n

        fp = _abi.RoutePlanFn(plan)
        return _abi.HlpDesc(_abi.CS_HLP_ROUTE, 0.0, 0.0, _abi.HlpVelocityFn(), _abi.HlpSetTargetFn(),
                            _abi.HlpRemoveFn(), None, fp, self.scale, self.arrive, self.speed), [fp]


def field_velocity(origin, cell, vectors, bilinear, x, y):
    """The rule of cs_register_hlp_field (include/crowdstep_state.h, "Flow-field high-level planner") for one agent at
    (x, y), in numpy f64 with exactly those operations, each rounded once.  vectors: float32 (ny, nx, 2).  -> (vx, vy) as
    Python floats that hold f32 values, or None."""
    f64 = np.float64
    ny, nx = vectors.shape[0], vectors.shape[1]
    with np.errstate(all="ignore"):
        fx = (f64(x) - f64(origin[0])) / f64(cell[0])
        fy = (f64(y) - f64(origin[1])) / f64(cell[1])
        if not (0.0 <= fx and fx < f64(nx) and 0.0 <= fy and fy < f64(ny)):
            return None
        ix, iy = int(fx), int(fy)

        def nearest():
            s = vectors[iy, ix]
            if np.isnan(s[0]) or np.isnan(s[1]):
                return None
            return float(s[0]), float(s[1])

        if not bilinear:
            return nearest()

        def axis(f, n):
            a = f - f64(0.5)
            if a < 0.0:
                return 0, 0, f64(0.0)
            i0 = int(a)
            return i0, min(i0 + 1, n - 1), a - f64(i0)

        i0, i1, tx = axis(fx, nx)
        j0, j1, ty = axis(fy, ny)
        c00, c10 = vectors[j0, i0].astype(f64), vectors[j0, i1].astype(f64)
        c01, c11 = vectors[j1, i0].astype(f64), vectors[j1, i1].astype(f64)
        if np.isnan(c00).any() or np.isnan(c10).any() or np.isnan(c01).any() or np.isnan(c11).any():
            return nearest()
        out = []
        for k in (0, 1):
            a = c00[k] + (c10[k] - c00[k]) * tx
            b = c01[k] + (c11[k] - c01[k]) * tx
            out.append(float(np.float32(a + (b - a) * ty)))
        return out[0], out[1]


class FieldPlanner(HighLevelPlanner):
    """A navigation (flow) field: a raster of preferred velocities sampled at the agent's position, on the device
    (cs_register_hlp_field: no host call, no wait in a step).  origin: (x0, y0) of bin (0, 0); cell: a bin size, a scalar
    or (w, h); vectors: (ny, nx, 2) preferred velocities, stored as f32; sampling: "nearest" (the agent's own bin) or
    "bilinear" (between the four nearest bin centres, clamped at the edges).  A NaN bin is a wall: None under "nearest",
    and "bilinear" falls back to the agent's own bin next to one.  Outside the raster: None.  The field takes no
    targets.

    `get_desired_velocity` is the same rule in numpy f64, so on a library without the call (the test oracle) the planner
    registers as a plain host planner, and `as_host_planner()` does so everywhere: the comparison the device path is
    checked against bit for bit."""

    def __init__(self, origin, cell, vectors, sampling="nearest"):
        if sampling not in ("nearest", "bilinear"):
            raise CrowdSimError('FieldPlanner: sampling is "nearest" or "bilinear"')
        self.origin = (float(origin[0]), float(origin[1]))
        cell = np.asarray(cell, dtype=np.float64).reshape(-1)
        if len(cell) not in (1, 2):
            raise CrowdSimError("FieldPlanner: cell is a scalar or a pair (w, h)")
        self.cell = (float(cell[0]), float(cell[-1]))
        self.sampling = sampling
        self.vectors = self._checked(vectors, None)
        self._bound = []  # (lib or mesh registrar, engine or mesh, planner handle) of every device registration
        self._sims = []   # the simulations and meshes it is registered with (solve)

    @staticmethod
    def _checked(vectors, shape):
        v = np.ascontiguousarray(np.asarray(vectors, dtype=np.float32))
        if v.ndim != 3 or v.shape[2] != 2 or (shape is not None and v.shape != shape):
            raise CrowdSimError("FieldPlanner: vectors has shape (ny, nx, 2)" + (" of the registered raster" if shape else ""))
        return v.copy()

    def update(self, vectors):
        """New values for the same raster.  Steps already queued use the old ones; nothing waits for the device."""
        self.vectors = self._checked(vectors, self.vectors.shape)
        for lib, engine, handle in self._bound:
            if lib.cs_hlp_field_update(engine, handle, self.vectors.ctypes.data_as(C.POINTER(C.c_float))) != 0:
                raise CrowdSimError(lib.cs_last_error(engine).decode())

    def _registered_with(self, sim):
        self._sims.append(sim)

    def solve(self, goals, speed, **how):
        """Solve the flow field to `goals` on the device and write it into this planner, in every simulation it is
        registered with (Simulation.solve_flow_field with planner=self, whose keywords `how` are).  Steps already queued
        use the old values.  -> (vectors | None, dist | None, stats) of the last of them."""
        if not self._sims:
            raise CrowdSimError("FieldPlanner.solve: the planner is registered with no simulation yet")
        out = None
        for sim in self._sims:
            out = sim.solve_flow_field(self.origin, self.cell, goals, speed, planner=self, **how)
        return out

    def get_desired_velocity(self, agent, time):
        return field_velocity(self.origin, self.cell, self.vectors, self.sampling == "bilinear", agent.position[0],
                              agent.position[1])

    def as_host_planner(self):
        """The same field as a planner that always takes the host callback path (it follows `update`)."""
        return _HostFieldPlanner(self)

    def _register(self, lib, engine):
        try:
            register = lib.cs_register_hlp_field
        except AttributeError:  # a library without the call: the plain callback descriptor
            return HighLevelPlanner._register(self, lib, engine)
        desc = field_desc(self.origin, self.cell, self.vectors.shape[:2])
        sampling = _abi.CS_HLP_FIELD_BILINEAR if self.sampling == "bilinear" else _abi.CS_HLP_FIELD_NEAREST
        handle = register(engine, C.byref(desc), sampling, self.vectors.ctypes.data_as(C.POINTER(C.c_float)))
        if handle != 0xFFFFFFFF:
            self._bound.append((lib, engine, handle))
        return handle


class _HostFieldPlanner(HighLevelPlanner):
    def __init__(self, field):
        self.field = field

    def get_desired_velocity(self, agent, time):
        return self.field.get_desired_velocity(agent, time)


# ---- source / sink ---------------------------------------------------------
class CrowdGenerator:
    """trait CrowdGenerator, source_sink.rs:30-33."""

    def get_number_to_spawn(self, time_elapsed):
        return 0

    def _fill(self, desc):
        def gen(_user, dt):
            return int(self.get_number_to_spawn(datetime.timedelta(seconds=dt)))
        fn = _abi.GeneratorFn(gen)
        desc.generator_kind = _abi.CS_GEN_CALLBACK
        desc.generator = fn
        return [fn]


class MonotonicCrowd(CrowdGenerator):
    """MonotonicCrowd::new(rate): round(dt * rate) per step; source_sink.rs:85-101."""

    def __init__(self, rate):
        self.rate = float(rate)

    def get_number_to_spawn(self, time_elapsed):
        v = time_elapsed.total_seconds() * self.rate
        return max(0, int(np.floor(abs(v) + 0.5) * np.sign(v)))

    def _fill(self, desc):
        desc.generator_kind = _abi.CS_GEN_MONOTONIC
        desc.rate = self.rate
        return []


class PoissonCrowd(CrowdGenerator):
    """PoissonCrowd::new(rate), source_sink.rs:63-82: Poisson(dt * rate) drawn from an UNSEEDED generator on every
    call (the reference's `thread_rng`), so two runs differ, as they do in the reference; asked on the host through the
    CrowdGenerator callback (a tile mesh refuses it: its tiles must draw alike).  SeededPoissonCrowd is the
    reproducible form."""

    def __init__(self, rate):
        self.rate = float(rate)
        self._rng = np.random.default_rng()  # OS entropy: unseeded like thread_rng

    def get_number_to_spawn(self, time_elapsed):
        rt = time_elapsed.total_seconds() * self.rate
        if not rt > 0.0:  # statrs' Poisson::new(lambda <= 0 or NaN) is an Err that the reference unwraps: a panic
            raise ValueError("PoissonCrowd: dt * rate must be positive (Poisson::new(rt).unwrap(), source_sink.rs:79)")
        return int(self._rng.poisson(rt))


class SeededPoissonCrowd(CrowdGenerator):
    """Seeded replacement for PoissonCrowd (source_sink.rs:63-82, whose
    thread_rng cannot be seeded): Poisson(dt * rate) from a counter-based
    generator keyed by (seed, step index)."""

    def __init__(self, rate, seed):
        self.rate = float(rate)
        self.seed = int(seed)

    def _fill(self, desc):
        desc.generator_kind = _abi.CS_GEN_POISSON_SEEDED
        desc.rate = self.rate
        desc.seed = self.seed
        return []


@dataclass
class SourceSink:
    """struct SourceSink, source_sink.rs:36-60."""
    source: tuple
    radius_sink: float
    crowd_generator: CrowdGenerator
    high_level_planner: HighLevelPlanner
    local_planner: LocalPlanner
    waypoints: list
    loop_forever: bool
    agent_eyesight_range: float


# ---- listeners -------------------------------------------------------------
class EventListener:
    """trait EventListener, lib.rs:22-33."""

    def agent_spawned(self, position, agent):
        pass

    def agent_destroyed(self, agent):
        pass

    def waypoint_reached(self, position, agent):
        """Declared by the reference, never called (lib.rs:32)."""


# ---- the simulation --------------------------------------------------------
def source_sink_desc(source_sink, handle_of):
    """cs_source_sink_desc of a SourceSink (source_sink.rs:36-60); handle_of(planner) -> its handle with the engine
    (or mesh) the sink is being added to.  Returns (desc, what must stay alive while the sink does)."""
    wps = np.ascontiguousarray(np.asarray(source_sink.waypoints, dtype=np.float64).reshape(-1, 2))
    desc = _abi.SourceSinkDesc()
    desc.source_x, desc.source_y = float(source_sink.source[0]), float(source_sink.source[1])
    desc.radius_sink = float(source_sink.radius_sink)
    keep = [source_sink.crowd_generator._fill(desc), wps]
    desc.hlp = handle_of(source_sink.high_level_planner)
    desc.lp = handle_of(source_sink.local_planner)
    desc.waypoints_xy = wps.ctypes.data_as(C.POINTER(C.c_double))
    desc.n_waypoints = wps.shape[0]
    desc.loop_forever = 1 if source_sink.loop_forever else 0
    desc.agent_eyesight_range = float(source_sink.agent_eyesight_range)
    return desc, keep


AGENT_DTYPE = np.dtype([("id", "<u8"), ("x", "<f8"), ("y", "<f8"), ("vx", "<f8"), ("vy", "<f8"),
                        ("next_waypoint", "<u8"), ("eyesight_range", "<f8")])

# the fields write_agents sets (include/crowdstep_state.h); eyesight_range, orientation and angular_vel are not writable
WRITE_FIELDS = {"position": _abi.CS_WRITE_POSITION, "velocity": _abi.CS_WRITE_VELOCITY,
                "next_waypoint": _abi.CS_WRITE_NEXT_WAYPOINT}


def write_mask(fields):
    """CS_WRITE_* bits of `fields`: an int mask, one name of WRITE_FIELDS or several."""
    if isinstance(fields, (int, np.integer)):
        return int(fields)
    if isinstance(fields, str):
        fields = (fields,)
    mask = 0
    for name in fields:
        if name not in WRITE_FIELDS:
            raise CrowdSimError(f"write_agents: {name!r} is not writable (writable: {', '.join(WRITE_FIELDS)})")
        mask |= WRITE_FIELDS[name]
    return mask


def write_records(records):
    """`records` as a contiguous AGENT_DTYPE array (the structured array read_agents returns, or any with its names)."""
    arr = np.asarray(records)
    if arr.dtype != AGENT_DTYPE:
        if arr.dtype.names is None or "id" not in arr.dtype.names:
            raise CrowdSimError("write_agents takes the structured array read_agents returns (AGENT_DTYPE)")
        out = np.zeros(arr.shape, dtype=AGENT_DTYPE)
        for name in AGENT_DTYPE.names:
            if name in arr.dtype.names:
                out[name] = arr[name]
        arr = out
    return np.ascontiguousarray(arr.reshape(-1))


def id_batch(ids):
    """`ids` as a contiguous uint64 array (agent ids, in the order given)."""
    arr = np.asarray(ids)
    if arr.size and arr.dtype.kind not in "ui":
        raise CrowdSimError("agent ids must be integers")
    if arr.size and arr.dtype.kind == "i" and (arr < 0).any():
        raise CrowdSimError("agent ids must not be negative")
    return np.ascontiguousarray(arr.reshape(-1), dtype=np.uint64)


def state_fn(lib, backend, symbol, what):
    """An entry point of include/crowdstep_state.h, or the error of a library without that header (the oracle)."""
    fn = getattr(lib, symbol, None)
    if fn is None:
        raise CrowdSimError(f"{what} needs the HIP engine: the {backend} library does not implement "
                            "include/crowdstep_state.h")
    return fn


def read_by_id(fn, handle, ids, missing_ok):
    """cs_read_agents_by_id / cs_mesh_read_agents_by_id -> (rc, records, found mask or None)"""
    keys = id_batch(ids)
    out = np.zeros(len(keys), dtype=AGENT_DTYPE)
    found = np.zeros(len(keys), dtype=np.uint8) if missing_ok else None
    rc = fn(handle, keys.ctypes.data_as(C.POINTER(C.c_uint64)), len(keys), out.ctypes.data_as(C.POINTER(_abi.AgentView)),
            found.ctypes.data_as(C.POINTER(C.c_uint8)) if missing_ok else None)
    return rc, out, (found.astype(bool) if missing_ok else None)


def set_targets_by_id(fn, handle, ids, goals, tolerance):
    """cs_set_targets / cs_mesh_set_targets -> (rc, status array: one _abi.CS_TARGET_* byte per entry)"""
    keys = id_batch(ids)
    xy = np.ascontiguousarray(np.asarray(goals, dtype=np.float64).reshape(-1, 2))
    if len(xy) != len(keys):
        raise CrowdSimError(f"set_targets: {len(keys)} ids but {len(xy)} goals")
    tol = np.asarray(tolerance, dtype=np.float64).reshape(2)
    status = np.zeros(len(keys), dtype=np.uint8)
    rc = fn(handle, keys.ctypes.data_as(C.POINTER(C.c_uint64)), xy.ctypes.data_as(C.POINTER(C.c_double)), len(keys),
            float(tol[0]), float(tol[1]), status.ctypes.data_as(C.POINTER(C.c_uint8)))
    return rc, status


NO_SOURCE_SINK = 0xFFFFFFFF  # Selection(source_sink=NO_SOURCE_SINK): the agents no sink spawned (add_agents)
_NO_HANDLE = 0xFFFFFFFE      # a planner the engine has never seen: it selects nobody


class Selection:
    """A condition on agents, an AND of the terms given (include/crowdstep_state.h, cs_selection); no term: every agent.
        rect=(x0, y0, x1, y1)       x0 <= x < x1 and y0 <= y < y1
        circle=(cx, cy, r)          (x-cx)*(x-cx) + (y-cy)*(y-cy) < r*r
        source_sink=handle          spawned by that source-sink, removed or not; NO_SOURCE_SINK: by none (add_agents)
        high_level_planner=, local_planner=    the planner object the agents were added with (or its integer handle)
        waypoint=(lo, hi) or k      lo <= next_waypoint <= hi
        speed=(lo, hi)              lo*lo <= vx*vx + vy*vy < hi*hi
    Every term is judged on the record read_agents() returns for the agent, in f64."""
    __slots__ = ("rect", "circle", "source_sink", "high_level_planner", "local_planner", "waypoint", "speed")

    def __init__(self, rect=None, circle=None, source_sink=None, high_level_planner=None, local_planner=None,
                 waypoint=None, speed=None):
        self.rect, self.circle, self.source_sink = rect, circle, source_sink
        self.high_level_planner, self.local_planner = high_level_planner, local_planner
        self.waypoint, self.speed = waypoint, speed

    def struct(self, handle_of=None):
        """The cs_selection of this condition.  handle_of(planner) -> the engine's handle of a planner object, or None
        if it was never registered there."""
        sel = _abi.Selection()

        def planner(p):
            if isinstance(p, (int, np.integer)):
                return int(p)
            h = handle_of(p) if handle_of is not None else None
            return _NO_HANDLE if h is None else int(h)
        if self.rect is not None:
            sel.terms |= _abi.CS_SEL_RECT
            sel.x0, sel.y0, sel.x1, sel.y1 = (float(v) for v in self.rect)
        if self.circle is not None:
            sel.terms |= _abi.CS_SEL_CIRCLE
            sel.cx, sel.cy, sel.r = (float(v) for v in self.circle)
        if self.source_sink is not None:
            sel.terms |= _abi.CS_SEL_SOURCE_SINK
            sel.source_sink = int(self.source_sink)
        if self.high_level_planner is not None:
            sel.terms |= _abi.CS_SEL_HLP
            sel.hlp = planner(self.high_level_planner)
        if self.local_planner is not None:
            sel.terms |= _abi.CS_SEL_LP
            sel.lp = planner(self.local_planner)
        if self.waypoint is not None:
            sel.terms |= _abi.CS_SEL_WAYPOINT
            lo, hi = (self.waypoint, self.waypoint) if isinstance(self.waypoint, (int, np.integer)) else self.waypoint
            lo, hi = max(int(lo), 0), int(hi)
            sel.wp_lo, sel.wp_hi = (lo, hi) if hi >= 0 else (1, 0)  # (a negative upper bound: nobody)
        if self.speed is not None:
            sel.terms |= _abi.CS_SEL_SPEED
            sel.speed_lo, sel.speed_hi = (float(v) for v in self.speed)
        return sel


def selection_struct(selection, handle_of):
    """A Selection, a dict of its keywords or a ready _abi.Selection -> _abi.Selection"""
    if isinstance(selection, _abi.Selection):
        return selection
    if isinstance(selection, dict):
        selection = Selection(**selection)
    if not isinstance(selection, Selection):
        raise CrowdSimError("a selection is a Selection, a dict of its keywords or an _abi.Selection")
    return selection.struct(handle_of)


_SIZE_MAX = C.c_size_t(-1).value


def select_ids(fn, handle, sel, cap):
    """cs_select_agents / cs_remove_selected and their mesh forms, with room for `cap` ids -> (the full count, or None on
    error; the first min(count, cap) ids as a uint64 array)"""
    cap = max(int(cap), 0)
    out = np.empty(max(cap, 1), dtype=np.uint64)
    got = fn(handle, C.byref(sel), out.ctypes.data_as(C.POINTER(C.c_uint64)), cap)
    if got == _SIZE_MAX:
        return None, np.zeros(0, dtype=np.uint64)
    return got, out[:min(got, cap)].copy()


def count_selected(fn, handle, selections, handle_of):
    """cs_count_agents / cs_mesh_count_agents -> (rc, uint64 counts)"""
    structs = [selection_struct(s, handle_of) for s in selections]
    arr = (_abi.Selection * max(len(structs), 1))(*structs)
    out = np.zeros(len(structs), dtype=np.uint64)
    rc = fn(handle, arr, len(structs), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, out


def field_desc(origin, cell, shape):
    """(x0, y0), a bin size (a scalar or a pair (w, h)) and (ny, nx) -> _abi.FieldDesc"""
    d = _abi.FieldDesc()
    d.x0, d.y0 = (float(v) for v in origin)
    cell = np.asarray(cell, dtype=np.float64).reshape(-1)
    if len(cell) not in (1, 2):
        raise CrowdSimError("agent_field: cell is a scalar or a pair (w, h)")
    d.cell_w, d.cell_h = float(cell[0]), float(cell[-1])
    ny, nx = (int(v) for v in shape)
    if not (0 <= nx < 2 ** 32 and 0 <= ny < 2 ** 32):
        raise CrowdSimError("agent_field: shape is (ny, nx), each below 2^32")
    d.nx, d.ny = nx, ny
    return d


def field_raster(fn, handle, desc, sel, velocity):
    """cs_agent_field / cs_mesh_agent_field -> (rc, uint32[ny, nx] counts, float64[ny, nx, 2] sums or None); `sel`: an
    _abi.Selection or None (every agent)"""
    bins = int(desc.nx) * int(desc.ny)
    if not 1 <= bins <= _abi.CS_FIELD_MAX_CELLS:
        bins = 1  # (the call refuses such a raster before it touches an output)
    count = np.zeros(bins, dtype=np.uint32)
    vx = np.zeros(bins, dtype=np.float64) if velocity else None
    vy = np.zeros(bins, dtype=np.float64) if velocity else None
    dbl = C.POINTER(C.c_double)
    rc = fn(handle, C.byref(desc), C.byref(sel) if sel is not None else None, count.ctypes.data_as(C.POINTER(C.c_uint32)),
            vx.ctypes.data_as(dbl) if velocity else None, vy.ctypes.data_as(dbl) if velocity else None)
    if rc != 0:
        return rc, None, None
    shape = (int(desc.ny), int(desc.nx))
    return rc, count.reshape(shape), np.stack([vx.reshape(shape), vy.reshape(shape)], axis=-1) if velocity else None


def close_pairs_call(fn, handle, distance, sel_a, sel_b, cap, distances):
    """cs_close_pairs / cs_mesh_close_pairs with room for `cap` pairs -> (the full count, or None on error; uint64[n, 2]
    pairs; float64[n] squared distances or None).  sel_a / sel_b: an _abi.Selection or None (everyone); cap == 0: the
    count only."""
    cap = max(int(cap), 0)
    pairs = np.zeros((max(cap, 1), 2), dtype=np.uint64)
    d2 = np.zeros(max(cap, 1), dtype=np.float64) if (distances and cap) else None
    got = fn(handle, float(distance), C.byref(sel_a) if sel_a is not None else None,
             C.byref(sel_b) if sel_b is not None else None,
             pairs.ctypes.data_as(C.POINTER(_abi.IdPair)) if cap else None,
             d2.ctypes.data_as(C.POINTER(C.c_double)) if d2 is not None else None, cap)
    if got == _SIZE_MAX:
        return None, np.zeros((0, 2), dtype=np.uint64), None
    n = min(got, cap)
    return got, pairs[:n].copy(), (d2[:n].copy() if d2 is not None else (np.zeros(0) if distances else None))


def close_pairs_of(fn, handle, handle_of, err, distance, a, b, limit, distances):
    """close_pairs of Simulation and NativeTileMesh: limit=None lists every pair (one counting call first)"""
    sel_a = None if a is None else selection_struct(a, handle_of)
    sel_b = None if b is None else selection_struct(b, handle_of)
    if limit is None:
        limit, _, _ = close_pairs_call(fn, handle, distance, sel_a, sel_b, 0, False)
        if limit is None:
            raise err()
        if limit > _abi.CS_PAIRS_MAX:
            limit = 1  # (the listing is refused by the library, with its message: no room is made for it here)
    n, pairs, d2 = close_pairs_call(fn, handle, distance, sel_a, sel_b, limit, distances)
    if n is None:
        raise err()
    return (pairs, d2) if distances else pairs


CLUSTER_DTYPE = np.dtype([("label", np.uint64), ("size", np.uint64), ("min_x", np.float64), ("min_y", np.float64),
                          ("max_x", np.float64), ("max_y", np.float64), ("sum_x", np.float64), ("sum_y", np.float64)])
assert CLUSTER_DTYPE.itemsize == C.sizeof(_abi.Cluster)


def agent_clusters_call(fn, handle, distance, sel, min_size, agent_cap, cluster_cap):
    """cs_agent_clusters / cs_mesh_agent_clusters with room for `agent_cap` members and `cluster_cap` clusters -> (rc,
    n_agents, n_clusters, uint64 ids, uint64 labels, CLUSTER_DTYPE table).  sel: an _abi.Selection or None (everyone); a
    cap of 0: that list is not asked for."""
    agent_cap, cluster_cap = max(int(agent_cap), 0), max(int(cluster_cap), 0)
    ids = np.zeros(max(agent_cap, 1), dtype=np.uint64)
    labels = np.zeros(max(agent_cap, 1), dtype=np.uint64)
    table = np.zeros(max(cluster_cap, 1), dtype=CLUSTER_DTYPE)
    n_agents, n_clusters = C.c_size_t(0), C.c_size_t(0)
    u64 = C.POINTER(C.c_uint64)
    rc = fn(handle, float(distance), C.byref(sel) if sel is not None else None, int(min_size),
            ids.ctypes.data_as(u64) if agent_cap else None, labels.ctypes.data_as(u64) if agent_cap else None, agent_cap,
            C.byref(n_agents), table.ctypes.data_as(C.POINTER(_abi.Cluster)) if cluster_cap else None, cluster_cap,
            C.byref(n_clusters))
    if rc != 0:
        return rc, 0, 0, ids[:0].copy(), labels[:0].copy(), table[:0].copy()
    na, nc = min(n_agents.value, agent_cap), min(n_clusters.value, cluster_cap)
    return rc, n_agents.value, n_clusters.value, ids[:na].copy(), labels[:na].copy(), table[:nc].copy()


def agent_clusters_of(fn, handle, handle_of, err, distance, members, min_size, limit):
    """agent_clusters of Simulation and NativeTileMesh: limit=None lists everything (one counting call first)"""
    if int(min_size) < 0:
        raise CrowdSimError("agent_clusters: min_size is negative")
    sel = None if members is None else selection_struct(members, handle_of)
    if limit is None:
        rc, agent_cap, cluster_cap, _, _, _ = agent_clusters_call(fn, handle, distance, sel, min_size, 0, 0)
        if rc != 0:
            raise err()
    else:
        agent_cap = cluster_cap = max(int(limit), 0)
    rc, _, _, ids, labels, table = agent_clusters_call(fn, handle, distance, sel, min_size, agent_cap, cluster_cap)
    if rc != 0:
        raise err()
    return ids, labels, table


def count_clusters_of(fn, handle, handle_of, err, distance, members, min_size):
    if int(min_size) < 0:
        raise CrowdSimError("agent_clusters: min_size is negative")
    sel = None if members is None else selection_struct(members, handle_of)
    rc, n_agents, n_clusters, _, _, _ = agent_clusters_call(fn, handle, distance, sel, min_size, 0, 0)
    if rc != 0:
        raise err()
    return int(n_clusters), int(n_agents)


NEIGHBOUR_DTYPE = np.dtype([("id", np.uint64), ("count", np.uint64), ("nearest", np.uint64), ("nearest_d2", np.float64)])
assert NEIGHBOUR_DTYPE.itemsize == C.sizeof(_abi.NeighbourStat) == 32


def agent_neighbours_call(fn, handle, distance, sel_subjects, sel_others, min_count, cap):
    """cs_agent_neighbours / cs_mesh_agent_neighbours with room for `cap` rows -> (the number of reported subjects, or
    None on error; the first min(number, cap) rows as a NEIGHBOUR_DTYPE array).  sel_subjects / sel_others: an
    _abi.Selection or None (everyone); cap == 0: the number only."""
    cap = max(int(cap), 0)
    rows = np.zeros(max(cap, 1), dtype=NEIGHBOUR_DTYPE)
    got = fn(handle, float(distance), C.byref(sel_subjects) if sel_subjects is not None else None,
             C.byref(sel_others) if sel_others is not None else None, int(min_count),
             rows.ctypes.data_as(C.POINTER(_abi.NeighbourStat)) if cap else None, cap)
    if got == _SIZE_MAX:
        return None, rows[:0].copy()
    return got, rows[:min(got, cap)].copy()


def agent_neighbours_of(fn, handle, handle_of, err, distance, subjects, others, min_count, limit):
    """agent_neighbours and count_agents_with_neighbours of Simulation and NativeTileMesh.  limit=None lists every
    reported subject (one counting call first), limit=0 only counts -> (number, rows)"""
    if int(min_count) < 0:
        raise CrowdSimError("agent_neighbours: min_count is negative")
    sel_s = None if subjects is None else selection_struct(subjects, handle_of)
    sel_o = None if others is None else selection_struct(others, handle_of)
    if limit is None:
        limit, _ = agent_neighbours_call(fn, handle, distance, sel_s, sel_o, min_count, 0)
        if limit is None:
            raise err()
    n, rows = agent_neighbours_call(fn, handle, distance, sel_s, sel_o, min_count, limit)
    if n is None:
        raise err()
    return int(n), rows


ENCOUNTER_DTYPE = np.dtype([("a", np.uint64), ("b", np.uint64), ("t", np.float64), ("d2", np.float64)])
assert ENCOUNTER_DTYPE.itemsize == C.sizeof(_abi.Encounter) == 32


def encounters_call(fn, handle, distance, horizon, range_, sel_a, sel_b, cap):
    """cs_encounters / cs_mesh_encounters with room for `cap` rows -> (the full count, or None on error; the first
    min(count, cap) rows as an ENCOUNTER_DTYPE array).  sel_a / sel_b: an _abi.Selection or None (everyone); cap == 0:
    the count only."""
    cap = max(int(cap), 0)
    rows = np.zeros(max(cap, 1), dtype=ENCOUNTER_DTYPE)
    got = fn(handle, float(distance), float(horizon), float(range_), C.byref(sel_a) if sel_a is not None else None,
             C.byref(sel_b) if sel_b is not None else None,
             rows.ctypes.data_as(C.POINTER(_abi.Encounter)) if cap else None, cap)
    if got == _SIZE_MAX:
        return None, rows[:0].copy()
    return got, rows[:min(got, cap)].copy()


def encounters_of(fn, handle, handle_of, err, distance, horizon, range_, a, b, limit):
    """encounters and count_encounters of Simulation and NativeTileMesh.  limit=None lists every encounter (one counting
    call first), limit=0 only counts -> (count, rows)"""
    sel_a = None if a is None else selection_struct(a, handle_of)
    sel_b = None if b is None else selection_struct(b, handle_of)
    if limit is None:
        limit, _ = encounters_call(fn, handle, distance, horizon, range_, sel_a, sel_b, 0)
        if limit is None:
            raise err()
        if limit > _abi.CS_PAIRS_MAX:
            limit = 1  # (the listing is refused by the library, with its message: no room is made for it here)
    n, rows = encounters_call(fn, handle, distance, horizon, range_, sel_a, sel_b, limit)
    if n is None:
        raise err()
    return int(n), rows


RAY_DTYPE = np.dtype([("ox", np.float64), ("oy", np.float64), ("ux", np.float64), ("uy", np.float64),
                      ("t_max", np.float64), ("ignore", np.uint64)])
RAY_HIT_DTYPE = np.dtype([("id", np.uint64), ("t", np.float64)])
assert RAY_DTYPE.itemsize == C.sizeof(_abi.Ray) == 48 and RAY_HIT_DTYPE.itemsize == C.sizeof(_abi.RayHit) == 16


def rays_array(origins, directions, t_max=np.inf, ignore=None):
    """The RAY_DTYPE array of n rays: origins and directions are (n, 2); t_max and ignore one value for all or one per ray
    (ignore None: nobody)."""
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 2)
    directions = np.asarray(directions, dtype=np.float64).reshape(-1, 2)
    if len(origins) != len(directions):
        raise ValueError("cast_rays: as many directions as origins")
    rays = np.zeros(len(origins), dtype=RAY_DTYPE)
    rays["ox"], rays["oy"] = origins[:, 0], origins[:, 1]
    rays["ux"], rays["uy"] = directions[:, 0], directions[:, 1]
    rays["t_max"] = np.asarray(t_max, dtype=np.float64)
    rays["ignore"] = _abi.CS_NO_HIT if ignore is None else np.asarray(ignore, dtype=np.uint64)
    return rays


def cast_rays_of(fn, handle, handle_of, err, rays, radius, targets, want_rows):
    """cast_rays and count_ray_hits of Simulation and NativeTileMesh -> (the number of rays that hit, the RAY_HIT_DTYPE
    rows or None)"""
    sel = None if targets is None else selection_struct(targets, handle_of)
    rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    n = len(rays)
    rows = np.zeros(max(n, 1), dtype=RAY_HIT_DTYPE) if want_rows else None
    got = fn(handle, rays.ctypes.data_as(C.POINTER(_abi.Ray)) if n else None, n, float(radius),
             C.byref(sel) if sel is not None else None,
             rows.ctypes.data_as(C.POINTER(_abi.RayHit)) if want_rows else None)
    if got == _SIZE_MAX:
        raise err()
    return int(got), (rows[:n].copy() if want_rows else None)


LEG_DTYPE = np.dtype([("x0", np.float64), ("y0", np.float64), ("vx", np.float64), ("vy", np.float64),
                      ("t0", np.float64), ("t1", np.float64), ("ignore", np.uint64)])
LEG_HIT_DTYPE = np.dtype([("id", np.uint64), ("s", np.float64)])
assert LEG_DTYPE.itemsize == C.sizeof(_abi.Leg) == 56 and LEG_HIT_DTYPE.itemsize == C.sizeof(_abi.LegHit) == 16


def legs_array(starts, velocities, t0, t1, ignore=None):
    """The LEG_DTYPE array of n legs: starts and velocities are (n, 2), or one pair for all legs; t0, t1 and ignore one
    value for all or one per leg (ignore None: nobody)."""
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 2)
    velocities = np.asarray(velocities, dtype=np.float64).reshape(-1, 2)
    n = np.broadcast_shapes((len(starts),), (len(velocities),), np.shape(t0), np.shape(t1),
                            () if ignore is None else np.shape(ignore))
    if len(n) != 1:
        raise ValueError("leg_conflicts: t0, t1 and ignore are scalars or one value per leg")
    legs = np.zeros(n[0], dtype=LEG_DTYPE)
    legs["x0"], legs["y0"] = starts[:, 0], starts[:, 1]
    legs["vx"], legs["vy"] = velocities[:, 0], velocities[:, 1]
    legs["t0"] = np.asarray(t0, dtype=np.float64)
    legs["t1"] = np.asarray(t1, dtype=np.float64)
    legs["ignore"] = _abi.CS_NO_HIT if ignore is None else np.asarray(ignore, dtype=np.uint64)
    return legs


def _path_legs(waypoints, times, ignore=None):
    """The legs of one timed polyline of k + 1 points: leg i runs from point i at times[i] to point i + 1 at
    times[i + 1] with velocity (p[i + 1] - p[i]) / (times[i + 1] - times[i]); a zero-duration leg is dropped, equal points
    over a positive duration are a wait."""
    p = np.asarray(waypoints, dtype=np.float64).reshape(-1, 2)
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    if len(p) != len(t) or len(t) < 1:
        raise ValueError("path_conflict: as many times as waypoints, and at least one")
    if not (np.isfinite(p).all() and np.isfinite(t).all() and t[0] >= 0.0 and (np.diff(t) >= 0.0).all()):
        raise ValueError("path_conflict: finite waypoints and finite non-decreasing times, the first >= 0")
    keep = np.diff(t) > 0.0
    lo, hi = t[:-1][keep], t[1:][keep]
    return legs_array(p[:-1][keep], (p[1:][keep] - p[:-1][keep]) / (hi - lo)[:, None], lo, hi, ignore)


def paths_legs(paths):
    """Many timed paths as one array of legs: paths is a list of (waypoints, times) as for path_conflict.  Returns (legs,
    path_of_leg): the LEG_DTYPE legs of all paths in order (ignore: nobody; set legs["ignore"] as needed) and for each leg
    the index of its path, so that one leg_conflicts call answers all paths and numpy reduces its rows."""
    legs = [_path_legs(w, t) for w, t in paths]
    owner = [np.full(len(l), k, dtype=np.int64) for k, l in enumerate(legs)]
    if not legs:
        return np.zeros(0, dtype=LEG_DTYPE), np.zeros(0, dtype=np.int64)
    return np.concatenate(legs), np.concatenate(owner)


def leg_conflicts_of(fn, handle, handle_of, err, legs, distance, speed_max, targets, want_rows):
    """leg_conflicts and count_leg_conflicts of Simulation and NativeTileMesh -> (the number of legs with a conflict, the
    LEG_HIT_DTYPE rows or None)"""
    sel = None if targets is None else selection_struct(targets, handle_of)
    legs = np.ascontiguousarray(legs, dtype=LEG_DTYPE)
    n = len(legs)
    rows = np.zeros(max(n, 1), dtype=LEG_HIT_DTYPE) if want_rows else None
    got = fn(handle, legs.ctypes.data_as(C.POINTER(_abi.Leg)) if n else None, n, float(distance), float(speed_max),
             C.byref(sel) if sel is not None else None,
             rows.ctypes.data_as(C.POINTER(_abi.LegHit)) if want_rows else None)
    if got == _SIZE_MAX:
        raise err()
    return int(got), (rows[:n].copy() if want_rows else None)


def path_conflict_of(leg_conflicts, waypoints, times, distance, speed_max, ignore, targets):
    """path_conflict of Simulation and NativeTileMesh over their leg_conflicts"""
    legs = _path_legs(waypoints, times, ignore)
    rows = leg_conflicts(legs, distance, speed_max, targets=targets)
    hit = np.nonzero(rows["id"] != np.uint64(_abi.CS_NO_HIT))[0]
    if not len(hit):
        return None
    k = int(hit[0])
    l, s = legs[k], float(rows["s"][k])
    return int(rows["id"][k]), float(l["t0"]) + s, k, (float(l["x0"]) + float(l["vx"]) * s, float(l["y0"]) + float(l["vy"]) * s)


LEG_INTERVAL_DTYPE = np.dtype(_abi.LEG_INTERVAL_DTYPE)
assert LEG_INTERVAL_DTYPE.itemsize == C.sizeof(_abi.LegInterval) == 32


def leg_intervals_call(fn, handle, legs, distance, speed_max, sel, want_counts, cap):
    """cs_leg_intervals / cs_mesh_leg_intervals with room for `cap` rows -> (the full count, or None on error; the
    per-leg uint64 counts, or None; the first min(count, cap) rows as a LEG_INTERVAL_DTYPE array).  cap == 0: counts only."""
    legs = np.ascontiguousarray(legs, dtype=LEG_DTYPE)
    n, cap = len(legs), max(int(cap), 0)
    counts = np.zeros(max(n, 1), dtype=np.uint64) if want_counts else None
    rows = np.zeros(max(cap, 1), dtype=LEG_INTERVAL_DTYPE)
    got = fn(handle, legs.ctypes.data_as(C.POINTER(_abi.Leg)) if n else None, n, float(distance), float(speed_max),
             C.byref(sel) if sel is not None else None,
             counts.ctypes.data_as(C.POINTER(C.c_uint64)) if want_counts else None,
             rows.ctypes.data_as(C.POINTER(_abi.LegInterval)) if cap else None, cap)
    if got == _SIZE_MAX:
        return None, None, rows[:0].copy()
    return got, (counts[:n].copy() if want_counts else None), rows[:min(got, cap)].copy()


def leg_intervals_of(fn, handle, handle_of, err, legs, distance, speed_max, targets, limit):
    """leg_intervals and count_leg_intervals of Simulation and NativeTileMesh.  limit=None lists every interval (one
    counting call first), limit=0 only counts -> (count, per-leg counts, rows)"""
    sel = None if targets is None else selection_struct(targets, handle_of)
    if limit is None:
        limit, _, _ = leg_intervals_call(fn, handle, legs, distance, speed_max, sel, False, 0)
        if limit is None:
            raise err()
        if limit > _abi.CS_PAIRS_MAX:
            limit = 1  # (the listing is refused by the library, with its message: no room is made for it here)
    n, counts, rows = leg_intervals_call(fn, handle, legs, distance, speed_max, sel, True, limit)
    if n is None:
        raise err()
    return int(n), counts, rows


def merge_leg_intervals(rows, n_legs):
    """The occupied time of each leg: (offsets, spans).  rows: LEG_INTERVAL_DTYPE rows of legs 0 .. n_legs - 1 in any
    order; spans: float64 (m, 2), the union of the [s_in, s_out] of each leg as disjoint (start, end) in seconds after the
    leg's t0, ascending in time, overlapping and touching spans merged; the spans of leg k are
    spans[offsets[k]:offsets[k + 1]] (offsets: int64, n_legs + 1 entries).  Pure numpy."""
    rows = np.asarray(rows, dtype=LEG_INTERVAL_DTYPE)
    n_legs = int(n_legs)
    if len(rows) and int(rows["leg"].max()) >= n_legs:
        raise ValueError("merge_leg_intervals: a row of a leg beyond n_legs")
    order = np.lexsort((rows["s_out"], rows["s_in"], rows["leg"]))
    leg, lo, hi = rows["leg"][order].astype(np.int64), rows["s_in"][order], rows["s_out"][order]
    first = np.ones(len(rows), dtype=bool)  # does row i begin a span: another leg, or later than all that came before
    if len(rows) > 1:
        # the largest end so far within the leg, on the ranks of the times (integers: exact, so touching spans merge);
        # legs are kept apart by an offset larger than any rank
        times, rank = np.unique(np.concatenate([lo, hi]), return_inverse=True)
        r_lo, r_hi, step = rank[:len(rows)], rank[len(rows):], len(times) + 1
        reach = np.maximum.accumulate(r_hi + leg * step)[:-1] - leg[1:] * step
        first[1:] = (leg[1:] != leg[:-1]) | (r_lo[1:] > reach)
    begin = np.nonzero(first)[0]
    spans = np.zeros((len(begin), 2), dtype=np.float64)
    if len(begin):
        spans[:, 0] = lo[begin]
        spans[:, 1] = np.maximum.reduceat(hi, begin)
    offsets = np.zeros(n_legs + 1, dtype=np.int64)
    np.cumsum(np.bincount(leg[begin], minlength=n_legs), out=offsets[1:])
    return offsets, spans


def flow_field_to_goals(blocked, goals, origin, cell, speed, return_distance=False):
    """Vectors for a FieldPlanner(origin, cell, vectors) that lead to the nearest goal around the blocked bins.  blocked,
    goals: bool (ny, nx).  An 8-connected Dijkstra from the goal bins over the free ones (a step costs the distance between
    the bin centres; a diagonal step needs both bins beside it free, so nobody cuts a wall's corner); every free bin gets
    `speed` times the unit vector to the neighbour through which its path is cheapest, a goal bin gets zero, blocked and
    unreachable bins get NaN.  -> float32 (ny, nx, 2), with return_distance also the path lengths, float64 (ny, nx), inf
    where no path exists.  Pure numpy and a heap; for examples and benchmarks, it claims no optimality.  (The origin does
    not enter the vectors; it is taken so that the call reads like the planner's.)"""
    import heapq
    blocked = np.asarray(blocked, dtype=bool)
    goals = np.asarray(goals, dtype=bool)
    if blocked.ndim != 2 or goals.shape != blocked.shape:
        raise ValueError("flow_field_to_goals: blocked and goals are bool arrays of one shape (ny, nx)")
    float(origin[0]), float(origin[1])
    cell = np.asarray(cell, dtype=np.float64).reshape(-1)
    cw, ch = float(cell[0]), float(cell[-1])
    ny, nx = blocked.shape
    dist = np.full((ny, nx), np.inf)
    via = np.zeros((ny, nx, 2), dtype=np.int64)  # the step (dx, dy) towards the goal
    heap = []
    for iy, ix in zip(*np.nonzero(goals & ~blocked)):
        dist[iy, ix] = 0.0
        heap.append((0.0, int(iy), int(ix)))
    heapq.heapify(heap)
    steps = [(dx, dy, float(np.hypot(dx * cw, dy * ch))) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]
    while heap:
        d, iy, ix = heapq.heappop(heap)
        if d > dist[iy, ix]:
            continue
        for dx, dy, cost in steps:
            jx, jy = ix + dx, iy + dy
            if not (0 <= jx < nx and 0 <= jy < ny) or blocked[jy, jx]:
                continue
            if dx and dy and (blocked[iy, jx] or blocked[jy, ix]):
                continue
            if d + cost < dist[jy, jx]:
                dist[jy, jx] = d + cost
                via[jy, jx] = (-dx, -dy)
                heapq.heappush(heap, (d + cost, jy, jx))
    out = np.full((ny, nx, 2), np.nan, dtype=np.float32)
    reached = np.isfinite(dist)
    step = via[reached].astype(np.float64) * (cw, ch)
    norm = np.hypot(step[:, 0], step[:, 1])
    norm[norm == 0.0] = 1.0  # (the goal bins: a zero vector)
    out[reached] = (float(speed) * step / norm[:, None]).astype(np.float32)
    return (out, dist) if return_distance else out


FLOW_STEPS = tuple((dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy)  # the order of cs_flow_field_solve


def _flow_masks(goals, blocked, slowness, counts):
    goals = np.asarray(goals)
    if goals.ndim != 2 or goals.size == 0:
        raise CrowdSimError("flow field: goals is an array of shape (ny, nx)")
    shape = goals.shape
    goals = np.ascontiguousarray(goals != 0, dtype=np.uint8)
    if blocked is not None:
        blocked = np.asarray(blocked)
        if blocked.shape != shape:
            raise CrowdSimError("flow field: blocked has the shape of goals")
        blocked = np.ascontiguousarray(blocked != 0, dtype=np.uint8)
    if slowness is not None:
        slowness = np.ascontiguousarray(np.asarray(slowness, dtype=np.float32))
        if slowness.shape != shape:
            raise CrowdSimError("flow field: slowness has the shape of goals")
    if counts is not None:
        counts = np.ascontiguousarray(np.asarray(counts, dtype=np.uint32))
        if counts.shape != shape:
            raise CrowdSimError("flow field: counts has the shape of goals")
    return goals, blocked, slowness, counts


def flow_field_solve_host(blocked, goals, cell, speed, *, slowness=None, counts=None, density_weight=0.0):
    """The rule of cs_flow_field_solve (include/crowdstep_state.h, "Solving a flow field on the device") on the host, as a
    heap Dijkstra in f64 with exactly the rule's operations, each rounded once: what the device solver is checked against
    bit for bit, and what a library without the call falls back to.  blocked (or None), goals: (ny, nx), non-zero = set;
    cell: a scalar or (w, h); slowness: float32 (ny, nx) or None; counts: uint32 (ny, nx), what agent_field reports, used
    when density_weight != 0.  A step from a bin costs len(step) * s(bin), s = slowness * (1 + density_weight * count).
    -> (vectors float32 (ny, nx, 2), dist float64 (ny, nx)): zero at goals, NaN / inf at blocked and unreachable bins."""
    import heapq
    import math
    goals, blocked, slowness, counts = _flow_masks(goals, blocked, slowness, counts)
    cell = np.asarray(cell, dtype=np.float64).reshape(-1)
    cw, ch = float(cell[0]), float(cell[-1])
    speed, w = float(speed), float(density_weight)
    if not (math.isfinite(speed) and speed >= 0.0 and math.isfinite(w) and 0.0 <= w <= 2.0 ** 32):
        raise CrowdSimError("flow field: speed is finite and >= 0, density_weight in [0, 2^32]")
    if slowness is not None and not (np.isfinite(slowness).all() and (slowness >= 0).all()):
        raise CrowdSimError("flow field: a slowness that is NaN, infinite or negative")
    if w != 0.0 and counts is None:
        raise CrowdSimError("flow field: a density_weight needs counts")
    ny, nx = goals.shape
    wall = blocked.astype(bool).tolist() if blocked is not None else [[False] * nx for _ in range(ny)]
    diag = math.sqrt(cw * cw + ch * ch)
    lens = [diag if dx and dy else cw if dx else ch for dx, dy in FLOW_STEPS]
    slow = [[1.0] * nx for _ in range(ny)] if slowness is None else slowness.astype(np.float64).tolist()
    if w != 0.0:
        cnt = counts.tolist()
        slow = [[slow[iy][ix] * (1.0 + w * float(cnt[iy][ix])) for ix in range(nx)] for iy in range(ny)]
    inf = math.inf
    dist = [[inf] * nx for _ in range(ny)]
    heap = []
    for iy, ix in zip(*np.nonzero(goals)):
        if not wall[iy][ix]:
            dist[iy][ix] = 0.0
            heap.append((0.0, int(iy), int(ix)))
    heapq.heapify(heap)
    while heap:
        d, iy, ix = heapq.heappop(heap)
        if d > dist[iy][ix]:
            continue
        # every bin (jx, jy) whose step k leads here: (jx + dx, jy + dy) == (ix, iy)
        for k, (dx, dy) in enumerate(FLOW_STEPS):
            jx, jy = ix - dx, iy - dy
            if not (0 <= jx < nx and 0 <= jy < ny) or wall[jy][jx]:
                continue
            if dx and dy and (wall[jy][ix] or wall[iy][jx]):
                continue
            c = d + lens[k] * slow[jy][jx]
            if c < dist[jy][jx]:
                dist[jy][jx] = c
                heapq.heappush(heap, (c, jy, jx))
    table = []
    with np.errstate(all="ignore"):
        for k, (dx, dy) in enumerate(FLOW_STEPS):
            sx, sy, n = np.float64(dx * cw), np.float64(dy * ch), np.float64(lens[k])
            table.append((np.float32((np.float64(speed) * sx) / n), np.float32((np.float64(speed) * sy) / n)))
    vectors = np.full((ny, nx, 2), np.nan, dtype=np.float32)
    for iy in range(ny):
        for ix in range(nx):
            if wall[iy][ix] or dist[iy][ix] == inf:
                continue
            if goals[iy, ix]:
                vectors[iy, ix] = (0.0, 0.0)
                continue
            best, pick = inf, None
            for k, (dx, dy) in enumerate(FLOW_STEPS):
                jx, jy = ix + dx, iy + dy
                if not (0 <= jx < nx and 0 <= jy < ny) or wall[jy][jx]:
                    continue
                if dx and dy and (wall[iy][jx] or wall[jy][ix]):
                    continue
                c = dist[jy][jx] + lens[k] * slow[iy][ix]
                if c < best:
                    best, pick = c, k
            if pick is not None:
                vectors[iy, ix] = table[pick]
    return vectors, np.array(dist, dtype=np.float64).reshape(ny, nx)


def flow_solve_call(fn, handle, origin, cell, goals, speed, blocked, slowness, density_weight, sel, hlp, vectors, distance):
    """cs_flow_field_solve / cs_mesh_flow_field_solve -> (rc, vectors or None, dist or None, {"reached", "rounds"})"""
    goals, blocked, slowness, _ = _flow_masks(goals, blocked, slowness, None)
    ny, nx = goals.shape
    desc = _abi.FlowDesc()
    desc.raster = field_desc(origin, cell, (ny, nx))
    u8 = C.POINTER(C.c_uint8)
    desc.goals = goals.ctypes.data_as(u8)
    desc.blocked = blocked.ctypes.data_as(u8) if blocked is not None else None
    desc.slowness = slowness.ctypes.data_as(C.POINTER(C.c_float)) if slowness is not None else None
    desc.speed, desc.density_weight = float(speed), float(density_weight)
    desc.density_filter = C.pointer(sel) if sel is not None else None
    vec = np.zeros((ny, nx, 2), dtype=np.float32) if vectors else None
    dist = np.zeros((ny, nx), dtype=np.float64) if distance else None
    stats = _abi.FlowStats()
    rc = fn(handle, C.byref(desc), 0xFFFFFFFF if hlp is None else hlp,
            vec.ctypes.data_as(C.POINTER(C.c_float)) if vectors else None,
            dist.ctypes.data_as(C.POINTER(C.c_double)) if distance else None, C.byref(stats))
    return rc, vec, dist, {"reached": int(stats.reached), "rounds": int(stats.rounds)}


def flow_solve_of(sim, fn, handle, handle_of, origin, cell, goals, speed, blocked, slowness, density_weight, density_filter,
                  planner, vectors, distance):
    """solve_flow_field of a Simulation or a NativeTileMesh: the device call, or on a library without it (fn is None)
    agent_field + flow_field_solve_host + FieldPlanner.update"""
    shape = np.asarray(goals).shape
    if planner is not None:
        if not isinstance(planner, FieldPlanner):
            raise CrowdSimError("solve_flow_field: planner is a FieldPlanner")
        same = field_desc(planner.origin, planner.cell, planner.vectors.shape[:2])
        mine = field_desc(origin, cell, shape if len(shape) == 2 else (0, 0))
        if bytes(same) != bytes(mine):
            raise CrowdSimError("solve_flow_field: the planner's raster is not the solve's")
    hlp = None if planner is None else sim._handle(planner)
    if fn is not None and (planner is None or planner._bound):
        sel = None if density_filter is None else selection_struct(density_filter, handle_of)
        rc, vec, dist, stats = flow_solve_call(fn, handle, origin, cell, goals, speed, blocked, slowness, density_weight,
                                               sel, hlp, vectors, distance)
        if rc != 0:
            raise sim._err()
        if planner is not None and vec is not None:
            planner.vectors = vec.copy()  # (the host copy follows what the device now samples)
        return vec, dist, stats
    counts = sim.agent_field(origin, cell, shape, density_filter) if float(density_weight) != 0.0 else None
    vec, dist = flow_field_solve_host(blocked, goals, cell, speed, slowness=slowness, counts=counts,
                                      density_weight=density_weight)
    if planner is not None:
        planner.update(vec)
    stats = {"reached": int(np.isfinite(dist).sum()), "rounds": 0}
    return (vec if vectors else None), (dist if distance else None), stats


def free_spans(offsets, spans, t0, t1):
    """The complement of merge_leg_intervals' spans inside each leg: per leg a list of (start, end) ABSOLUTE times inside
    [t0[k], t1[k]] during which nobody is within the distance, ascending; spans of zero length are left out."""
    out = []
    for k in range(len(offsets) - 1):
        a, b, free = float(t0[k]), float(t1[k]), []
        at = a
        for s, e in spans[offsets[k]:offsets[k + 1]]:
            if a + float(s) > at:
                free.append((at, a + float(s)))
            at = max(at, a + float(e))
        if b > at:
            free.append((at, b))
        out.append(free)
    return out


def free_intervals_of(leg_intervals, points, t0, t1, distance, speed_max, ignore, targets):
    """free_intervals of Simulation and NativeTileMesh over their leg_intervals"""
    legs = legs_array(points, (0.0, 0.0), t0, t1, ignore)
    offsets, spans = merge_leg_intervals(leg_intervals(legs, distance, speed_max, targets=targets), len(legs))
    return free_spans(offsets, spans, legs["t0"], legs["t1"])


ZONE_DTYPE = np.dtype(_abi.ZONE_DTYPE)
ZONE_AGENT_DTYPE = np.dtype(_abi.ZONE_AGENT_DTYPE)
assert ZONE_DTYPE.itemsize == C.sizeof(_abi.Zone) == 16 and ZONE_AGENT_DTYPE.itemsize == C.sizeof(_abi.ZoneAgent) == 16


def zones_array(polygons):
    """The polygons of zone_agents as the library takes them: polygons, a list of (k, 2) arrays of (x, y) vertices (k >= 3,
    the ring closes from the last to the first) -> (zones, a ZONE_DTYPE array of one run per polygon; vertices, float64
    (n_vertices, 2), the polygons' vertices one after the other).  A pair (zones, vertices) that is already of this form
    (zones that share vertices are written that way) is passed through."""
    if isinstance(polygons, tuple) and len(polygons) == 2 and getattr(polygons[0], "dtype", None) == ZONE_DTYPE:
        return (np.ascontiguousarray(polygons[0], dtype=ZONE_DTYPE),
                np.ascontiguousarray(polygons[1], dtype=np.float64).reshape(-1, 2))
    rings = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in polygons]
    zones = np.zeros(len(rings), dtype=ZONE_DTYPE)
    zones["count"] = [len(r) for r in rings]
    zones["first"] = np.concatenate([[0], np.cumsum(zones["count"].astype(np.uint64))[:-1]]) if len(rings) else []
    vertices = np.concatenate(rings) if rings else np.zeros((0, 2), dtype=np.float64)
    return zones, np.ascontiguousarray(vertices, dtype=np.float64)


def zone_agents_call(fn, handle, zones, vertices, sel, want_counts, cap):
    """cs_zone_agents / cs_mesh_zone_agents with room for `cap` rows -> (the full count, or None on error; the per-zone
    uint64 counts, or None; the first min(count, cap) rows as a ZONE_AGENT_DTYPE array).  cap == 0: counts only."""
    zones = np.ascontiguousarray(zones, dtype=ZONE_DTYPE)
    vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 2)
    n, cap = len(zones), max(int(cap), 0)
    counts = np.zeros(max(n, 1), dtype=np.uint64) if want_counts else None
    rows = np.zeros(max(cap, 1), dtype=ZONE_AGENT_DTYPE)
    got = fn(handle, zones.ctypes.data_as(C.POINTER(_abi.Zone)) if n else None, n,
             vertices.ctypes.data_as(C.POINTER(C.c_double)) if len(vertices) else None, len(vertices),
             C.byref(sel) if sel is not None else None,
             counts.ctypes.data_as(C.POINTER(C.c_uint64)) if want_counts else None,
             rows.ctypes.data_as(C.POINTER(_abi.ZoneAgent)) if cap else None, cap)
    if got == _SIZE_MAX:
        return None, None, rows[:0].copy()
    return got, (counts[:n].copy() if want_counts else None), rows[:min(got, cap)].copy()


def zone_agents_of(fn, handle, handle_of, err, polygons, filter, limit):
    """zone_agents and count_zone_agents of Simulation and NativeTileMesh.  limit=None lists every row (one counting call
    first), limit=0 only counts -> (count, per-zone counts, rows)"""
    zones, vertices = zones_array(polygons)
    sel = None if filter is None else selection_struct(filter, handle_of)
    if limit is None:
        limit, _, _ = zone_agents_call(fn, handle, zones, vertices, sel, False, 0)
        if limit is None:
            raise err()
        if limit > _abi.CS_PAIRS_MAX:
            limit = 1  # (the listing is refused by the library, with its message: no room is made for it here)
    n, counts, rows = zone_agents_call(fn, handle, zones, vertices, sel, True, limit)
    if n is None:
        raise err()
    return int(n), counts, rows


GATE_DTYPE = np.dtype(_abi.GATE_DTYPE)
GATE_CROSSING_DTYPE = np.dtype(_abi.GATE_CROSSING_DTYPE)
assert GATE_DTYPE.itemsize == C.sizeof(_abi.Gate) == 48
assert GATE_CROSSING_DTYPE.itemsize == C.sizeof(_abi.GateCrossing) == 32


def gates_array(segments, t0=0.0, t1=1.0):
    """The GATE_DTYPE array of n gates: segments is (n, 4) rows (ax, ay, bx, by), or (n, 2, 2) pairs of points A, B; t0 and
    t1 (seconds from now) one value for all or one per gate.  Left and right are those of somebody looking from A to B."""
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 4)
    n = np.broadcast_shapes((len(seg),), np.shape(t0), np.shape(t1))
    if len(n) != 1:
        raise ValueError("gate_crossings: t0 and t1 are scalars or one value per gate")
    gates = np.zeros(n[0], dtype=GATE_DTYPE)
    gates["ax"], gates["ay"], gates["bx"], gates["by"] = seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3]
    gates["t0"] = np.asarray(t0, dtype=np.float64)
    gates["t1"] = np.asarray(t1, dtype=np.float64)
    return gates


def path_gates(points, t0, t1):
    """The chain of gates along a polyline of k + 1 points: gate i runs from point i to point i + 1, all with the window
    t0 .. t1.  The gates share their vertices and u is half-open, so a walker that passes through a vertex belongs to one
    gate of the chain wherever the arithmetic is exact."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if len(p) < 2:
        raise ValueError("path_gates: at least two points")
    return gates_array(np.concatenate([p[:-1], p[1:]], axis=1), t0, t1)


def gate_crossings_call(fn, handle, gates, speed_max, sel, want_counts, cap):
    """cs_gate_crossings / cs_mesh_gate_crossings with room for `cap` rows -> (the full count, or None on error; the
    uint64 counts (n, 2), column 0 dir +1 and column 1 dir -1, or None; the first min(count, cap) rows as a
    GATE_CROSSING_DTYPE array).  cap == 0: counts only."""
    gates = np.ascontiguousarray(gates, dtype=GATE_DTYPE)
    n, cap = len(gates), max(int(cap), 0)
    counts = np.zeros((max(n, 1), 2), dtype=np.uint64) if want_counts else None
    rows = np.zeros(max(cap, 1), dtype=GATE_CROSSING_DTYPE)
    got = fn(handle, gates.ctypes.data_as(C.POINTER(_abi.Gate)) if n else None, n, float(speed_max),
             C.byref(sel) if sel is not None else None,
             counts.ctypes.data_as(C.POINTER(C.c_uint64)) if want_counts else None,
             rows.ctypes.data_as(C.POINTER(_abi.GateCrossing)) if cap else None, cap)
    if got == _SIZE_MAX:
        return None, None, rows[:0].copy()
    return got, (counts[:n].copy() if want_counts else None), rows[:min(got, cap)].copy()


def gate_crossings_of(fn, handle, handle_of, err, gates, speed_max, filter, limit):
    """gate_crossings and count_gate_crossings of Simulation and NativeTileMesh.  limit=None lists every row (one counting
    call first), limit=0 only counts -> (count, counts (n, 2), rows)"""
    sel = None if filter is None else selection_struct(filter, handle_of)
    if limit is None:
        limit, _, _ = gate_crossings_call(fn, handle, gates, speed_max, sel, False, 0)
        if limit is None:
            raise err()
        if limit > _abi.CS_PAIRS_MAX:
            limit = 1  # (the listing is refused by the library, with its message: no room is made for it here)
    n, counts, rows = gate_crossings_call(fn, handle, gates, speed_max, sel, True, limit)
    if n is None:
        raise err()
    return int(n), counts, rows


def _agents_dict(arr):
    return {int(r["id"]): Agent(int(r["id"]), np.array([r["x"], r["y"]]), np.array([r["vx"], r["vy"]]),
                                int(r["next_waypoint"]), float(r["eyesight_range"]))
            for r in arr}


def edited_agents(agents, read):
    """(records, mask): the entries of an `agents` dict whose position, velocity or next_waypoint differ (bit for bit)
    from `read`, the array the dict was made from, and the union of the fields that changed.  Raises CrowdSimError if a
    field that cannot be written changed, or if the dict holds an id that was not read."""
    by_id = {int(r["id"]): k for k, r in enumerate(read)}
    extra = [i for i in agents if i not in by_id]
    if extra:
        raise CrowdSimError(f"commit_agents: agent {min(extra)} was not read; commit_agents writes existing agents "
                            "(add_agents adds them)")
    rows, mask = [], 0
    for aid, a in agents.items():
        r = read[by_id[aid]]
        if (int(a.agent_id) != aid or float(a.eyesight_range) != float(r["eyesight_range"]) or a.orientation != 0.0
                or a.angular_vel != 0.0):
            raise CrowdSimError(f"commit_agents: agent {aid}: only position, velocity and next_waypoint are writable "
                                "(agent_id, eyesight_range, orientation and angular_vel changed)")
        pos = np.asarray(a.position, dtype=np.float64).reshape(2)
        vel = np.asarray(a.velocity, dtype=np.float64).reshape(2)
        wp = int(a.next_waypoint)
        if wp < 0:
            raise CrowdSimError(f"commit_agents: agent {aid}: next_waypoint {wp} is negative")
        m = 0
        if pos.tobytes() != np.array([r["x"], r["y"]]).tobytes():
            m |= _abi.CS_WRITE_POSITION
        if vel.tobytes() != np.array([r["vx"], r["vy"]]).tobytes():
            m |= _abi.CS_WRITE_VELOCITY
        if wp != int(r["next_waypoint"]):
            m |= _abi.CS_WRITE_NEXT_WAYPOINT
        if m:
            row = r.copy()
            row["x"], row["y"], row["vx"], row["vy"], row["next_waypoint"] = pos[0], pos[1], vel[0], vel[1], wp
            rows.append(row)
            mask |= m
    return np.array(rows, dtype=AGENT_DTYPE), mask


class Simulation:
    """Simulation<LocationHash2D>, lib.rs:69-383, on one MI355X."""

    def __init__(self, spatial_index, device=0, flags=_abi.CS_CFG_DEFAULT, capacity_hint=0,
                 stream=None, tile=None, halo_cells=0):
        self._lib = self._load_library()
        form = spatial_index.device_form() if hasattr(spatial_index, "device_form") else None
        if form is None or not hasattr(form, "_desc"):
            raise CrowdSimError(
                "Simulation<T: SpatialIndex>: on this backend the spatial index is the neighbour kernel itself; "
                f"{type(spatial_index).__name__} does not describe itself as a uniform grid (device_form() -> LocationHash2D)")
        spatial_index = form
        grid = spatial_index._desc()
        cfg = _abi.DeviceCfg(int(device), int(flags), 0, 0, 0, 0, 0, 0, int(capacity_hint),
                             C.c_void_p(stream) if stream else None)
        if tile is not None:
            cfg.tile_cx0, cfg.tile_cx1, cfg.tile_cy0, cfg.tile_cy1 = [int(t) for t in tile]
            cfg.halo_cells = int(halo_cells)
        self.spatial_index = spatial_index
        self._engine = self._lib.cs_create(C.byref(grid), C.byref(cfg))
        if not self._engine:
            raise CrowdSimError("cs_create failed: " + self._lib.cs_last_error(None).decode())
        self._lib.cs_event_recording(self._engine, 0)  # no listeners yet (lib.rs:88)
        self._planner_handles = {}
        self._planners_alive = []
        self._host_lps = False  # some LocalPlanner is host code: its agents are tracked for remove_agent
        self._host_lp_of_agent = {}
        self._host_lp_of_sink = {}
        self._listeners = {}
        self._next_listener = 0
        self._source_sinks = {}
        self._agents_cache = None
        self.last_report = None

    def _load_library(self):
        return _native.load()

    @classmethod
    def borrowed(cls, lib, engine, spatial_index=None):
        """A view of an engine somebody else owns (a tile of a mesh, cs_mesh_tile): profiling, kernel statistics,
        snapshots, queries of that tile.  Closing the view leaves the engine alone."""
        self = cls.__new__(cls)
        self._lib, self._engine, self._borrowed = lib, engine, True
        self.spatial_index = spatial_index
        self._planner_handles, self._planners_alive = {}, []
        self._host_lps, self._host_lp_of_agent, self._host_lp_of_sink = False, {}, {}
        self._listeners, self._next_listener, self._source_sinks = {}, 0, {}
        self._agents_cache, self.last_report = None, None
        return self

    def close(self):
        if getattr(self, "_engine", None):
            if not getattr(self, "_borrowed", False):
                self._lib.cs_destroy(self._engine)
            self._engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers --
    @property
    def backend(self):
        return self._lib.cs_backend_name(self._engine).decode()

    def _err(self):
        why = self._lib.cs_last_error(self._engine).decode()
        for planner in self._planners_alive:  # a host planner that raised: its exception is the cause
            cause = getattr(planner, "failure", None)
            if cause is not None:
                planner.failure = None
                err = CrowdSimError(f"{why} ({cause!r})")
                err.__cause__ = cause
                return err
        return CrowdSimError(why)

    def _handle(self, planner):
        key = id(planner)
        if key not in self._planner_handles:
            handle = planner._register(self._lib, self._engine)
            if handle == 0xFFFFFFFF:  # the engine refused the planner (cs_last_error says why)
                raise self._err()
            self._planner_handles[key] = handle
            self._planners_alive.append(planner)
            if hasattr(planner, "_registered_with"):
                planner._registered_with(self)
        return self._planner_handles[key]

    def _dispatch_events(self):
        buf = (_abi.Event * 4096)()
        while True:
            n = self._lib.cs_drain_events(self._engine, buf, len(buf))
            for i in range(n):
                ev = buf[i]
                if self._host_lps:  # LocalPlanner::remove_agent for agents of host planners (lib.rs:181-184)
                    if ev.kind == _abi.CS_EVENT_SPAWNED and ev.source_sink in self._host_lp_of_sink:
                        self._host_lp_of_agent[int(ev.id)] = self._host_lp_of_sink[ev.source_sink]
                    elif ev.kind == _abi.CS_EVENT_DESTROYED:
                        planner = self._host_lp_of_agent.pop(int(ev.id), None)
                        if planner is not None:
                            planner.remove_agent(int(ev.id))
                for listener in self._listeners.values():
                    if ev.kind == _abi.CS_EVENT_SPAWNED:
                        listener.agent_spawned(np.array([ev.x, ev.y]), int(ev.id))
                    elif ev.kind == _abi.CS_EVENT_DESTROYED:
                        listener.agent_destroyed(int(ev.id))
            if n < len(buf):
                break

    # -- reference API --
    def add_agents(self, spawn_positions, high_level_planner, local_planner,
                   agent_eyesight_range):
        """lib.rs:119-156 -> list of agent ids (sequential from the last allocated id)."""
        pts = np.ascontiguousarray(np.asarray(spawn_positions, dtype=np.float64).reshape(-1, 2))
        n = pts.shape[0]
        ids = np.zeros(n, dtype=np.uint64)
        rc = self._lib.cs_add_agents(
            self._engine, pts.ctypes.data_as(C.POINTER(C.c_double)), n,
            self._handle(high_level_planner), self._handle(local_planner),
            float(agent_eyesight_range), ids.ctypes.data_as(C.POINTER(C.c_uint64)))
        self._agents_cache = None
        if getattr(local_planner, "_host_code", False):
            self._host_lps = True
            self._lib.cs_event_recording(self._engine, 1)
            for i in ids[:n if rc == 0 else 0]:
                self._host_lp_of_agent[int(i)] = local_planner
        self._dispatch_events()
        if rc != 0:
            raise self._err()
        return [int(i) for i in ids]

    def add_source_sink(self, source_sink):
        """lib.rs:159-161 -> handle"""
        desc, keep = source_sink_desc(source_sink, self._handle)
        handle = self._lib.cs_add_source_sink(self._engine, C.byref(desc))
        if handle == 0xFFFFFFFF:
            raise self._err()
        self._source_sinks[handle] = (source_sink, keep)
        if getattr(source_sink.local_planner, "_host_code", False):
            self._host_lps = True
            self._host_lp_of_sink[handle] = source_sink.local_planner
            self._lib.cs_event_recording(self._engine, 1)
        return handle

    def remove_source_sink(self, handle, with_agents=False):
        """lib.rs:164-168: the registry entry goes and the agents it spawned walk on.  with_agents=True removes those
        agents first (remove_selected(source_sink=handle), events and planner callbacks included): the reference's own
        TODO (lib.rs:165-166)."""
        if with_agents:
            self.remove_selected(source_sink=int(handle))
        self._lib.cs_remove_source_sink(self._engine, int(handle))
        self._source_sinks.pop(handle, None)

    def add_event_listener(self, event_listener):
        """lib.rs:171-173 -> handle"""
        handle = self._next_listener
        self._next_listener += 1
        self._listeners[handle] = event_listener
        self._lib.cs_event_recording(self._engine, 1)
        return handle

    def remove_agents(self, agent):
        """lib.rs:176-192 (an unknown id raises instead of panicking)."""
        rc = self._lib.cs_remove_agent(self._engine, int(agent))
        self._agents_cache = None
        self._dispatch_events()
        if rc != 0:
            raise self._err()

    def step(self, dur, report=True):
        """lib.rs:195-383.  `dur`: seconds (float) or datetime.timedelta."""
        dt = dur.total_seconds() if isinstance(dur, datetime.timedelta) else float(dur)
        rep = _abi.StepReport()
        need_report = report or bool(self._listeners) or self._host_lps
        rc = self._lib.cs_step(self._engine, dt, C.byref(rep) if need_report else None)
        self._agents_cache = None
        if need_report:
            self.last_report = rep.as_dict()
        if self._listeners or self._host_lps or rc != 0:
            self._dispatch_events()
        if rc != 0:
            raise self._err()

    def synchronize(self):
        if self._lib.cs_synchronize(self._engine) != 0:
            raise self._err()

    # -- observation --
    def read_agents(self):
        """Structured array (id, x, y, vx, vy, next_waypoint, eyesight_range), ascending id.
        Steps taken without a report return before the device has finished: an Err of such a
        step ("Index out of bounds") is raised here, by the first call that waits for it."""
        self.synchronize()
        n = self._lib.cs_agent_count(self._engine)
        buf = (_abi.AgentView * max(n, 1))()
        got = self._lib.cs_read_agents(self._engine, buf, n)
        return np.frombuffer(buf, dtype=AGENT_DTYPE, count=got).copy()

    @property
    def agents(self):
        """`pub agents: HashMap<AgentId, Agent>` (lib.rs:71), read back lazily."""
        if self._agents_cache is None:
            arr = self.read_agents()
            self._agents_cache = _agents_dict(arr)
            self._agents_read = arr  # (what commit_agents compares the dict with)
        return self._agents_cache

    def write_agents(self, records, fields=_abi.CS_WRITE_ALL):
        """`agents.get_mut(&id)` (lib.rs:71) for a batch: `records` is the structured array read_agents returns
        (AGENT_DTYPE), `fields` an int mask of _abi.CS_WRITE_* bits or names from WRITE_FIELDS ("position",
        "velocity", "next_waypoint").  The written values become the agents' start-of-step state; eyesight_range is
        ignored.  All or nothing: a refused batch raises CrowdSimError and changes nothing (include/crowdstep_state.h)."""
        fn = getattr(self._lib, "cs_write_agents", None)
        if fn is None:
            raise CrowdSimError(f"write_agents needs the HIP engine: the {self.backend} library does not implement "
                                "include/crowdstep_state.h")
        arr = write_records(records)
        rc = fn(self._engine, arr.ctypes.data_as(C.POINTER(_abi.AgentView)), len(arr), write_mask(fields))
        self._agents_cache = None
        if rc != 0:
            raise self._err()
        return len(arr)

    def read_agents_by_id(self, ids, missing_ok=False):
        """`agents.get(&id)` (lib.rs:71) for a batch: the rows of read_agents() with these ids, in the order asked (an
        id may repeat), without reading the rest of the crowd.  missing_ok=False: an id that is not a live agent raises
        CrowdSimError ("unknown agent id").  missing_ok=True: returns (records, found) with `found` a bool mask; the
        record of a missing id is zero except for its id.  A read changes nothing (include/crowdstep_state.h)."""
        fn = state_fn(self._lib, self.backend, "cs_read_agents_by_id", "read_agents_by_id")
        rc, out, found = read_by_id(fn, self._engine, ids, missing_ok)
        if rc != 0:
            raise self._err()
        return (out, found) if missing_ok else out

    def remove_agents_by_id(self, ids):
        """`remove_agents(id)` (lib.rs:176-192) for a batch, in one pass over the crowd: the state, the events and the
        planner callbacks are those of remove_agents(ids[0]) ... remove_agents(ids[-1]).  All or nothing: an unknown id
        or an id given twice raises CrowdSimError and removes nothing.  Returns the number of agents removed."""
        fn = state_fn(self._lib, self.backend, "cs_remove_agents", "remove_agents_by_id")
        keys = id_batch(ids)
        rc = fn(self._engine, keys.ctypes.data_as(C.POINTER(C.c_uint64)), len(keys))
        self._agents_cache = None
        self._dispatch_events()
        if rc != 0:
            raise self._err()
        return len(keys)

    def _selection(self, selection, terms):
        if selection is not None and any(v is not None for v in terms.values()):
            raise CrowdSimError("give a Selection or its keywords, not both")
        return selection_struct(selection if selection is not None else Selection(**terms),
                                lambda p: self._planner_handles.get(id(p)))

    def select_agents(self, selection=None, *, rect=None, circle=None, source_sink=None, high_level_planner=None,
                      local_planner=None, waypoint=None, speed=None, limit=None):
        """`sim.agents.values().filter(..)` (lib.rs:71) on the device: the ids of the agents that satisfy every term
        given (see Selection), ascending, as a uint64 array ready for read_agents_by_id / remove_agents_by_id /
        set_targets.  `limit`: at most that many ids (the first ones).  A selection changes nothing
        (include/crowdstep_state.h)."""
        fn = state_fn(self._lib, self.backend, "cs_select_agents", "select_agents")
        sel = self._selection(selection, dict(rect=rect, circle=circle, source_sink=source_sink,
                                              high_level_planner=high_level_planner, local_planner=local_planner,
                                              waypoint=waypoint, speed=speed))
        n, ids = select_ids(fn, self._engine, sel, len(self) if limit is None else limit)
        if n is None:
            raise self._err()
        return ids

    def count_agents(self, selections):
        """How many agents each of up to 1024 selections (Selection objects or dicts of their keywords) selects, in one
        pass over the crowd: the occupancy of every door, cabin and zone per step.  -> uint64 array."""
        fn = state_fn(self._lib, self.backend, "cs_count_agents", "count_agents")
        rc, out = count_selected(fn, self._engine, list(selections), lambda p: self._planner_handles.get(id(p)))
        if rc != 0:
            raise self._err()
        return out

    def agent_field(self, origin, cell, shape, selection=None, velocity=False):
        """Where the crowd is and which way it flows, as a grid, in one pass over the agents on the device
        (cs_agent_field): `shape` = (ny, nx) bins of size `cell` (a scalar or a pair (w, h)) from the low corner
        `origin` = (x0, y0), independent of the simulation's grid.  Returns the number of agents per bin, uint32[ny, nx]
        and, with velocity=True, also the sums of their velocities, float64[ny, nx, 2] (mean flow = sum / count).
        `selection` (what count_agents accepts) rasterises only the agents it selects.  An agent is binned by the record
        read_agents() returns for it: ix = floor((x - x0) / w), in when 0 <= ix < nx (include/crowdstep_state.h).  A
        raster changes nothing."""
        fn = state_fn(self._lib, self.backend, "cs_agent_field", "agent_field")
        sel = None if selection is None else selection_struct(selection, lambda p: self._planner_handles.get(id(p)))
        rc, count, sums = field_raster(fn, self._engine, field_desc(origin, cell, shape), sel, velocity)
        if rc != 0:
            raise self._err()
        return (count, sums) if velocity else count

    def solve_flow_field(self, origin, cell, goals, speed, *, blocked=None, slowness=None, density_weight=0.0,
                         density_filter=None, planner=None, vectors=True, distance=False):
        """Solve a flow field on the device (cs_flow_field_solve, include/crowdstep_state.h): the preferred velocities
        that lead every bin of the raster (`origin`, `cell`, the shape (ny, nx) of `goals`) to its cheapest goal bin
        round the `blocked` bins, 8-connected, no corner cutting.  A step out of a bin costs its length times the bin's
        slowness, `slowness` (float32 (ny, nx), default 1) times 1 + density_weight * (the agents in the bin, those
        `density_filter` selects): a jam in front of one exit sends people to the other.  `planner`: a FieldPlanner of
        this raster, registered here; the vectors are written into its device samples behind the steps already queued,
        and with vectors=False and distance=False no raster crosses the bus.  The call waits for the device.
        -> (vectors float32 (ny, nx, 2) | None, dist float64 (ny, nx) | None, {"reached": bins with a path, "rounds"}).
        Distances are the same bits as flow_field_solve_host, which a library without the call falls back to."""
        return flow_solve_of(self, getattr(self._lib, "cs_flow_field_solve", None), self._engine,
                             lambda p: self._planner_handles.get(id(p)), origin, cell, goals, speed, blocked, slowness,
                             density_weight, density_filter, planner, vectors, distance)

    def close_pairs(self, distance, a=None, b=None, *, limit=None, distances=False):
        """The pairs of agents closer than `distance`, on the device (cs_close_pairs): contacts, overlaps, near misses.
        Returns a uint64[n, 2] array of (a, b) ids with a < b, every pair once, ascending; with distances=True also the
        float64[n] left-hand sides dx*dx + dy*dy.  Two agents are a pair iff dx*dx + dy*dy < distance*distance in f64 on
        the positions read_agents() reports, both inside the grid's rectangle (include/crowdstep_state.h).  `a`, `b`: the
        two roles of a pair, what select_agents accepts (a Selection, a dict of its keywords, None: everyone); a pair
        counts iff one of the two is in `a` and the other in `b`.  `limit`: at most that many pairs (the first ones);
        listing more than _abi.CS_PAIRS_MAX pairs raises, count_close_pairs has no limit.  Changes nothing."""
        fn = state_fn(self._lib, self.backend, "cs_close_pairs", "close_pairs")
        return close_pairs_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, distance, a, b,
                              limit, distances)

    def count_close_pairs(self, distance, a=None, b=None):
        """len(close_pairs(distance, a, b)) from one pass that lists nothing, exact whatever its size."""
        fn = state_fn(self._lib, self.backend, "cs_close_pairs", "close_pairs")
        handle_of = lambda p: self._planner_handles.get(id(p))  # noqa: E731
        n, _, _ = close_pairs_call(fn, self._engine, distance, None if a is None else selection_struct(a, handle_of),
                                   None if b is None else selection_struct(b, handle_of), 0, False)
        if n is None:
            raise self._err()
        return int(n)

    def agent_clusters(self, distance, members=None, *, min_size=1, limit=None):
        """Which agents hang together, on the device (cs_agent_clusters): jams, groups, contact chains.  The clusters are
        the connected components of the members under the links of close_pairs(distance, members, members); `members` is
        what select_agents accepts (None: everyone), and an agent that is no member bridges nobody.  Returns (ids
        uint64[n], labels uint64[n], table): the members of the reported clusters ascending by id, the label of each (the
        smallest id of its cluster), and a structured array (label, size, min_x, min_y, max_x, max_y, sum_x, sum_y) of the
        clusters ascending by label; the centroid is sum / size.  Only clusters of at least `min_size` members are
        reported; `limit`: at most that many entries of each list (the first ones).  Changes nothing."""
        fn = state_fn(self._lib, self.backend, "cs_agent_clusters", "agent_clusters")
        return agent_clusters_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, distance, members,
                                 min_size, limit)

    def count_clusters(self, distance, members=None, *, min_size=1):
        """(number of clusters, number of their members) of agent_clusters(distance, members, min_size=min_size), from a
        call that lists nothing."""
        fn = state_fn(self._lib, self.backend, "cs_agent_clusters", "agent_clusters")
        return count_clusters_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, distance, members,
                                 min_size)

    def agent_neighbours(self, distance, subjects=None, others=None, *, min_count=0, limit=None):
        """What surrounds each agent, on the device (cs_agent_neighbours): local density, violated personal space, the
        pedestrian closest to each robot.  For every subject (an agent `subjects` selects, None: everyone) the number of
        others (`others`, None: everyone; itself never) with dx*dx + dy*dy < distance*distance on the positions
        read_agents() reports, in f64, and the nearest of them (ties: the smallest id).  Returns a structured array (id,
        count, nearest, nearest_d2) ascending by id, of the subjects with count >= min_count (0: all, the isolated ones
        with nearest == _abi.CS_NO_NEIGHBOUR and nearest_d2 == inf); `limit`: at most that many rows (the first ones).
        Selections as for close_pairs.  Changes nothing."""
        fn = state_fn(self._lib, self.backend, "cs_agent_neighbours", "agent_neighbours")
        return agent_neighbours_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, distance, subjects,
                                   others, min_count, limit)[1]

    def count_agents_with_neighbours(self, distance, subjects=None, others=None, *, min_count=1):
        """len(agent_neighbours(distance, subjects, others, min_count=min_count)) from a pass that lists no row: how many
        people have somebody within 0.4 m, in one launch."""
        fn = state_fn(self._lib, self.backend, "cs_agent_neighbours", "agent_neighbours")
        return agent_neighbours_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, distance, subjects,
                                   others, min_count, 0)[0]

    def encounters(self, distance, horizon, range, a=None, b=None, *, limit=None):
        """Who comes close to whom in the near future, on the device (cs_encounters): the pairs of agents now closer than
        `range` whose closest approach within the next `horizon` seconds, both keeping the velocity read_agents()
        reports, is closer than `distance`.  Returns a structured array (a, b, t, d2) with a < b, every encounter once,
        ascending by (a, b): t the time of the closest approach in [0, horizon] (0: not approaching), d2 the squared
        distance then, both bit for bit the f64 rule of include/crowdstep_state.h.  `a`, `b`: the two roles of a pair, as
        for close_pairs.  `limit`: at most that many rows (the first ones); listing more than _abi.CS_PAIRS_MAX rows
        raises, count_encounters has no limit.  Changes nothing."""
        fn = state_fn(self._lib, self.backend, "cs_encounters", "encounters")
        return encounters_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, distance, horizon,
                             range, a, b, limit)[1]

    def count_encounters(self, distance, horizon, range, a=None, b=None):
        """len(encounters(distance, horizon, range, a, b)) from one pass that lists nothing, exact whatever its size."""
        fn = state_fn(self._lib, self.backend, "cs_encounters", "encounters")
        return encounters_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, distance, horizon,
                             range, a, b, 0)[0]

    def cast_rays(self, origins, directions, radius, *, t_max=np.inf, ignore=None, targets=None):
        """What does each ray hit first, on the device (cs_cast_rays): every agent is a disc of `radius` around the
        position read_agents() reports.  origins, directions: (n, 2) arrays; the point of ray k at t is origin + direction
        * t, the direction taken AS GIVEN (a unit direction makes t a distance).  t_max (hits with t < t_max count) and
        ignore (an agent id the ray passes through: the robot that casts it; None: nobody) are one value for all rays or
        one per ray.  targets: who can be hit (a selection as for select_agents; None: everyone).  Returns a structured
        array (id, t), row k for ray k: the first agent entered and where, bit for bit the f64 rule of
        include/crowdstep_state.h, of equal t the smaller id; (_abi.CS_NO_HIT, inf) for a ray that hits nobody.  Line of
        sight from A to B: origin A, direction B - A, t_max 1, ignore A; B is visible iff the hit is B.  Changes
        nothing."""
        fn = state_fn(self._lib, self.backend, "cs_cast_rays", "cast_rays")
        return cast_rays_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err,
                            rays_array(origins, directions, t_max, ignore), radius, targets, True)[1]

    def count_ray_hits(self, origins, directions, radius, *, t_max=np.inf, ignore=None, targets=None):
        """The number of rays of cast_rays(...) that hit somebody; no rows are written."""
        fn = state_fn(self._lib, self.backend, "cs_cast_rays", "cast_rays")
        return cast_rays_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err,
                            rays_array(origins, directions, t_max, ignore), radius, targets, False)[0]

    def leg_conflicts(self, legs, distance, speed_max, *, targets=None):
        """Who comes within `distance` of each timed leg first if the crowd keeps walking as it does now, on the device
        (cs_leg_conflicts).  legs: a LEG_DTYPE array (legs_array, paths_legs): a probe at (x0, y0) at time t0 moving with
        (vx, vy) until t1, seconds from now; (0, 0) is a wait; ignore is an agent id the leg passes through (the robot
        itself).  Agents at or above speed_max are not considered: the bound is what lets the device look no further than
        distance + speed_max * t1 from the leg, so pass the planners' top speed or more (inf: everyone, the whole grid is
        walked).  targets: who can conflict (a selection as for select_agents; None: everyone).  Returns a structured
        array (id, s), row k for leg k: the first agent and the seconds after t0 at which it comes within the distance,
        bit for bit the f64 rule of include/crowdstep_state.h, of equal s the smaller id; (_abi.CS_NO_HIT, inf) for a
        free leg.  Changes nothing."""
        fn = state_fn(self._lib, self.backend, "cs_leg_conflicts", "leg_conflicts")
        return leg_conflicts_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, legs, distance,
                                speed_max, targets, True)[1]

    def count_leg_conflicts(self, legs, distance, speed_max, *, targets=None):
        """The number of legs of leg_conflicts(...) with a conflict; no rows are written."""
        fn = state_fn(self._lib, self.backend, "cs_leg_conflicts", "leg_conflicts")
        return leg_conflicts_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, legs, distance,
                                speed_max, targets, False)[0]

    def path_conflict(self, waypoints, times, distance, speed_max, *, ignore=None, targets=None):
        """One timed polyline against the moving crowd: waypoints (k + 1, 2) reached at the non-decreasing finite `times`
        (the first >= 0), each piece a leg of leg_conflicts (a zero-duration piece is dropped, equal points over a positive
        duration are a wait).  Returns None, or (id, t, leg_index, (x, y)) of the first leg in path order that has a
        conflict: who, the time t = t0 + s from now, the leg (counted without the dropped ones) and where the probe is
        then."""
        return path_conflict_of(self.leg_conflicts, waypoints, times, distance, speed_max, ignore, targets)

    def leg_intervals(self, legs, distance, speed_max, *, targets=None, limit=None):
        """Everybody who comes within `distance` of each timed leg, and when, on the device (cs_leg_intervals): the
        arguments of leg_conflicts.  Returns a structured array (leg, id, s_in, s_out), ascending by (leg, id): agent id
        is within the distance of leg `leg` from t0 + s_in to t0 + s_out, s_out at most t1 - t0 (equal: it is still there
        when the leg ends); a row for exactly the (leg, agent) that conflict by the rule of leg_conflicts, s_in that
        rule's s, both times bit for bit the f64 rule of include/crowdstep_state.h.  limit: at most that many rows (the
        first ones); None lists all, and above _abi.CS_PAIRS_MAX raises, count_leg_intervals has no limit.  Changes
        nothing.  merge_leg_intervals turns the rows into the occupied spans of each leg."""
        fn = state_fn(self._lib, self.backend, "cs_leg_intervals", "leg_intervals")
        return leg_intervals_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, legs, distance,
                                speed_max, targets, limit)[2]

    def count_leg_intervals(self, legs, distance, speed_max, *, targets=None):
        """The number of rows of leg_intervals(...) per leg (uint64, one entry per leg), from one pass that lists
        nothing, exact whatever its size."""
        fn = state_fn(self._lib, self.backend, "cs_leg_intervals", "leg_intervals")
        return leg_intervals_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, legs, distance,
                                speed_max, targets, 0)[1]

    def free_intervals(self, points, t0, t1, distance, speed_max, *, ignore=None, targets=None):
        """When is each point free of the crowd: one waiting leg per point of points (n, 2) from t0 to t1 (scalars or one
        value per point, seconds from now) in one leg_intervals call.  Returns, per point, the list of (start, end)
        absolute times inside [t0, t1] during which nobody slower than speed_max is within `distance` of it, ascending."""
        return free_intervals_of(self.leg_intervals, points, t0, t1, distance, speed_max, ignore, targets)

    zones_array = staticmethod(zones_array)

    def zone_agents(self, polygons, *, filter=None, limit=None):
        """The agents inside each polygon zone, on the device (cs_zone_agents).  polygons: a list of (k, 2) arrays of
        (x, y) vertices, or the (zones, vertices) of zones_array; zones may overlap.  Returns (rows, counts): rows a
        structured array (zone, id) ascending by (zone, id), counts the full number of rows of each zone (uint64).  An
        agent is in a zone by the even-odd rule of include/crowdstep_state.h ("Agents in polygon zones"), in f64, bit for
        bit: a ring (x0,y0) (x1,y0) (x1,y1) (x0,y1) holds exactly the agents rect=(x0, y0, x1, y1) selects.  filter: a
        selection (as for select_agents) the agents must match too.  limit: at most that many rows (the first ones); None
        lists all, and above _abi.CS_PAIRS_MAX raises, count_zone_agents has no limit.  Changes nothing."""
        fn = state_fn(self._lib, self.backend, "cs_zone_agents", "zone_agents")
        _, counts, rows = zone_agents_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, polygons,
                                         filter, limit)
        return rows, counts

    def count_zone_agents(self, polygons, filter=None):
        """The number of agents in each zone of zone_agents(...) (uint64, one entry per zone), from one pass that lists
        nothing, exact whatever its size."""
        fn = state_fn(self._lib, self.backend, "cs_zone_agents", "zone_agents")
        return zone_agents_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, polygons, filter, 0)[1]

    def gate_crossings(self, gates, speed_max, *, filter=None, limit=None):
        """Who walks through each gate within its window, on the device (cs_gate_crossings).  gates: a GATE_DTYPE array
        (gates_array, path_gates): segments A -> B with a window t0 .. t1 in seconds from now.  Returns (rows, counts):
        rows a structured array (gate, dir, id, s, u) ascending by (gate, id): agent id crosses gate `gate` at t0 + s at
        the point A + u * (B - A) and ends on the left (dir +1) or the right (dir -1) of A -> B, if it keeps the velocity
        it has now; counts (n, 2) uint64, the full number of rows of each gate with dir +1 and with dir -1.  The rule is
        that of include/crowdstep_state.h ("Who crosses a line"), in f64, bit for bit.  Agents at or above speed_max are
        not considered.  `filter`: a selection (a dict of select_agents' terms, or a Selection) or None for everyone.
        `limit`: at most that many rows (the first ones); None lists all, and above _abi.CS_PAIRS_MAX raises,
        count_gate_crossings has no limit.  Changes nothing."""
        fn = state_fn(self._lib, self.backend, "cs_gate_crossings", "gate_crossings")
        _, counts, rows = gate_crossings_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, gates,
                                            speed_max, filter, limit)
        return rows, counts

    def count_gate_crossings(self, gates, speed_max, filter=None):
        """The number of rows of gate_crossings(...) per gate and direction ((n, 2) uint64: dir +1, dir -1), from one
        pass that lists nothing, exact whatever its size."""
        fn = state_fn(self._lib, self.backend, "cs_gate_crossings", "gate_crossings")
        return gate_crossings_of(fn, self._engine, lambda p: self._planner_handles.get(id(p)), self._err, gates, speed_max,
                                 filter, 0)[1]

    def remove_selected(self, selection=None, *, rect=None, circle=None, source_sink=None, high_level_planner=None,
                        local_planner=None, waypoint=None, speed=None):
        """remove_agents_by_id(select_agents(..)) in one call: the same agents gone, the same events and planner
        callbacks, in ascending id.  Returns the removed ids."""
        fn = state_fn(self._lib, self.backend, "cs_remove_selected", "remove_selected")
        sel = self._selection(selection, dict(rect=rect, circle=circle, source_sink=source_sink,
                                              high_level_planner=high_level_planner, local_planner=local_planner,
                                              waypoint=waypoint, speed=speed))
        n, ids = select_ids(fn, self._engine, sel, len(self))
        self._agents_cache = None
        self._dispatch_events()
        if n is None:
            raise self._err()
        return ids

    def set_targets(self, ids, goals, tolerance=(0.0, 0.0)):
        """`planner.set_target(&sim.agents[&id], goal, tolerance)` (rmf/mod.rs:217-236) for a batch, between steps: the
        calls are made in the order of the batch on the planner of each agent (a RouteFollower plans the first entry of
        every new (start, goal) hash pair and books it for the rest; a host planner's set_target is called).  `goals`:
        one (x, y) per id.  Returns one _abi.CS_TARGET_* status per entry (uint8).  All or nothing: an unknown id or a
        non-finite goal raises CrowdSimError with no planner called (include/crowdstep_state.h)."""
        fn = state_fn(self._lib, self.backend, "cs_set_targets", "set_targets")
        rc, status = set_targets_by_id(fn, self._engine, ids, goals, tolerance)
        if rc != 0:
            raise self._err()
        return status

    @property
    def targets_answered_on_device(self):
        """Entries of all set_targets calls so far whose (start, goal) pair the device's route book held: the host made
        no lookup for them (cs_set_targets_device_hits; on a tile of a mesh: NativeTileMesh.tile(k))."""
        fn = state_fn(self._lib, self.backend, "cs_set_targets_device_hits", "targets_answered_on_device")
        return int(fn(self._engine))

    def commit_agents(self):
        """Write back the entries of `agents` whose position, velocity or next_waypoint were edited since they were
        read (the reference's `agents.get_mut(&id).position = p`, made explicit).  Raises CrowdSimError if a field that
        cannot be written changed.  Returns the number of agents written."""
        if self._agents_cache is None:
            return 0
        rows, mask = edited_agents(self._agents_cache, self._agents_read)
        if not len(rows):
            return 0
        return self.write_agents(rows, mask)

    def __len__(self):
        return int(self._lib.cs_agent_count(self._engine))

    def get_neighbours_in_radius(self, radius, position):
        """SpatialIndex::get_neighbours_in_radius, location_hash_2d.rs:240-258."""
        cap = 256
        while True:
            out = np.zeros(cap, dtype=np.uint64)
            n = self._lib.cs_query_radius(self._engine, float(radius), float(position[0]),
                                          float(position[1]),
                                          out.ctypes.data_as(C.POINTER(C.c_uint64)), cap)
            if n <= cap:
                return [int(i) for i in out[:n]]
            cap = int(n)

    def get_nearest_neighbours(self, n, position):
        """SpatialIndex::get_nearest_neighbours, location_hash_2d.rs:151-238."""
        out = np.zeros(max(int(n), 1) + len(self), dtype=np.uint64)
        got = self._lib.cs_query_knn(self._engine, int(n), float(position[0]), float(position[1]),
                                     out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return [int(i) for i in out[:got]]

    def query_radius_batch(self, radii, positions, details=False):
        """n radius queries in one launch (cs_query_radius_batch).  -> list of id lists in the order of
        get_neighbours_in_radius; with details=True a list of (ids, squared distances, global cells)
        arrays per query (what a tile mesh needs to merge the answers of its tiles)."""
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.float64).reshape(-1, 2))
        n = len(pos)
        rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float64), (n,)))
        cap = 64
        while True:
            ids = np.zeros((n, cap), dtype=np.uint64)
            counts = np.zeros(n, dtype=np.uint64)
            d2 = np.zeros((n, cap), dtype=np.float32)
            cells = np.zeros((n, cap), dtype=np.uint32)
            rc = self._lib.cs_query_radius_batch(
                self._engine, n, pos.ctypes.data_as(C.POINTER(C.c_double)), rad.ctypes.data_as(C.POINTER(C.c_double)),
                cap, ids.ctypes.data_as(C.POINTER(C.c_uint64)), counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                d2.ctypes.data_as(C.POINTER(C.c_float)), cells.ctypes.data_as(C.POINTER(C.c_uint32)))
            if rc != 0:
                raise self._err()
            if n == 0 or counts.max() <= cap:
                break
            cap = int(counts.max())
        if details:
            return [(ids[i, :int(counts[i])].copy(), d2[i, :int(counts[i])].copy(), cells[i, :int(counts[i])].copy())
                    for i in range(n)]
        return [[int(v) for v in ids[i, :int(counts[i])]] for i in range(n)]

    def query_knn_batch(self, k, positions, details=False):
        """The k nearest agents of n points in one call (cs_query_knn_batch), nearest first, ties by id."""
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.float64).reshape(-1, 2))
        n, k = len(pos), int(k)
        ids = np.zeros((n, max(k, 1)), dtype=np.uint64)
        counts = np.zeros(n, dtype=np.uint64)
        d2 = np.zeros((n, max(k, 1)), dtype=np.float32)
        rc = self._lib.cs_query_knn_batch(self._engine, n, pos.ctypes.data_as(C.POINTER(C.c_double)), k,
                                          ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          d2.ctypes.data_as(C.POINTER(C.c_float)))
        if rc != 0:
            raise self._err()
        if details:
            return [(ids[i, :int(counts[i])].copy(), d2[i, :int(counts[i])].copy()) for i in range(n)]
        return [[int(v) for v in ids[i, :int(counts[i])]] for i in range(n)]

    # -- streaming view for renderers (lib.rs:71 read every frame, main.rs:112-128) --
    def request_snapshot(self):
        """Queue a copy of the live agents into pinned host memory behind the steps queued so
        far; returns at once, the next step overlaps the transfer."""
        if self._lib.cs_snapshot_request(self._engine) != 0:
            raise self._err()

    def snapshot(self, wait=True):
        """The most recently requested snapshot as a structured array view (x, y, vx, vy, id,
        next_waypoint; unordered) and the number of steps it was taken after, or None when it is
        not complete yet (wait=False) or nothing was requested.  The view is valid until the
        second request_snapshot() from now."""
        out = C.POINTER(_abi.SnapshotRecord)()
        n, step = C.c_size_t(0), C.c_uint64(0)
        rc = self._lib.cs_snapshot_acquire(self._engine, 1 if wait else 0, C.byref(out), C.byref(n),
                                           C.byref(step))
        if rc in (1, 2):
            return None
        if rc != 0:
            raise self._err()
        if n.value == 0:
            return np.zeros(0, dtype=_abi.SNAPSHOT_DTYPE), int(step.value)
        buf = (C.c_char * (n.value * C.sizeof(_abi.SnapshotRecord))).from_address(C.addressof(out.contents))
        return np.frombuffer(buf, dtype=_abi.SNAPSHOT_DTYPE), int(step.value)

    def spawn_probe_dev(self, dur, flags_ptr, n):
        """Tile engines, no host wait: flags (one int32 per sink) go to device memory at flags_ptr."""
        dt = dur.total_seconds() if isinstance(dur, datetime.timedelta) else float(dur)
        if self._lib.cs_spawn_probe_dev(self._engine, dt, C.c_void_p(flags_ptr), int(n)) != 0:
            raise self._err()

    def spawn_commit_dev(self, flags_ptr, n):
        if self._lib.cs_spawn_commit_dev(self._engine, C.c_void_p(flags_ptr), int(n)) != 0:
            raise self._err()

    @property
    def host_events_needed(self):
        """True when spawn / waypoint / destroy events must reach the host (listeners, host local planners)."""
        return bool(self._listeners) or self._host_lps

    # -- tiles (multi-GPU): halo hooks, see tiles.py --
    def halo_set_buffers(self, direction, send_ptr, recv_ptr, capacity_records):
        if self._lib.cs_halo_set_buffers(self._engine, int(direction), C.c_void_p(send_ptr),
                                         C.c_void_p(recv_ptr), int(capacity_records)) != 0:
            raise self._err()

    def halo_pack(self, axis):
        if self._lib.cs_halo_pack(self._engine, int(axis)) != 0:
            raise self._err()

    def halo_unpack(self, axis):
        if self._lib.cs_halo_unpack(self._engine, int(axis)) != 0:
            raise self._err()

    def halo_pack_all(self):
        if self._lib.cs_halo_pack_all(self._engine) != 0:
            raise self._err()

    def halo_unpack_all(self):
        if self._lib.cs_halo_unpack_all(self._engine) != 0:
            raise self._err()

    # -- tiles: re-cutting a running mesh (cs_tile_histogram / _export / _retile / _import) --
    def tile_histogram(self, rows, cols):
        """Adds this tile's owned agents per global x-row / y-column into the uint64 arrays."""
        if self._lib.cs_tile_histogram(self._engine, rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       cols.ctypes.data_as(C.POINTER(C.c_uint64))) != 0:
            raise self._err()

    def tile_export(self):
        """Every owned agent as a halo record: a (n, CS_HALO_RECORD_BYTES) uint8 array."""
        n = self._lib.cs_tile_export(self._engine, None, 0)
        if n == C.c_size_t(-1).value:
            raise self._err()
        buf = np.zeros((max(n, 1), _abi.CS_HALO_RECORD_BYTES), dtype=np.uint8)
        got = self._lib.cs_tile_export(self._engine, buf.ctypes.data_as(C.c_void_p), n)
        if got == C.c_size_t(-1).value:
            raise self._err()
        return buf[:min(n, got)]

    def tile_retile(self, rect):
        if self._lib.cs_tile_retile(self._engine, *[int(v) for v in rect]) != 0:
            raise self._err()
        self._agents_cache = None

    def tile_import(self, records):
        rec = np.ascontiguousarray(records, dtype=np.uint8)
        if len(rec) and self._lib.cs_tile_import(self._engine, rec.ctypes.data_as(C.c_void_p), len(rec)) != 0:
            raise self._err()
        self._agents_cache = None

    # -- tiles: route followers' set_target calls that missed the route book (cs_route_misses / _resolve) --
    def route_misses(self):
        n = self._lib.cs_route_misses(self._engine, None, 0)
        if n == 0:
            return []
        buf = (_abi.RouteMiss * n)()
        self._lib.cs_route_misses(self._engine, buf, n)
        return [(int(m.id), int(m.hlp), int(m.slot), m.px, m.py, m.tx, m.ty) for m in buf]

    def route_resolve(self, misses):
        buf = (_abi.RouteMiss * max(len(misses), 1))()
        for k, m in enumerate(misses):
            buf[k] = _abi.RouteMiss(*m)
        if self._lib.cs_route_resolve(self._engine, buf, len(misses)) != 0:
            raise self._err()

    # -- tiles: the RCCL transport of the C ABI (cs_rccl_*, cs_halo_exchange_rccl) --
    def rccl_unique_id(self):
        """Rank 0: the 128 bytes every rank passes to rccl_comm_init (ncclGetUniqueId)."""
        buf = (C.c_uint8 * _abi.CS_RCCL_UNIQUE_ID_BYTES)()
        if self._lib.cs_rccl_unique_id(buf) != 0:
            raise CrowdSimError("RCCL is not available (librccl.so.1)")
        return bytes(buf)

    def rccl_comm_init(self, n_ranks, rank, unique_id):
        buf = (C.c_uint8 * _abi.CS_RCCL_UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        if self._lib.cs_rccl_comm_init(self._engine, int(n_ranks), int(rank), buf) != 0:
            raise self._err()

    def halo_set_peers(self, peers):
        arr = (C.c_int32 * 8)(*[int(p) for p in peers])
        if self._lib.cs_halo_set_peers(self._engine, arr) != 0:
            raise self._err()

    def halo_exchange_rccl(self, axis=-1):
        if self._lib.cs_halo_exchange_rccl(self._engine, int(axis)) != 0:
            raise self._err()

    def allreduce_max_rccl(self, dev_ptr, n):
        if self._lib.cs_allreduce_max_i32_rccl(self._engine, C.c_void_p(dev_ptr), int(n)) != 0:
            raise self._err()

    def tile_step_rccl(self, dur, report=False):
        """One multi-GPU step of this tile in ONE call into the engine (cs_tile_step_rccl)."""
        dt = dur.total_seconds() if isinstance(dur, datetime.timedelta) else float(dur)
        rep = _abi.StepReport()
        rc = self._lib.cs_tile_step_rccl(self._engine, dt, C.byref(rep) if report else None)
        self._agents_cache = None
        if report:
            self.last_report = rep.as_dict()
        if rc != 0:
            raise self._err()

    def spawn_probe(self, dur):
        """Tile engines: which of MY source-sinks would spawn this step (uint8 flag per sink)."""
        dt = dur.total_seconds() if isinstance(dur, datetime.timedelta) else float(dur)
        # one flag per sink SLOT: a removed sink keeps its slot in the engine (registry.rs:16-21)
        flags = np.zeros(max(int(self._lib.cs_source_sink_slots(self._engine)), 1), dtype=np.uint8)
        n = self._lib.cs_spawn_probe(self._engine, dt, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     len(flags))
        if n == C.c_size_t(-1).value:
            raise self._err()
        return flags[:n]

    @property
    def device_bytes(self):
        """Device memory held by the engine (grows with capacity, never with steps or ids)."""
        return int(self._lib.cs_device_bytes(self._engine))

    def kernel_stat(self, which):
        """Diagnostics of the tiled kernel's work decomposition since creation (cs_kernel_stat):
        0 = windows that left the LDS path, 1 = windows walked in chunks; 2 / 3 = halo exchanges a tile with
        CS_CFG_TILE_OVERLAP issued ahead / could use."""
        return int(self._lib.cs_kernel_stat(self._engine, int(which)))

    @property
    def source_sink_slots(self):
        """Source-sink handles handed out so far (removed sinks keep their slot)."""
        return int(self._lib.cs_source_sink_slots(self._engine))

    def remove_agent_here(self, agent):
        """Tiles: remove `agent` if THIS engine holds it.  True = removed, False = not here;
        any other failure of the engine (poisoned, HIP error) raises."""
        rc = self._lib.cs_remove_agent(self._engine, int(agent))
        if rc == 0:
            self._agents_cache = None
            self._dispatch_events()
            return True
        if rc == 2:
            return False
        raise self._err()

    def spawn_commit(self, flags):
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        if self._lib.cs_spawn_commit(self._engine, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     len(flags)) != 0:
            raise self._err()

    # -- measurement --
    def profile_enable(self, kernel_mask=0xFFFFFFFF):
        """Bit k times kernel CS_K_k with hipEvents on the engine's stream; 0 = off."""
        self._lib.cs_profile_enable(self._engine, int(kernel_mask) & 0xFFFFFFFF)

    def profile_stride(self, every):
        """Time only every `every`-th launch of the enabled kernels."""
        self._lib.cs_profile_stride(self._engine, int(every))

    def profile_reset(self):
        self._lib.cs_profile_reset(self._engine)

    def profile_read(self):
        out = {}
        for k, name in enumerate(_abi.KERNEL_NAMES):
            ms, cnt = C.c_double(0), C.c_uint64(0)
            self._lib.cs_profile_read(self._engine, k, C.byref(ms), C.byref(cnt))
            out[name] = {"total_ms": ms.value, "launches": int(cnt.value)}
        return out
