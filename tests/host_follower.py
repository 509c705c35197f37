"""The follower of RMFPlanner (rmf/mod.rs:195-242) as HOST code: a HighLevelPlanner subclass in Python that the f64 oracle
runs through its CS_HLP_CALLBACK path (velocity per agent and step, set_target at spawn and at waypoints).  It is the
reference for Simulation.set_targets: a test calls `set_target(agent, goal, tol)` on it directly, agent by agent, as a
reference host calls `planner.set_target(&sim.agents[&id], goal, tol)`.

The arithmetic is the oracle's own (oracle/crowdstep_oracle.cpp, CS_HLP_ROUTE): sqrt(dx*dx + dy*dy), t / n * speed, the
hash round(v / scale) with ties away from zero.  tests/test_set_targets_abi.py pins it: the oracle with this object
equals the oracle with RouteFollower bit for bit."""
import math

from rmf_crowdsim_amd import HighLevelPlanner

BOOKED, PLANNED, NO_PATH = 1, 2, 3  # what a set_target call did (_abi.CS_TARGET_*)


def spatial_hash(v, scale):
    """SpatialHash::new, rmf/mod.rs:70-77: (v / scale).round() as i64 (round: ties away from zero)"""
    r = v / scale
    a = abs(r)
    f = math.floor(a)
    n = f + 1 if a - f >= 0.5 else f  # (a - f is exact)
    return int(-n if r < 0 else n)


class HostFollower(HighLevelPlanner):
    def __init__(self, plan_route, scale=1.0, arrive=0.1, speed=1.0):
        self.plan_route = plan_route
        self.scale, self.arrive, self.speed = float(scale), float(arrive), float(speed)
        self.agent_cache = {}              # id -> (route, next waypoint)
        self.route_list = []
        self.route_plans_by_location = {}  # (hash of start, hash of goal) -> route
        self.statuses = []                 # one per set_target call, in call order

    def get_desired_velocity(self, agent, time):  # rmf/mod.rs:197-215
        entry = self.agent_cache.get(agent.agent_id)
        if entry is None:
            return None
        route, wp = self.route_list[entry[0]], entry[1]
        px, py = float(agent.position[0]), float(agent.position[1])
        dx, dy = px - route[wp][0], py - route[wp][1]
        if math.sqrt(dx * dx + dy * dy) < self.arrive and len(route) > wp + 1:
            wp += 1
            self.agent_cache[agent.agent_id] = (entry[0], wp)
        tx, ty = route[wp][0] - px, route[wp][1] - py
        n = math.sqrt(tx * tx + ty * ty)
        if n == 0.0:  # normalize() on the waypoint itself: 0 / 0
            return (math.nan, math.nan)
        return (tx / n * self.speed, ty / n * self.speed)

    def set_target(self, agent, point, tolerance):  # rmf/mod.rs:217-236
        sx, sy = float(agent.position[0]), float(agent.position[1])
        gx, gy = float(point[0]), float(point[1])
        key = (spatial_hash(sx, self.scale), spatial_hash(sy, self.scale),
               spatial_hash(gx, self.scale), spatial_hash(gy, self.scale))
        route = self.route_plans_by_location.get(key)
        if route is not None:
            self.agent_cache[agent.agent_id] = (route, 0)
            self.statuses.append(BOOKED)
            return
        pts = self.plan_route((sx, sy), (gx, gy))
        if not pts:
            self.statuses.append(NO_PATH)  # "Failed to find contiguous path": the agent keeps what it had
            return
        self.route_plans_by_location[key] = len(self.route_list)
        self.agent_cache[agent.agent_id] = (len(self.route_list), 0)
        self.route_list.append([(float(p[0]), float(p[1])) for p in pts])
        self.statuses.append(PLANNED)

    def remove_agent_id(self, agent_id):  # rmf/mod.rs:239-241
        self.agent_cache.pop(agent_id, None)
