"""rmf_crowdsim_amd — MI355X-native engine for the `Simulation::step` hot path of rmf_crowdsim.

Host-side mirror of the reference trait surface over the C ABI of the HIP engine
(include/crowdstep.h, csrc/crowdstep_hip.hip).  There is no CPU fallback.
"""
from ._abi import (CS_CFG_DEFAULT, CS_CFG_DENSE, CS_CFG_FORCE_GATHER, CS_CFG_FORCE_TILED, CS_CFG_WIDE_IDS,
                   CS_WRITE_NEXT_WAYPOINT, CS_WRITE_POSITION, CS_WRITE_VELOCITY)
from .simulation import (Agent, CrowdGenerator, CrowdSimError, EventListener, FieldPlanner, HighLevelPlanner,
                         IdParityHighLevelPlan, LocalPlanner, LocationHash2D, MonotonicCrowd,
                         NoHighLevelPlan, NoLocalPlan, PoissonCrowd, RouteFollower, SeededPoissonCrowd, Selection,
                         Simulation, SourceSink, SpatialIndex,
                         StubHighLevelPlan, Zanlungo, flow_field_solve_host, flow_field_to_goals)

__all__ = [
    "Agent", "CrowdGenerator", "CrowdSimError", "EventListener", "FieldPlanner", "HighLevelPlanner",
    "IdParityHighLevelPlan", "LocalPlanner", "LocationHash2D", "MonotonicCrowd",
    "NoHighLevelPlan", "NoLocalPlan", "PoissonCrowd", "RouteFollower", "SeededPoissonCrowd", "Selection", "Simulation",
    "SourceSink", "SpatialIndex",
    "StubHighLevelPlan", "Zanlungo", "flow_field_solve_host", "flow_field_to_goals", "CS_CFG_DEFAULT", "CS_CFG_DENSE",
    "CS_CFG_FORCE_GATHER",
    "CS_CFG_FORCE_TILED", "CS_CFG_WIDE_IDS", "CS_WRITE_NEXT_WAYPOINT", "CS_WRITE_POSITION", "CS_WRITE_VELOCITY",
]
