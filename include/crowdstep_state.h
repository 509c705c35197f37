/*
 * crowdstep_state.h — writing the crowd's state between steps (the HIP engine only).
 *
 * The reference's crowd state is a public, mutable map (`pub agents: HashMap<AgentId, Agent>`, lib.rs:71): a host
 * that drives the simulation writes to it directly (an actor teleported by a simulator integration, a robot modelled
 * as a crowd member whose position comes from elsewhere), and the next `step` works from what it wrote.  These calls
 * are that write, by agent id.
 *
 * This header is separate from crowdstep.h on purpose: it holds the engine's entry points that the test oracle
 * (oracle/crowdstep_oracle.cpp, frozen) does not implement.  crowdstep.h stays the ABI that both libraries export,
 * symbol for symbol, and that the Rust shim's ffi.rs mirrors exactly.
 *
 * Semantics ("Writing agents between steps"):
 *   - A write sets the START-OF-STEP state of existing agents.  The next step runs exactly as if the previous step had
 *     left them there: its neighbour queries, the spawn-occupancy probe (lib.rs:214) and the between-step queries
 *     (cs_query_*) all see the written positions.
 *   - Position (x, y): placed like cs_add_agents places the same point (location_to_index with its saturating casts and
 *     the alias of y beyond the row stride, then the f32 offset from the stored cell).
 *   - Velocity (vx, vy): stored as f32, as the step stores it.
 *   - next_waypoint: below the number of waypoints of the agent's source-sink while that sink is registered; 0 for
 *     any other agent.  Writing it does not call set_target and does not change a route follower's route (a get_mut
 *     in the reference).
 *   - eyesight_range of cs_agent_view is ignored (a per-group value on the device); orientation and angular_vel are
 *     not part of the view.
 *   - All or nothing: a refused batch changes nothing and does not poison the engine.  Refused are an id that is not a
 *     live indexed agent ("unknown agent id", as cs_remove_agent), an id given twice, a non-finite written value, a
 *     position the index refuses ("Index out of bounds"), an out-of-range next_waypoint, an empty or unknown field
 *     mask and, on a tile engine driven by hand, a position in a cell the tile does not own.
 *   - Ids are external ids (CS_CFG_WIDE_IDS: below or above a renumbering alike); a write never renumbers.
 *   - Steps queued without a report complete first (stream order); if one of them failed, the write returns that Err.
 *   - A write fires no events and leaves the last step report alone.
 * cs_agent_view makes read -> edit -> write a round trip: cs_read_agents, change the fields, cs_write_agents.
 */
#ifndef CROWDSTEP_STATE_H
#define CROWDSTEP_STATE_H

#include "crowdstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the fields a write sets (bits of `fields`) */
#define CS_WRITE_POSITION 1u
#define CS_WRITE_VELOCITY 2u
#define CS_WRITE_NEXT_WAYPOINT 4u

/* `agents.get_mut(&id)` for n agents at once (lib.rs:71).  0 = Ok, else Err (cs_last_error says why). */
int cs_write_agents(cs_engine*, const cs_agent_view* in, size_t n, uint32_t fields);
/* The same on a mesh.  Collective: every rank passes the same batch.  An agent written into a cell another tile owns
 * moves there (the record format of cs_tile_export).  A refused batch fails on every rank, with nothing applied. */
int cs_mesh_write_agents(cs_mesh*, const cs_agent_view* in, size_t n, uint32_t fields);

#ifdef __cplusplus
}
#endif
#endif /* CROWDSTEP_STATE_H */
