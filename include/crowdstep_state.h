/*
 * crowdstep_state.h — the crowd's state between steps, by agent id: write, read and remove in batches (the HIP engine
 * only).
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
 *
 * Reading and removing by id ("Reading and removing agents by id"): the other two uses of the map,
 * `agents.get(&id)` and `remove_agents(id)` (lib.rs:176-192), for a batch of ids at once.  One pass over the slots
 * matches the whole batch; the cost of a call does not grow with the columns of the crowd (the read) or with one scan
 * and one wait per id (the remove).
 *   - cs_read_agents_by_id: out[k] is the record cs_read_agents returns for ids[k] at the same moment, byte for byte,
 *     agents the index never took included.  An id may repeat.  A read changes nothing: the next step runs exactly as
 *     it would have.
 *   - cs_remove_agents: leaves the engine in the state cs_remove_agent(ids[0]) ... cs_remove_agent(ids[n-1]) leave it
 *     in: the same agents gone, the same DESTROYED events and planner remove_agent callbacks in the order of the batch.
 *     All or nothing: an id that is not a live agent ("unknown agent id", 2) or an id given twice (3) refuses the
 *     batch with nothing removed, no event, no callback, and the engine not poisoned.
 *   - Both: external ids under CS_CFG_WIDE_IDS; queued steps complete first and a failure of one of them is returned;
 *     on a tile engine whose arrays hold ghosts only owned agents match; n == 0 is Ok.
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


/* `agents.get(&id)` for n ids at once (lib.rs:71).  out[k] answers ids[k], in the order asked.
 * found == NULL: every id must be a live agent, else Err "unknown agent id" (2) and out is not written.
 * found != NULL: found[k] = 1 / 0; for a missing id out[k] is all zero except out[k].id = ids[k]; returns 0. */
int cs_read_agents_by_id(cs_engine*, const uint64_t* ids, size_t n, cs_agent_view* out, uint8_t* found);
/* `remove_agents(id)` (lib.rs:176-192) for n ids at once, all or nothing. */
int cs_remove_agents(cs_engine*, const uint64_t* ids, size_t n);
/* The same on a mesh.  Collective: every rank passes the same batch and gets the same answer (the read returns the
 * whole batch on every rank, as cs_mesh_read_agents returns the whole crowd).  The number of collectives does not
 * depend on n.  A refused batch fails on every rank, with nothing removed. */
int cs_mesh_read_agents_by_id(cs_mesh*, const uint64_t* ids, size_t n, cs_agent_view* out, uint8_t* found);
int cs_mesh_remove_agents(cs_mesh*, const uint64_t* ids, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CROWDSTEP_STATE_H */
