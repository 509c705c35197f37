/*
 * crowdstep_state.h — the crowd's state between steps, by agent id: write, read, remove, send to goals in batches, select,
 * rasterise into a grid, list the pairs of agents within a distance of one another and cluster the agents by that distance
 * (the HIP engine only).
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
 *
 * Sending agents to goals ("Sending agents to goals between steps"): the planner half of the same
 * surface, `planner.set_target(&sim.agents[&id], goal, tol)` (rmf/mod.rs:217-236) as a host calls it for an evacuation,
 * a shift change, a visitor sent to a room, for a batch of (id, goal) entries at once.
 *   - cs_set_targets: the result is that of set_target(&agents[&ids[k]], goals[k], tol) made for k = 0 .. n-1 IN THE
 *     ORDER OF THE BATCH, on the planner of each agent's group.  Order matters for CS_HLP_ROUTE: the first entry of a new
 *     (SpatialHash(start), SpatialHash(goal)) pair calls route_plan with ITS exact position and goal, later entries of the
 *     same pair (in this batch or any later one) take that route from the book (rmf/mod.rs:222-233).  Routes are numbered
 *     in that order.
 *   - `start` is the agent's position as cs_read_agents reports it at that moment: the device's book lookup and the
 *     host's planning hash the very same f64 value.
 *   - The agent's agent_cache entry becomes (route, waypoint 0); velocity, position and next_waypoint are untouched.  The
 *     tolerance is passed on to CALLBACK planners and ignored by ROUTE (as the reference ignores it).
 *   - An id may appear more than once: the calls are made in order, so the last entry decides the agent's route while
 *     earlier ones still plan and book theirs.
 *   - Agents of source-sinks may be sent too.  Their next_waypoint stays; when they reach the sink's waypoint the step's
 *     own set_target takes over again, as in the reference.
 *   - All or nothing, decided before any planner is called: an id that is not a live indexed agent ("unknown agent id",
 *     2; agents the index never took included, as for the write), a non-finite goal or tolerance, null arrays with n > 0
 *     (3).  A refused batch calls no route_plan and no callback, leaves the route book as it was and does not poison the
 *     engine.  n == 0 is Ok.
 *   - External ids under CS_CFG_WIDE_IDS; the call never renumbers.  Queued steps complete first and a failure of one of
 *     them is returned.  No events; the last step report is left alone.  On a tile engine an exchange made ahead
 *     (CS_CFG_TILE_OVERLAP) is void afterwards, as after every other change between steps (route state travels in halo
 *     records).
 *
 * Selecting agents ("Selecting agents between steps"): the fourth use of the map, iterating it with a
 * condition (`sim.agents.values().filter(..)`), which is how a host gets the ids the calls above start from.
 *   - A cs_selection is an AND of terms (CS_SEL_*).  Every term is evaluated on the record cs_read_agents returns for
 *     the agent at that moment: x, y the reported f64 position, vx, vy the f32 velocity widened to f64, all arithmetic and
 *     comparisons in f64, each product and sum rounded once.  cs_select_agents(sel) is exactly the ids of the records of
 *     cs_read_agents that satisfy the expressions written next to the CS_SEL_* bits, ascending.  A NaN coordinate or
 *     velocity fails every comparison it takes part in.
 *   - Agents the index never took are judged by the same rule on the record cs_read_agents lists for them.  On a tile
 *     engine whose arrays hold ghosts only owned agents count.
 *   - Refused with 3 (SIZE_MAX where the result is a count), nothing done, the engine usable: unknown term bits, a NaN in
 *     a field a set term reads (+-inf are fine), r < 0, null pointers with a non-zero count, more than CS_SELECT_MAX
 *     selections in one counting call.  Unknown planner or sink handles select nobody, as do x1 <= x0 and wp_hi < wp_lo.
 *   - Queued steps complete first and a failure of one of them is the call's; external ids under CS_CFG_WIDE_IDS; a
 *     selection or a count never renumbers and clears no flag of the engine: the next step runs exactly as it would have.
 *
 * Rasterising the crowd ("Rasterising the crowd between steps"): the read every consumer of a crowd
 * makes every step, where the people are and which way they flow, as a grid: a costmap layer, a density heatmap, level of
 * service, jam detection.  cs_agent_field costs one pass over the agents whatever the number of bins.
 *   - The raster is a cs_field_desc: nx * ny bins of cell_w x cell_h from the low corner (x0, y0), independent of the
 *     simulation's grid.  Every output holds nx * ny values, bin (ix, iy) at iy * nx + ix.
 *   - An agent is the record cs_read_agents returns for it at that moment: x, y the reported f64 position, vx, vy the f32
 *     velocity widened to f64.  fx = (x - x0) / cell_w in f64: one subtraction and one correctly rounded division, no
 *     reciprocal, no contraction.  The agent is inside along x iff 0 <= fx && fx < nx (a NaN or an infinity is outside),
 *     and then ix = (uint32_t)fx; the same for y with y0, cell_h, ny.  So an agent exactly on x0 is in bin 0, one exactly
 *     on an inner edge is in the upper bin, one exactly on x0 + nx * cell_w is outside.  An agent outside on either axis,
 *     or failing `filter` (a cs_selection, judged as for cs_select_agents; NULL: every agent), contributes nothing.
 *   - out_count[bin] is exact.  out_sum_vx / out_sum_vy[bin] are the f64 sums of the widened velocities of the bin's
 *     agents, added in any order: a bin without agents is exactly +0.0, a bin with one agent holds its velocity exactly
 *     (a zero sum has the sign +), a bin with n agents is within n * 2^-52 * sum|v| of the exactly rounded sum (twice the
 *     bound of recursive summation of n terms in any order).  IEEE propagation holds: an agent with a NaN velocity is
 *     counted and makes the sums of its bin NaN.
 *   - An output may be NULL; at least one must be given, and the two sums come together or not at all.  The velocities
 *     are not loaded when only counts are asked for and the filter has no speed term.
 *   - Agents the index never took are binned by the same rule on the record cs_read_agents lists for them.  On a tile
 *     engine whose arrays hold ghosts only owned agents count.
 *   - Refused with 3, the outputs untouched, the engine or mesh usable: a null description, a non-finite x0, y0, cell_w or
 *     cell_h, cell_w or cell_h <= 0, nx or ny == 0, nx * ny > CS_FIELD_MAX_CELLS, no output, one sum without the other, a
 *     filter cs_select_agents refuses.
 *   - Queued steps complete first and a failure of one of them is the call's; no events; the last step report is left
 *     alone; nothing is renumbered and no flag of the engine is cleared: the next step runs exactly as it would have.
 *
 * Pairs of agents between steps ("Pairs of agents between steps"): the questions about TWO agents,
 * how many overlap (closer than 2 * agent_radius), which pedestrians are within 0.5 m of a robot the host writes into the
 * crowd, which pairs were within 1.5 m step after step.  cs_close_pairs answers them on the device from the cell-sorted
 * arrays; nothing of the crowd comes to the host but the pairs asked for.
 *   - An agent is the record cs_read_agents returns for it at that moment: x, y the reported f64 position.
 *   - An agent TAKES PART iff its reported position is finite and inside the grid's own rectangle,
 *     gx0 <= x && x < gx1 && gy0 <= y && y < gy1, the corners being the f64 values cs_read_agents would report for the
 *     low corner of cell (0, 0) and of the cell one beyond the last row and the last column: gx0 = offset_x,
 *     gx1 = offset_x + rows * cell_size with rows = (size_t)(height / cell_size) (the index runs x over that many rows),
 *     gy0 = offset_y, gy1 = offset_y + stride * cell_size with stride = (size_t)(width / cell_size).  On a tile engine
 *     and on a mesh the rectangle is the GLOBAL grid's.  So no part take: agents the index never took, agents clamped
 *     into row or column 0 from below the low edge, agents aliased beyond the row stride, agents with a NaN position.
 *     The last three are exactly the agents whose stored offset does not lie in the cell they are indexed under, which
 *     is why the search of ceil(distance / cell_size) + 1 cells each way finds every pair.
 *   - Two agents p and q that both take part are a PAIR iff dx * dx + dy * dy < distance * distance with dx = x_p - x_q,
 *     dy = y_p - y_q: f64, every difference, product and sum rounded once (no contraction), the comparison strict like
 *     the index and CS_SEL_CIRCLE.  The expression is symmetric.  distance = +inf: every two participants are a pair;
 *     distance = 0: no pair, even for two agents on one point.
 *   - Roles: sel_a and sel_b are cs_selection values judged exactly as for cs_select_agents, NULL: everyone.  A pair is
 *     reported iff (A(p) && B(q)) || (A(q) && B(p)).  Robots against everyone: sel_a = the robots' local-planner handle
 *     (CS_SEL_LP), sel_b = NULL.
 *   - The answer: every pair once, as (a, b) with a < b (external ids under CS_CFG_WIDE_IDS), in ascending order of
 *     (a, b).  The call returns the full count and writes the first min(count, cap) pairs; out_d2[k] (optional) is the
 *     left-hand side of pair k, bit for bit.
 *   - out_pairs == NULL or cap == 0: the count only, from one pass that materialises nothing, exact whatever its size
 *     (92,700 agents within reach of one another are more than 2^32 pairs).
 *   - With cap > 0 a count above CS_PAIRS_MAX is refused (SIZE_MAX, "too many pairs to list", the engine usable): the
 *     sorted prefix needs every pair materialised.  The device scratch of a listing is kept while it is at most 16 MiB
 *     (and then part of cs_device_bytes); a larger one is freed before the call returns.
 *   - Refused with SIZE_MAX, nothing written, the engine or mesh usable: a NaN or negative distance, a selection
 *     cs_select_agents refuses, out_d2 without out_pairs.
 *   - Queued steps complete first and a failure of one of them is the call's; no events; the last step report is left
 *     alone; nothing is renumbered.  The call may sort the arrays by cell, as the spatial queries do: the next step runs
 *     to the same bytes as on an engine that never made the call.  On a tile engine whose arrays hold ghosts only owned
 *     agents take part.
 *
 * Clusters of agents between steps ("Clusters of agents between steps"): the question about MANY
 * agents, which of them hang together: which stalled agents form one jam, how big it is and where, which pedestrians
 * walk as a group, which blob blocks a corridor, who is in one contact chain.  cs_agent_clusters answers with the
 * connected components of the graph cs_close_pairs defines, merged on the device; what comes to the host is one label per
 * agent and 64 bytes per cluster, never a pair.
 *   - An agent is the record cs_read_agents returns for it at that moment: x, y the reported f64 position.
 *   - An agent is a MEMBER iff it takes part by the rule of cs_close_pairs (a finite reported position inside the grid's
 *     own rectangle, gx0 <= x && x < gx1 && gy0 <= y && y < gy1) and satisfies `members`, a cs_selection judged exactly
 *     as for cs_select_agents, NULL: everyone.  On a tile engine whose arrays hold ghosts only owned agents are members.
 *     Agents the index never took are no members.
 *   - Two members p and q are LINKED iff they are a pair of cs_close_pairs(distance, members, members): dx * dx + dy * dy <
 *     distance * distance with dx = x_p - x_q, dy = y_p - y_q, f64, every difference, product and sum rounded once (no
 *     contraction, no f32 pre-reject), the comparison strict.
 *   - A CLUSTER is a connected component of the members under the links.  A member without a link is a cluster of size 1.
 *     An agent that is no member never bridges two members, however close it stands to both.  distance = 0: every member
 *     is its own cluster, even two on one point; distance = +inf: all members are one cluster.
 *   - A cluster's LABEL is the smallest id among its members (external ids under CS_CFG_WIDE_IDS), so it depends neither
 *     on the order of the slots, nor on tiles, nor on the order in which the device merged.
 *   - min_size: only clusters with at least min_size members are reported, in both outputs and both counts; 0 and 1 both
 *     report every cluster.
 *   - The answer: *n_agents = the members of reported clusters; out_ids gets the first min(*n_agents, agent_cap) of their
 *     ids, ascending, and out_labels[k] the label of out_ids[k].  *n_clusters = the reported clusters; out_clusters gets
 *     the first min(*n_clusters, cluster_cap) of them, ascending by label.  Nothing is written beyond those entries.
 *   - Of a cs_cluster, label, size, min_x, min_y, max_x, max_y (the box of the members' reported positions) are exact.
 *     sum_x / sum_y are the f64 sums of the members' reported positions, added in any order: a cluster of one member
 *     holds its position exactly, a cluster of n members is within n * 2^-52 * sum|x| of the exactly rounded sum (the
 *     bound of cs_agent_field).  The centroid is sum / size.
 *   - Every pointer among the outputs and the two counts may be NULL (out_ids may be given without out_labels); with all
 *     of them NULL the call only validates.
 *   - Refused with 3, nothing written, the engine or mesh usable: a NaN or negative distance, a selection
 *     cs_select_agents refuses, out_labels without out_ids.
 *   - Queued steps complete first and a failure of one of them is the call's; no events; the last step report is left
 *     alone; nothing is renumbered.  The call may sort the arrays by cell, as the spatial queries do: the next step runs
 *     to the same bytes as on an engine that never made the call.  The device scratch of a call is kept while it is at
 *     most 16 MiB (the scratch of cs_close_pairs, part of cs_device_bytes); a larger one is freed before the call returns.
 *
 * Neighbours of each agent between steps ("Neighbours of each agent between steps"): the question
 * about EACH agent and its surroundings: how many people stand within 1 m of this person (local density), whose personal
 * space is violated right now, which pedestrian is closest to each robot and how far, how many agents have nobody within
 * 3 m.  cs_agent_neighbours answers on the device from the cell-sorted arrays; what comes to the host is at most one
 * 32-byte row per agent, never a pair.
 *   - An agent is the record cs_read_agents returns for it at that moment: x, y the reported f64 position.
 *   - It TAKES PART by the rule of cs_close_pairs: a finite reported position inside the grid's own rectangle; on a tile
 *     engine and on a mesh the rectangle is the GLOBAL grid's.  A SUBJECT is a participant that satisfies `subjects`, an
 *     OTHER a participant that satisfies `others`, both judged exactly as for cs_select_agents, NULL: everyone.  Agents
 *     the index never took, clamped agents, aliased agents and NaN agents are neither subject nor other.  On a tile engine
 *     whose arrays hold ghosts only owned agents are subjects or others.
 *   - An other q != p is a NEIGHBOUR of subject p iff dx * dx + dy * dy < distance * distance with dx = x_p - x_q,
 *     dy = y_p - y_q: f64, every difference, product and sum rounded once (no contraction, no f32 pre-reject), the
 *     comparison strict.  This is the expression of cs_close_pairs: with subjects == others == NULL the counts of all rows
 *     sum to exactly 2 * cs_close_pairs(distance, NULL, NULL).  A subject that is also an other does not count itself.
 *     Two agents on one point are neighbours for any distance > 0, with nearest_d2 == +0.0.  distance = 0: every subject
 *     has count 0.  distance = +inf: every other but itself is a neighbour (on a single engine; a mesh of more than one
 *     tile refuses +inf, as for the pairs).
 *   - `nearest` is the neighbour with the smallest nearest_d2, among equal values the one with the smallest id (external
 *     ids under CS_CFG_WIDE_IDS; ascending device id is ascending external id).  So the row depends neither on the order
 *     of the slots, nor on tiles, nor on the order of the walk.
 *   - min_count: a subject is REPORTED iff count >= min_count; 0 reports every subject, the isolated ones included.
 *   - The answer: the call returns the number of reported subjects and writes the first min(that, cap) rows, ascending by
 *     id.  Nothing is written beyond them.
 *   - out == NULL or cap == 0: the number only, from a pass that materialises no row (one 64-bit tally per workgroup):
 *     "how many people have somebody within 0.4 m" in one launch.
 *   - Refused with SIZE_MAX, nothing written, the engine or mesh usable: a NaN or negative distance, a selection
 *     cs_select_agents refuses, and on a mesh of more than one tile a distance above halo_cells * cell_size.  There is no
 *     limit in the style of CS_PAIRS_MAX: the answer never exceeds one row per agent.
 *   - Queued steps complete first and a failure of one of them is the call's; no events; the last step report is left
 *     alone; nothing is renumbered.  The call may sort the arrays by cell, as the spatial queries do: the next step runs
 *     to the same bytes as on an engine that never made the call.  The device scratch of a call is kept while it is at
 *     most 16 MiB (the scratch of cs_close_pairs, part of cs_device_bytes); a larger one is freed before the call returns.
 *
 * Encounters between steps ("Encounters between steps"): the questions about the NEAR FUTURE of two
 * agents: which pedestrians will come within 0.5 m of this robot in the next 3 s, how soon and how close; the same over
 * all pairs for a conflict monitor, a near-miss statistic, a door interlock.  cs_encounters answers with the closest
 * approach of every pair within a horizon, both agents keeping the velocity they have now (the time to closest approach
 * the Zanlungo planner is built on); nothing of the crowd comes to the host but the rows asked for.
 *   - An agent is the record cs_read_agents returns for it at that moment: x, y the reported f64 position, vx, vy the f32
 *     velocity widened to f64.
 *   - Who TAKES PART and the roles sel_a / sel_b are exactly those of cs_close_pairs: a finite position inside the grid's
 *     own rectangle (on a tile engine and on a mesh the GLOBAL grid's), owned agents only on a tile whose arrays hold
 *     ghosts, the selections judged as for cs_select_agents, NULL: everyone; a pair is reported iff
 *     (A(p) && B(q)) || (A(q) && B(p)).
 *   - For two participants p and q, every operation one f64 operation rounded once (no contraction, no reciprocal, no f32
 *     pre-reject; the division is the correctly rounded one):
 *         rx = x_q - x_p        ry = y_q - y_p
 *         wx = vx_q - vx_p      wy = vy_q - vy_p
 *         d2 = rx*rx + ry*ry                      IN RANGE   iff d2 < range*range   (the left-hand side of cs_close_pairs)
 *         ww = wx*wx + wy*wy    rw = rx*wx + ry*wy
 *         t  = 0                       if !(rw < 0)       (not approaching; equal velocities; a NaN)
 *         t  = -rw / ww, then horizon if !(t < horizon)   otherwise
 *         cx = rx + wx*t        cy = ry + wy*t
 *         m2 = cx*cx + cy*cy                      ENCOUNTER  iff in range && m2 < distance*distance
 *     Swapping p and q negates r, w and c exactly, so t, d2 and m2 are the same bits either way: the answer depends
 *     neither on the order of the slots nor on tiles.  Non-finite velocities fall wherever IEEE puts them
 *     (cs_write_agents refuses them).
 *   - horizon = 0: exactly the pairs of cs_close_pairs(min(distance, range)), with m2 == d2.  distance = +inf: every
 *     in-range pair with a finite m2.  range = 0 or distance = 0: none.  horizon = +inf and range = +inf are allowed (on
 *     one engine; a mesh of more than one tile refuses a range above halo_cells * cell_size).
 *   - The answer: every encounter once, as a cs_encounter (a, b, t, d2) with a < b (external ids under CS_CFG_WIDE_IDS),
 *     t and d2 = m2 bit for bit, in ascending order of (a, b).  The call returns the full count and writes the first
 *     min(count, cap) rows, and nothing beyond them.
 *   - out == NULL or cap == 0: the 64-bit count only, from one pass that materialises nothing.
 *   - With cap > 0 a count above CS_PAIRS_MAX is refused (SIZE_MAX, "too many encounters to list", the engine usable).
 *   - Refused with SIZE_MAX, nothing written, the engine or mesh usable: a NaN or negative distance, horizon or range, a
 *     selection cs_select_agents refuses, and on a mesh of more than one tile a range above halo_cells * cell_size.
 *   - Queued steps complete first and a failure of one of them is the call's; no events; the last step report is left
 *     alone; nothing is renumbered.  The call may sort the arrays by cell, as the spatial queries do: the next step runs
 *     to the same bytes as on an engine that never made the call.  The device scratch of a listing is kept while it is at
 *     most 16 MiB (the scratch of cs_close_pairs, part of cs_device_bytes); a larger one is freed before the call returns.
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

/* what happened to entry k of cs_set_targets (the optional out array) */
#define CS_TARGET_IGNORED   0u /* the agent's planner takes no targets: NONE, CONSTANT, ID_PARITY
                                  (their set_target does nothing, lib.rs:413-415), or ROUTE without route_plan */
#define CS_TARGET_BOOKED    1u /* ROUTE: the (start, goal) hash pair was in the route book, be it
                                  through an earlier entry of this very batch                       */
#define CS_TARGET_PLANNED   2u /* ROUTE: route_plan was called and its route added to the book      */
#define CS_TARGET_NO_PATH   3u /* ROUTE: route_plan returned 0, or the engine's route table is full
                                  (4,194,302 routes); the agent keeps what it had, nothing is booked */
#define CS_TARGET_FORWARDED 4u /* CALLBACK: the host planner's set_target was called                */

/* `planner.set_target(&agents[&ids[k]], goals[k], tol)` (rmf/mod.rs:217-236) for k = 0 .. n-1, in that order, all or
 * nothing.  goals_xy holds n (x, y) pairs; out_status (n bytes, CS_TARGET_*) may be NULL. */
int cs_set_targets(cs_engine*, const uint64_t* ids, const double* goals_xy, size_t n, double tol_x, double tol_y,
                   uint8_t* out_status);
/* The same on a mesh.  Collective: every rank passes the same batch and gets the same statuses.  The positions of all
 * entries are gathered (the number of collectives does not depend on n) and every tile runs the book part for the whole
 * batch in batch order, so that every tile's book numbers routes alike, assigning only to the agents it owns: route_plan
 * is called once per tile and new route, as by cs_route_resolve.  CALLBACK planners are called by the owning tile only,
 * in batch order, and BEFORE the route_plan calls of the batch (one engine interleaves the two kinds in batch order).
 * A refused batch fails on every rank, with no planner called. */
int cs_mesh_set_targets(cs_mesh*, const uint64_t* ids, const double* goals_xy, size_t n, double tol_x, double tol_y,
                        uint8_t* out_status);
/* How many entries of all cs_set_targets calls on this engine (for a mesh: on this tile, cs_mesh_tile) found their
 * (start, goal) pair in the device's copy of the route book, so that the host made no lookup for them. */
uint64_t cs_set_targets_device_hits(cs_engine*);

/* the terms of a selection (bits of cs_selection::terms, ANDed) */
#define CS_SEL_RECT         1u  /* x0 <= x < x1  &&  y0 <= y < y1                                   */
#define CS_SEL_CIRCLE       2u  /* (x-cx)*(x-cx) + (y-cy)*(y-cy) < r*r   (strict, like the index)   */
#define CS_SEL_SOURCE_SINK  4u  /* spawned by source-sink handle `source_sink`, removed or not;
                                   UINT32_MAX: the agents no sink spawned (cs_add_agents)            */
#define CS_SEL_HLP          8u  /* high-level planner handle                                         */
#define CS_SEL_LP          16u  /* local planner handle                                              */
#define CS_SEL_WAYPOINT    32u  /* wp_lo <= next_waypoint <= wp_hi                                   */
#define CS_SEL_SPEED       64u  /* speed_lo*speed_lo <= vx*vx + vy*vy < speed_hi*speed_hi            */
#define CS_SELECT_MAX 1024u     /* selections in one cs_count_agents call */
typedef struct cs_selection {
  uint32_t terms;                 /* CS_SEL_* bits, ANDed; 0 selects every agent */
  uint32_t source_sink, hlp, lp;
  double x0, y0, x1, y1;
  double cx, cy, r;
  uint64_t wp_lo, wp_hi;
  double speed_lo, speed_hi;
} cs_selection;

/* ids of the selected agents, ascending.  Returns the full count and writes min(count, cap) ids (the first ones);
 * out_ids == NULL or cap == 0: the count only.  SIZE_MAX on error. */
size_t cs_select_agents(cs_engine*, const cs_selection* sel, uint64_t* out_ids, size_t cap);
/* out_counts[k] = number of agents selections[k] selects, for n <= CS_SELECT_MAX selections in ONE pass over the crowd:
 * the occupancy of every door, cabin and zone of a building per step.  0 = Ok. */
int cs_count_agents(cs_engine*, const cs_selection* selections, size_t n, uint64_t* out_counts);
/* cs_remove_agents(cs_select_agents(sel)): the same agents gone, the same DESTROYED events and planner callbacks, in
 * ascending id.  Returns the number removed (and writes up to cap of their ids, optional).  SIZE_MAX on error. */
size_t cs_remove_selected(cs_engine*, const cs_selection* sel, uint64_t* out_ids, size_t cap);
/* The same on a mesh.  Collective: every rank passes the same selection(s) and gets the whole answer; the number of
 * collectives does not depend on the crowd or on the size of the answer. */
size_t cs_mesh_select_agents(cs_mesh*, const cs_selection* sel, uint64_t* out_ids, size_t cap);
int cs_mesh_count_agents(cs_mesh*, const cs_selection* selections, size_t n, uint64_t* out_counts);
size_t cs_mesh_remove_selected(cs_mesh*, const cs_selection* sel, uint64_t* out_ids, size_t cap);

#define CS_FIELD_MAX_CELLS 4194304u /* nx * ny of one raster */
typedef struct cs_field_desc {
  double x0, y0;          /* the low corner of bin (0, 0), world coordinates     */
  double cell_w, cell_h;  /* bin size, finite and > 0; independent of the grid's */
  uint32_t nx, ny;        /* bins along x and y, each >= 1                       */
} cs_field_desc;
/* Per bin of the raster: the number of agents (out_count) and the f64 sums of their velocities (out_sum_vx, out_sum_vy),
 * nx * ny values each, bin (ix, iy) at iy * nx + ix, in ONE pass over the crowd.  filter == NULL: every agent.  An output
 * may be NULL (the sums only together).  0 = Ok. */
int cs_agent_field(cs_engine*, const cs_field_desc* desc, const cs_selection* filter, uint32_t* out_count,
                   double* out_sum_vx, double* out_sum_vy);
/* The same on a mesh.  Collective: every rank passes the same arguments and gets the whole raster, the counts the same
 * bytes on every rank.  Every tile rasterises the agents it owns; a rank sends, per local tile, the bounding box of the
 * bins that tile touched and that part of its raster, never a whole raster: what travels does not grow with the crowd,
 * and the number of collectives depends neither on the raster nor on the crowd.  The parts are added in (rank, local
 * tile) order on every rank, the agents the index never took last.  A tile that fails makes every rank return Err. */
int cs_mesh_agent_field(cs_mesh*, const cs_field_desc* desc, const cs_selection* filter, uint32_t* out_count,
                        double* out_sum_vx, double* out_sum_vy);
/* Bytes this rank contributed to the gather of the last cs_mesh_agent_field (in one process: what it would have sent). */
uint64_t cs_mesh_field_gather_bytes(const cs_mesh*);

#define CS_PAIRS_MAX (1u << 26) /* pairs one listing may hold */
typedef struct cs_id_pair { uint64_t a, b; } cs_id_pair;   /* a < b */
/* The pairs of agents closer than `distance`, ascending by (a, b).  Returns the full count and writes min(count, cap)
 * pairs (the first ones) and, if asked, their squared distances; out_pairs == NULL or cap == 0: the count only (64-bit
 * on the device, no limit).  sel_a / sel_b: the two roles of a pair, NULL: everyone.  SIZE_MAX on error. */
size_t cs_close_pairs(cs_engine*, double distance, const cs_selection* sel_a, const cs_selection* sel_b,
                      cs_id_pair* out_pairs, double* out_d2, size_t cap);
/* The same on a mesh.  Collective: every rank passes the same arguments and gets the whole answer, byte for byte the
 * single engine's.  On a mesh of more than one tile `distance` is at most halo_cells * cell_size (so +inf is refused
 * there, too).  No halo exchange is made for it and the step's own exchange state is left as it is: every tile lists
 * the pairs among the agents it holds and exports a record (id, position, roles, tile) of each participant within reach
 * of an edge behind which another tile lies; one gather brings these band records to every rank, each rank tests its
 * tiles' band agents against the records of the tiles with a higher index (every cross-tile pair exactly once), one more
 * gather moves the pair lists (the count-only form: the counts), and every rank merges the sorted runs.  The number of
 * collectives depends neither on the crowd nor on the answer.  A tile that fails makes every rank return SIZE_MAX. */
size_t cs_mesh_close_pairs(cs_mesh*, double distance, const cs_selection* sel_a, const cs_selection* sel_b,
                           cs_id_pair* out_pairs, double* out_d2, size_t cap);

typedef struct cs_cluster {      /* 64 bytes */
  uint64_t label, size;                /* the smallest id among the members; their number       */
  double min_x, min_y, max_x, max_y;   /* of the members' reported positions: exact              */
  double sum_x, sum_y;                 /* f64 sums of them: centroid = sum / size                */
} cs_cluster;
/* The clusters of the members under the links of `distance`: connected components, labelled by their smallest id.
 * members == NULL: everyone.  Only clusters of at least min_size members are reported.  out_ids / out_labels (agent_cap
 * entries): the members of reported clusters, ascending by id, and the label of each; out_clusters (cluster_cap entries):
 * the reported clusters, ascending by label; *n_agents / *n_clusters: the full counts.  Every output may be NULL
 * (out_labels only with out_ids).  0 = Ok. */
int cs_agent_clusters(cs_engine*, double distance, const cs_selection* members, uint64_t min_size,
                      uint64_t* out_ids, uint64_t* out_labels, size_t agent_cap, size_t* n_agents,
                      cs_cluster* out_clusters, size_t cluster_cap, size_t* n_clusters);
/* The same on a mesh.  Collective: every rank passes the same arguments and gets the whole answer, byte for byte the
 * single engine's except sum_x / sum_y, which are under their bound.  On a mesh of more than one tile `distance` is at
 * most halo_cells * cell_size.  No halo exchange is made for it and the step's own exchange state is left as it is: every
 * tile clusters the agents it owns and exports a band record (id, position, local label, tile) of each member within
 * reach of an edge behind which another tile lies; one gather brings these records to every rank, each rank finds on the
 * device the links between its tiles' band agents and the records of the tiles with a higher index and reduces them to
 * distinct (local label, foreign label) pairs, a second gather moves those, every rank runs the same small union-find
 * over labels, applies the label map on the device and merges the per-cluster rows: sizes add, boxes merge, sums add in
 * tile-index order.  A third gather carries the answer.  The number of collectives depends neither on the crowd nor on
 * the answer; what travels before the answer grows with the agents near cuts, not with the crowd.  A tile that fails
 * makes every rank return Err. */
int cs_mesh_agent_clusters(cs_mesh*, double distance, const cs_selection* members, uint64_t min_size,
                           uint64_t* out_ids, uint64_t* out_labels, size_t agent_cap, size_t* n_agents,
                           cs_cluster* out_clusters, size_t cluster_cap, size_t* n_clusters);

#define CS_NO_NEIGHBOUR UINT64_MAX
typedef struct cs_neighbour_stat {   /* 32 bytes */
  uint64_t id;          /* the subject                                                    */
  uint64_t count;       /* others within `distance` of it, itself not among them: exact   */
  uint64_t nearest;     /* the closest of them; CS_NO_NEIGHBOUR when count == 0            */
  double   nearest_d2;  /* its squared distance, bit for bit; +inf when count == 0         */
} cs_neighbour_stat;
/* For each subject, the number of others closer than `distance` and the nearest of them.  Returns the number of subjects
 * with count >= min_count and writes the first min(that, cap) rows, ascending by id; out == NULL or cap == 0: the number
 * only.  subjects / others: NULL: everyone.  SIZE_MAX on error. */
size_t cs_agent_neighbours(cs_engine*, double distance, const cs_selection* subjects, const cs_selection* others,
                           uint64_t min_count, cs_neighbour_stat* out, size_t cap);
/* The same on a mesh.  Collective: every rank passes the same arguments and gets the whole answer, byte for byte the
 * single engine's: counts add exactly and `nearest` is a lexicographic minimum of (d2, id).  On a mesh of more than one
 * tile `distance` is at most halo_cells * cell_size (so +inf is refused there).  No halo exchange is made and the step's
 * own exchange state is left as it is: every tile computes the rows of the subjects it owns against the others it owns
 * and keeps them on its device; it exports a band record (id, position, bit 0 subject / bit 1 other, tile) of each
 * participant within reach of an edge behind which another tile lies; one gather brings these records to every rank;
 * each rank tests, on the device, its tiles' band subjects against the band others of every other tile and merges count
 * and (d2, id) into the subject's row; min_count is applied after that; a last gather carries the reported rows (the
 * count-only form: the counts) and every rank merges the id-sorted runs.  The number of collectives depends neither on
 * the crowd nor on the answer; what travels before the answer grows with the agents near cuts.  A tile that fails makes
 * every rank return SIZE_MAX. */
size_t cs_mesh_agent_neighbours(cs_mesh*, double distance, const cs_selection* subjects, const cs_selection* others,
                                uint64_t min_count, cs_neighbour_stat* out, size_t cap);

typedef struct cs_encounter {   /* 32 bytes */
  uint64_t a, b;        /* the two agents, a < b                                           */
  double   t;           /* the time of their closest approach, in [0, horizon]: bit for bit */
  double   d2;          /* their squared distance then (m2 of the rule): bit for bit        */
} cs_encounter;
/* The pairs of agents now closer than `range` that come closer than `distance` within `horizon`, both keeping their
 * velocity, ascending by (a, b).  Returns the full count and writes min(count, cap) rows (the first ones); out == NULL or
 * cap == 0: the count only (64-bit on the device, no limit).  sel_a / sel_b: the two roles of a pair, NULL: everyone.
 * SIZE_MAX on error. */
size_t cs_encounters(cs_engine*, double distance, double horizon, double range, const cs_selection* sel_a,
                     const cs_selection* sel_b, cs_encounter* out, size_t cap);
/* The same on a mesh.  Collective: every rank passes the same arguments and gets the whole answer, byte for byte the
 * single engine's.  On a mesh of more than one tile `range` is at most halo_cells * cell_size (so +inf is refused there).
 * The scheme is that of cs_mesh_close_pairs, the band record also carrying the widened velocity (40 bytes): no halo
 * exchange is made and the step's own exchange state is left as it is; one gather brings the band records to every rank,
 * each rank tests its tiles' band agents against the records of the tiles with a higher index (every cross-tile pair
 * exactly once), one more gather moves the rows (the count-only form: the counts), and every rank merges the sorted runs.
 * The number of collectives depends neither on the crowd nor on the answer.  A tile that fails makes every rank return
 * SIZE_MAX. */
size_t cs_mesh_encounters(cs_mesh*, double distance, double horizon, double range, const cs_selection* sel_a,
                          const cs_selection* sel_b, cs_encounter* out, size_t cap);

/* Rays against the crowd between steps.  A range scan (what does each lidar beam hit first, and how far away), a line of
 * sight, a free corridor: every agent is a disc of `radius` around the position cs_read_agents reports, and a ray
 * reports the first disc it enters.
 *
 * PARTICIPANTS are the pairs' participants: the agents whose reported position is finite and inside the grid's own
 * rectangle (on a tile or a mesh: the global one; on a tile engine with ghosts only owned agents).  `targets` (NULL:
 * everyone) restricts who can be hit; everybody else is transparent.
 *
 * THE RULE, for ray (o, u, t_max, ignore) and participant q != ignore at (x_q, y_q), with R2 = radius * radius and
 * uu = ux*ux + uy*uy, every operation one f64 operation rounded once (no contraction, no reciprocal, the correctly
 * rounded division and square root):
 *     rx = x_q - ox;  ry = y_q - oy;  d2 = rx*rx + ry*ry
 *     if d2 < R2:                    t = +0.0            (the origin stands inside the disc)
 *     else:
 *       b  = rx*ux + ry*uy;          miss if !(b > 0)
 *       cr = rx*uy - ry*ux
 *       h2 = R2*uu - cr*cr;          miss if !(h2 > 0)   (grazing is a miss)
 *       t  = (b - sqrt(h2)) / uu;    if t < 0: t = +0.0  (rounding only)
 *     HIT iff t < t_max
 * The answer of a ray is the lexicographic minimum of (t, id) over its hits (of two discs entered at the same t the
 * smaller id), or {CS_NO_HIT, +inf}.  It depends neither on slots nor on tiles.  t is in units of the direction AS GIVEN:
 * the point of entry is o + u * t, and a direction of length 2 halves t.  t_max == 0 and radius == 0 hit nothing;
 * t_max = +inf is allowed everywhere, the grid being finite.
 *
 * LINE OF SIGHT from agent A to agent B: o = A's position, u = B - A, t_max = 1, ignore = A; B is visible iff the hit is
 * B (anybody else's disc is entered first otherwise, and a miss means B itself is not a participant or not a target).
 *
 * Refused (SIZE_MAX, nothing written, the engine or mesh still usable; the text names the first bad ray): n >
 * CS_RAYS_MAX, rays == NULL with n > 0, a NaN or negative radius, a ray with a non-finite ox, oy, ux or uy, with uu
 * outside [2^-100, 2^100] (a zero direction included) or with a NaN or negative t_max, a selection cs_select_agents
 * refuses.  Queued steps complete first and an Err of one of them is the call's; no events, the last step report is left
 * alone, nothing is renumbered, and a twin that never asks stays byte-equal. */
#define CS_NO_HIT   UINT64_MAX
#define CS_RAYS_MAX (1u << 20)          /* rays of one call */
typedef struct cs_ray {                 /* 48 bytes */
  double ox, oy;        /* origin, world coordinates, finite                                   */
  double ux, uy;        /* direction AS GIVEN (not normalised): the point at t is o + u * t    */
  double t_max;         /* hits with t < t_max count; >= 0, +inf allowed                       */
  uint64_t ignore;      /* an agent id this ray passes through (the robot that casts it);
                           CS_NO_HIT: nobody; an id that is not alive: nobody                  */
} cs_ray;
typedef struct cs_ray_hit {             /* 16 bytes */
  uint64_t id;          /* the first agent hit; CS_NO_HIT: none                                */
  double   t;           /* its parameter, bit for bit by the rule; +inf when none              */
} cs_ray_hit;
/* Casts n rays; row k of `out` (n rows; may be NULL) is the answer of ray k.  Returns the number of rays that hit
 * something (n == 0: 0), SIZE_MAX on error. */
size_t cs_cast_rays(cs_engine*, const cs_ray* rays, size_t n, double radius, const cs_selection* targets,
                    cs_ray_hit* out /* n rows, row k for ray k; may be NULL */);
/* The same on a mesh.  Collective: every rank passes the same rays and gets the single engine's answer, byte for byte.
 * No halo exchange is made, there are no band records, and t_max and radius have no limit: every tile casts ALL rays
 * against the agents it owns and one gather moves n 16-byte rows per rank; every rank takes the lexicographic minimum of
 * (t, id) per ray.  The number of collectives depends neither on the crowd nor on the answer.  A tile that fails makes
 * every rank return SIZE_MAX.  The step's exchange state is not touched. */
size_t cs_mesh_cast_rays(cs_mesh*, const cs_ray* rays, size_t n, double radius, const cs_selection* targets,
                         cs_ray_hit* out);

/* Paths against the moving crowd between steps.  A route planner holds a TIMED path ("from A to B between 0 s and 2 s,
 * wait until 3.5 s, then to C by 6 s") and asks whether anyone comes within `distance` of it if the crowd keeps walking
 * as it does now, and if so who comes first, when and where.  A LEG is one piece of such a path: a probe point that is at
 * (x0, y0) at time t0 and moves with velocity (vx, vy) until t1, times in seconds from now; v = (0, 0) is a wait (can
 * this door close during the next 2 s).  A path is any number of legs and each leg is answered on its own.
 *
 * An agent is the record cs_read_agents returns for it: x, y in f64 and vx, vy the f32 velocity widened to f64, kept
 * constant.  PARTICIPANTS are the pairs' participants: the agents whose reported position is finite and inside the
 * grid's own rectangle (on a tile or a mesh: the global one; on a tile engine with ghosts only owned agents).  `targets`
 * (NULL: everyone) restricts who can conflict; everybody else is transparent.
 *
 * THE RULE, for leg (x0, y0, vx, vy, t0, t1, ignore) and participant q != ignore, with D2 = distance * distance and
 * T = t1 - t0, every operation one f64 operation rounded once (no contraction, no reciprocal, no f32 pre-reject, the
 * correctly rounded division and square root):
 *     ss = vx_q*vx_q + vy_q*vy_q;       SLOW ENOUGH iff ss < speed_max*speed_max   (else q is not considered; a NaN is not)
 *     px = x_q + vx_q*t0;  py = y_q + vy_q*t0                                     (where q is when the leg begins)
 *     rx = px - x0;  ry = py - y0;  wx = vx_q - vx;  wy = vy_q - vy
 *     d2 = rx*rx + ry*ry
 *     if d2 < D2:              s = +0.0                  (already within the distance when the leg begins)
 *     else:
 *       a  = rx*wx + ry*wy;    miss if !(a < 0)          (not approaching; equal velocities; a NaN)
 *       ww = wx*wx + wy*wy
 *       cr = rx*wy - ry*wx
 *       h2 = D2*ww - cr*cr;    miss if !(h2 > 0)         (grazing is a miss)
 *       s  = (-a - sqrt(h2)) / ww;   if s < 0: s = +0.0  (rounding only)
 *     CONFLICT iff s < T
 * The answer of a leg is the lexicographic minimum of (s, id) over its conflicts (of two agents that arrive at the same
 * s the smaller id), or {CS_NO_HIT, +inf}.  It depends neither on slots nor on tiles.  The time of the conflict is
 * t0 + s and the probe is then at (x0 + vx*s, y0 + vy*s).  T == 0 and distance == 0 give nothing; distance = +inf and
 * speed_max = +inf are allowed everywhere, the grid being finite.
 *
 * speed_max is part of the definition because it is what makes a bounded search sound: an agent slower than speed_max
 * that conflicts during the leg stands NOW within distance + speed_max * t1 of the segment the probe sweeps, and the
 * device looks no further.  A host that wants nobody left out passes a bound at or above its planners' top speed;
 * cs_count_agents with CS_SEL_SPEED tells it how many agents exceed a bound.
 *
 * Refused (SIZE_MAX, nothing written, the engine or mesh still usable; the text names the first bad leg): n >
 * CS_LEGS_MAX, legs == NULL with n > 0, a NaN or negative distance or speed_max, a leg with a non-finite x0, y0, vx, vy,
 * t0 or t1, with t0 < 0 or with t1 < t0, a selection cs_select_agents refuses.  Queued steps complete first and an Err of
 * one of them is the call's; no events, the last step report is left alone, nothing is renumbered, and a twin that never
 * asks stays byte-equal. */
#define CS_LEGS_MAX (1u << 20)          /* legs of one call */
typedef struct cs_leg {                 /* 56 bytes */
  double x0, y0;        /* where the probe is at t0, world coordinates, finite                 */
  double vx, vy;        /* its velocity during the leg; finite; (0, 0) is a wait               */
  double t0, t1;        /* 0 <= t0 <= t1, both finite, seconds from now                        */
  uint64_t ignore;      /* an agent id the leg passes through (the robot itself);
                           CS_NO_HIT: nobody; an id that is not alive: nobody                  */
} cs_leg;
typedef struct cs_leg_hit {             /* 16 bytes */
  uint64_t id;          /* the first agent to come within `distance`; CS_NO_HIT: none          */
  double   s;           /* seconds after t0 at which it does, bit for bit by the rule; +inf when none */
} cs_leg_hit;
/* Checks n legs; row k of `out` (n rows; may be NULL) is the answer of leg k.  Returns the number of legs with a
 * conflict (n == 0: 0), SIZE_MAX on error. */
size_t cs_leg_conflicts(cs_engine*, const cs_leg* legs, size_t n, double distance, double speed_max,
                        const cs_selection* targets, cs_leg_hit* out /* n rows, row k for leg k; may be NULL */);
/* The same on a mesh.  Collective: every rank passes the same legs and gets the single engine's answer, byte for byte.
 * No halo exchange is made, there are no band records, and distance, speed_max and t1 have no limit: every tile runs ALL
 * legs against the agents it owns and one gather moves n 16-byte rows per rank; every rank takes the lexicographic
 * minimum of (s, id) per leg.  The number of collectives depends neither on the crowd nor on the answer.  A tile that
 * fails makes every rank return SIZE_MAX.  The step's exchange state is not touched. */
size_t cs_mesh_leg_conflicts(cs_mesh*, const cs_leg* legs, size_t n, double distance, double speed_max,
                             const cs_selection* targets, cs_leg_hit* out);

/* Every agent that enters a leg, with the time it enters and the time it leaves.  cs_leg_conflicts says who comes within
 * `distance` of a leg FIRST; a planner that has to wait (a safe-interval planner asking when a vertex or a lane of its
 * graph is occupied during a horizon, a door interlock asking when the threshold is free for 2 s in a row) needs every
 * interval during which somebody is within the distance.  cs_leg_intervals lists them: one row per (leg, agent) that
 * conflicts.  Two points that move uniformly are apart by a convex quadratic of time, so a pair has at most one interval.
 *
 * THE RULE.  The legs, the participants, `targets`, `ignore`, the speed test and s_in are those of cs_leg_conflicts, word
 * for word: (leg k, agent q) is a row exactly when q is a conflict of leg k there, and s_in is that rule's s, the same
 * bits.  s_out is new; every operation is again one f64 operation rounded once, and a, ww, cr and h2 are computed also for
 * a candidate that is inside at the start:
 *     (ss, px, py, rx, ry, wx, wy, d2 as there)
 *     a = rx*wx + ry*wy;  ww = wx*wx + wy*wy;  cr = rx*wy - ry*wx;  h2 = D2*ww - cr*cr
 *     s_in:   +0.0 if d2 < D2;  else miss if !(a < 0), miss if !(h2 > 0), s_in = (-a - sqrt(h2)) / ww, +0.0 if s_in < 0
 *     ROW iff s_in < T
 *     s_out:  if !(h2 > 0):   T if ww == 0 (the same velocity, inside: it never leaves), else s_in (rounding only)
 *             else:           e = (-a + sqrt(h2)) / ww;  if !(e > s_in) e = s_in;  if !(e < T) e = T;  s_out = e
 * so 0 <= s_in <= s_out <= T; the agent is within the distance from t0 + s_in to t0 + s_out, and s_out == T says that it
 * is still there when the leg ends.  distance = +inf gives [0, T] for every slow participant (inf * ww is inf for ww > 0
 * and inf * 0 is a NaN, which takes the ww == 0 branch); T == 0 and distance == 0 give no rows.
 *
 * THE ANSWER.  Every row once, ascending by (leg, id).  The call returns the full count and writes the first
 * min(count, cap) rows, nothing beyond them; out_counts[k], if given, is the full number of rows of leg k whatever cap is.
 * out == NULL or cap == 0 asks for the counts only: one pass that makes no row, with a 64-bit total on the device, and no
 * limit.  With cap > 0 a count above CS_PAIRS_MAX is refused (SIZE_MAX, "too many intervals to list", the engine usable).
 * Every other refusal is that of cs_leg_conflicts (the text says leg_intervals and names the first bad leg); after a
 * refusal nothing is written, out_counts included.  n == 0 returns 0.  Queued steps complete first and an Err of one of
 * them is the call's; no events, the last step report is left alone, nothing is renumbered, and a twin that never asks
 * stays byte-equal. */
typedef struct cs_leg_interval {        /* 32 bytes */
  uint64_t leg;         /* index of the leg in the call                                        */
  uint64_t id;          /* the agent (the external id under CS_CFG_WIDE_IDS)                   */
  double   s_in;        /* seconds after t0 at which it comes within `distance`, bit for bit   */
  double   s_out;       /* seconds after t0 at which it leaves again, at most T, bit for bit   */
} cs_leg_interval;
size_t cs_leg_intervals(cs_engine*, const cs_leg* legs, size_t n, double distance, double speed_max,
                        const cs_selection* targets, uint64_t* out_counts /* n entries; may be NULL */,
                        cs_leg_interval* out, size_t cap);
/* The same on a mesh.  Collective: every rank passes the same legs and gets the single engine's answer, byte for byte.
 * No halo exchange is made, there are no band records, and distance, speed_max and t1 have no limit: every tile runs ALL
 * legs against the agents it owns.  One gather carries the per-leg counts (agents are disjoint across tiles, so counts
 * add, and every rank decides the CS_PAIRS_MAX refusal from them alike); when listing, one more carries each rank's first
 * rows, and every rank merges the (leg, id)-sorted runs.  The number of collectives depends neither on the crowd nor on
 * the answer.  A tile that fails makes every rank return SIZE_MAX.  The step's exchange state is not touched. */
size_t cs_mesh_leg_intervals(cs_mesh*, const cs_leg* legs, size_t n, double distance, double speed_max,
                             const cs_selection* targets, uint64_t* out_counts, cs_leg_interval* out, size_t cap);

/* Agents in polygon zones.  The regions a selection can name are an axis-aligned rectangle and a circle; the zones of a
 * building (rooms and corridors drawn in a traffic editor, a lift cabin that stands at an angle, an L-shaped lobby, the
 * keep-out region in front of a door, the catchment of a sink) are polygons.  cs_zone_agents counts, and lists, the agents
 * inside each of up to CS_ZONES_MAX polygons in one call.  A zone is a run of `count` vertices of the call's vertex
 * array (a vertex is two doubles, x then y); the ring closes from its last vertex to its first.  Zones may overlap, and
 * they may share vertices: their runs may overlap.
 *
 * WHO TAKES PART.  An agent is the record cs_read_agents returns for it at that moment, (x, y) its reported f64 position.
 * It takes part by the rule of cs_close_pairs: a finite position inside the grid's own rectangle (the global grid's on a
 * tile engine and on a mesh); on a tile whose arrays hold ghosts only owned agents; `filter` is judged as for
 * cs_select_agents, NULL is everyone.  Agents the index never took take no part, nor do clamped, aliased or NaN agents.
 *
 * THE RULE.  The box of a zone is the exact minimum and maximum of its vertices' coordinates, bx0, bx1, by0, by1.  Every
 * operation of the ring test is one f64 operation rounded once: no contraction, no reciprocal, no f32 pre-reject.  For
 * every edge of the ring, vertex i to vertex (i + 1) % count, let (lx, ly) be the end with the smaller y and (hx, hy) the
 * other (so two zones that share an edge, given by the same two vertices, evaluate it to the same bits whichever way each
 * runs along it).  An edge with ly == hy never straddles; otherwise
 *     the edge STRADDLES iff ly <= y && y < hy
 *     a straddling edge CROSSES iff c > 0,  ex = hx - lx;  ey = hy - ly;  px = x - lx;  py = y - ly;  c = ex*py - ey*px
 *     the agent is IN THE ZONE iff bx0 <= x && x <= bx1 && by0 <= y && y <= by1 and the number of crossing edges is odd
 * This is the even-odd rule, so concave and self-intersecting rings are defined.  The box is part of the rule.  It is what
 * lets the library visit only the cells the box touches and still be exact: for x > bx1, or y outside [by0, by1], no edge
 * crosses anyway (no edge straddles a y outside the box; for x beyond both ends of a straddling edge px >= |ex| and
 * py <= ey as rounded, products round monotonically, so c <= 0), but for x < bx0 the rounding of c could say otherwise,
 * and the box settles it.  What follows: the ring (x0,y0) (x1,y0) (x1,y1) (x0,y1) holds, in either winding, exactly the
 * participants CS_SEL_RECT selects with the same numbers, x0 <= x < x1 && y0 <= y < y1; of zones that tile a region with
 * matching vertices every agent in the region is in an odd number, because shared edges are judged alike, and in exactly
 * one where all the arithmetic is exact (small dyadic coordinates).
 *
 * THE ANSWER.  Every row (zone, id) once, ascending by (zone, id).  The call returns the full count and writes the first
 * min(count, cap) rows, nothing beyond them; out_counts[k], if given, is the full number of rows of zone k whatever cap
 * is.  out == NULL or cap == 0 asks for the counts only: one pass that makes no row, with a 64-bit total on the device,
 * and no limit.  With cap > 0 a count above CS_PAIRS_MAX is refused (SIZE_MAX, "too many zone agents to list", the engine
 * usable).  n == 0 returns 0.
 *
 * REFUSALS (SIZE_MAX; nothing is written, out_counts included; the engine or mesh stays usable; the text names the first
 * bad zone): null zones or vertices with n > 0, n > CS_ZONES_MAX, n_vertices > CS_ZONE_VERTICES_MAX, a filter that
 * cs_select_agents refuses, a zone with count < 3, with first + count > n_vertices, with flags != 0, or with a NaN or
 * infinite vertex.
 *
 * Queued steps complete first and an Err of one of them is the call's; no events, the last step report is left alone,
 * nothing is renumbered (the arrays may be sorted by cell, as by the other spatial queries), and a twin that never asks
 * stays byte-equal. */
#define CS_ZONES_MAX         65536u     /* zones in one call                    */
#define CS_ZONE_VERTICES_MAX (1u << 20) /* vertices of all zones of one call    */
typedef struct cs_zone {       /* 16 bytes: one polygon, a run of the call's vertex array          */
  uint64_t first;              /* index of its first vertex (a vertex is two doubles, x then y)    */
  uint32_t count;              /* its vertices, >= 3; the ring closes from the last to the first   */
  uint32_t flags;              /* 0                                                                */
} cs_zone;
typedef struct cs_zone_agent { /* 16 bytes: agent `id` is in zone `zone`                           */
  uint64_t zone;               /* index of the zone in the call                                    */
  uint64_t id;                 /* the agent (the external id under CS_CFG_WIDE_IDS)                */
} cs_zone_agent;
size_t cs_zone_agents(cs_engine*, const cs_zone* zones, size_t n, const double* vertices_xy, size_t n_vertices,
                      const cs_selection* filter, uint64_t* out_counts /* n entries; may be NULL */,
                      cs_zone_agent* out, size_t cap);
/* The same on a mesh.  Collective: every rank passes the same zones and gets the single engine's answer, byte for byte.
 * Every tile runs ALL zones against the agents it owns; one gather carries the per-zone counts (agents are disjoint
 * across tiles, so counts add, and every rank decides the CS_PAIRS_MAX refusal from them alike); when listing, one more
 * carries each rank's first rows, and every rank merges the (zone, id)-sorted runs.  No halo exchange is made and the
 * step's exchange state is not touched.  A tile that fails makes every rank return SIZE_MAX. */
size_t cs_mesh_zone_agents(cs_mesh*, const cs_zone* zones, size_t n, const double* vertices_xy, size_t n_vertices,
                           const cs_selection* filter, uint64_t* out_counts, cs_zone_agent* out, size_t cap);

/* Who crosses a line.  A door threshold, a turnstile, a crosswalk, a platform edge and a light barrier are all a segment,
 * and the question is who walks through it and in which direction: an automatic door asks whether anyone will pass its
 * threshold within the next 1.5 s and from which side, a traffic planner how many people are about to cross a lane, a
 * flow meter for the flow through a bottleneck per direction.  A GATE is the segment from A = (ax, ay) to B = (bx, by)
 * with a time window t0 <= t1, in seconds from now; cs_gate_crossings counts, and lists, for up to CS_GATES_MAX gates
 * in one call the agents that cross each within its window if everybody keeps walking as they do now.
 *
 * An agent is the record cs_read_agents returns for it: x, y in f64 and vx, vy the f32 velocity widened to f64, kept
 * constant.  Agents are points, as for zones.  PARTICIPANTS are the pairs' participants: the agents whose reported
 * position is finite and inside the grid's own rectangle (on a tile or a mesh: the global one; on a tile engine with
 * ghosts only owned agents).  `filter` is judged as for cs_select_agents; NULL is everyone.
 *
 * THE RULE, for gate (ax, ay, bx, by, t0, t1) and participant q, with S2 = speed_max * speed_max and T = t1 - t0, every
 * operation one f64 operation rounded once (no contraction, no reciprocal, no f32 pre-reject, the correctly rounded
 * division):
 *     ss = vx*vx + vy*vy;            SLOW ENOUGH iff ss < S2   (else q is not considered; a NaN is not)
 *     px = x + vx*t0;  py = y + vy*t0                          (where q is when the window opens)
 *     ex = bx - ax;    ey = by - ay
 *     rx = px - ax;    ry = py - ay
 *     c0 = ex*ry - ey*rx             (the side at t0: > 0 is left of A->B)
 *     cv = ex*vy - ey*vx             (the rate of change of the side)
 *     cu = rx*vy - ry*vx
 *     miss unless (cv > 0 && c0 <= 0) || (cv < 0 && c0 >= 0)   (parallel, A == B, moving away, a NaN: miss)
 *     s  = (-c0) / cv;  if !(s > 0): s = +0.0                  (on the line at t0 and moving off it: s = +0.0)
 *     u  = cu / cv
 *     CROSSING iff s < T && u >= 0 && u < 1
 *     dir = +1 if cv > 0 (the agent ends on the left of A->B), -1 otherwise
 * The crossing happens at time t0 + s at the point A + u * (B - A).  The interval of u is half-open, so gates that chain
 * through shared vertices (a polyline) count a walker once wherever every operation is exact (small dyadic
 * coordinates).  A straight walker crosses a line at most once, so (gate, id) is a unique key.  T == 0 gives nothing; a
 * gate with A == B is accepted and crosses nobody; speed_max = +inf and any finite t1 are allowed, the grid being finite.
 *
 * speed_max is part of the definition for the reason it is for legs: a slow-enough agent that crosses within the window
 * stands NOW within speed_max * t1 of the segment, and the device looks no further than that reach plus one spare cell.
 * The rule's roundings place the crossing off by about 2^-51 |r| / sin(angle between the gate and the velocity), far
 * below that cell; only a walker that is parallel to an oblique gate and collinear with it to within the rounding of cv
 * and c0 themselves (no such case exists where the products are exact: axis-aligned gates, dyadic coordinates) can be a
 * crossing by rounding alone, and it is listed when it stands within the reach and not when it stands beyond it.  A host
 * that wants nobody left out passes a bound at or above its planners' top speed.
 *
 * THE ANSWER.  Every row once, ascending by (gate, id); ids are external ids under CS_CFG_WIDE_IDS.  The call returns the
 * full count and writes the first min(count, cap) rows, nothing beyond them; out_counts[2k] and out_counts[2k + 1], if
 * given, are the full numbers of rows of gate k with dir +1 and with dir -1, whatever cap is.  out == NULL or cap == 0
 * asks for the counts only: one pass that makes no row, with a 64-bit total on the device, and no limit.  With cap > 0 a
 * count above CS_PAIRS_MAX is refused (SIZE_MAX, "too many crossings to list", the engine usable).  n == 0 returns 0.
 *
 * REFUSALS (SIZE_MAX; nothing is written, out_counts included; the engine or mesh stays usable; the text names the first
 * bad gate): n > CS_GATES_MAX, gates == NULL with n > 0, a NaN or negative speed_max, a gate with a non-finite field,
 * with t0 < 0 or with t1 < t0, a selection cs_select_agents refuses.
 *
 * Queued steps complete first and an Err of one of them is the call's; no events, the last step report is left alone,
 * nothing is renumbered, and a twin that never asks stays byte-equal. */
#define CS_GATES_MAX (1u << 20)         /* gates of one call */
typedef struct cs_gate {                /* 48 bytes */
  double ax, ay;        /* the end A, world coordinates, finite                                */
  double bx, by;        /* the end B; left and right are those of somebody looking from A to B */
  double t0, t1;        /* 0 <= t0 <= t1, both finite, seconds from now                        */
} cs_gate;
typedef struct cs_gate_crossing {       /* 32 bytes */
  uint32_t gate;        /* index of the gate in the call                                       */
  int32_t  dir;         /* +1: the agent ends on the left of A->B, -1: on the right            */
  uint64_t id;          /* the agent (the external id under CS_CFG_WIDE_IDS)                   */
  double   s;           /* seconds after t0 at which it crosses, bit for bit; never -0.0       */
  double   u;           /* where: the point A + u * (B - A), 0 <= u < 1, bit for bit           */
} cs_gate_crossing;
size_t cs_gate_crossings(cs_engine*, const cs_gate* gates, size_t n, double speed_max, const cs_selection* filter,
                         uint64_t* out_counts /* 2n entries: [2k] dir +1, [2k+1] dir -1; may be NULL */,
                         cs_gate_crossing* out, size_t cap);
/* The same on a mesh.  Collective: every rank passes the same gates and gets the single engine's answer, byte for byte.
 * Every tile runs ALL gates against the agents it owns; one gather carries the 2n counts (agents are disjoint across
 * tiles, so counts add, and every rank decides the CS_PAIRS_MAX refusal from them alike); when listing, one more carries
 * each rank's first rows, and every rank merges the (gate, id)-sorted runs.  No halo exchange is made and the step's
 * exchange state is not touched.  A tile that fails makes every rank return SIZE_MAX. */
size_t cs_mesh_gate_crossings(cs_mesh*, const cs_gate* gates, size_t n, double speed_max, const cs_selection* filter,
                              uint64_t* out_counts, cs_gate_crossing* out, size_t cap);

/* Flow-field high-level planner ("Flow-field planner"): a raster of preferred velocities that lives on
 * the device and is sampled there every step, for the planners that are a lookup by position: a distance transform to the
 * exits, a potential that avoids the density cs_agent_field reports, a lane direction map.  The step stays queued: no
 * download, no host call, no wait.
 *   - Handles come from the counter of cs_register_hlp and work wherever a planner handle works (cs_add_agents,
 *     cs_source_sink_desc.hlp, CS_SEL_HLP).  A field planner takes no targets (cs_set_targets: CS_TARGET_IGNORED), hears of
 *     no removal and gets no set_target event; a source-sink that names it runs its waypoint and sink tests as ever.
 *   - The raster is the cs_field_desc of cs_agent_field, bin (ix, iy) at iy * nx + ix, nx * ny <= CS_FIELD_MAX_CELLS; vxy
 *     holds nx * ny pairs (vx, vy) of f32 in HOST memory and is copied before the call returns.  +-inf samples are
 *     allowed, NaN samples have a meaning (below).
 *   - The rule.  The agent is the record cs_read_agents would report at the start of the step; x, y its f64 position.
 *     Every operation is ONE f64 operation rounded once: no contraction, no reciprocal.
 *       fx = (x - x0) / cell_w, fy = (y - y0) / cell_h (the expression of cs_agent_field); inside iff
 *       0 <= fx && fx < nx && 0 <= fy && fy < ny; then ix = (uint32_t)fx, iy = (uint32_t)fy.
 *       NONE is the preferred velocity (0, 0) (lib.rs:263).  An agent outside the raster, or with a NaN or infinite fx
 *       or fy, gets NONE.
 *       CS_HLP_FIELD_NEAREST: s = vxy[iy * nx + ix]; NONE if s.vx or s.vy is NaN, else s exactly.
 *       CS_HLP_FIELD_BILINEAR (samples sit at bin centres, the edges clamp): ax = fx - 0.5; if ax < 0 then i0 = i1 = 0
 *       and tx = 0, else i0 = (uint32_t)ax, tx = ax - (double)i0, i1 = min(i0 + 1, nx - 1); the same along y for j0,
 *       j1, ty.  The four samples c00 = (i0, j0), c10 = (i1, j0), c01 = (i0, j1), c11 = (i1, j1) are widened to f64.  If
 *       any of their eight components is NaN the answer is the NEAREST answer of the agent's own bin (a NaN bin marks a
 *       wall, and the agents next to it still move).  Otherwise, per component, a = c00 + (c10 - c00) * tx,
 *       b = c01 + (c11 - c01) * tx, r = a + (b - a) * ty, and the answer is ((float)r_x, (float)r_y).
 *     What the step integrates is what a CS_HLP_CALLBACK planner returning the same f64 pair would leave: (float)out.  So
 *     an engine with a field planner and one whose host planner evaluates this rule step to the same bytes.  (A NaN
 *     ANSWER, which only infinite samples can give, inf - inf or inf * 0, has no specified sign or payload.)
 *   - cs_hlp_field_update: new values for the same raster and sampling.  Steps already queued use the old values, the
 *     next step the new ones; the caller's buffer is copied before the call returns and nothing waits for the device.
 *   - Refused, nothing registered or changed, the engine usable (registration: UINT32_MAX and cs_last_error says why;
 *     update: 3): a null pointer, a raster cs_agent_field would refuse, an unknown sampling, an update of a handle that
 *     is not a field planner.
 *   - Every tile of a mesh holds the whole field (it is indexed in world coordinates); re-cuts keep it.  On a
 *     distributed mesh both mesh calls are collective with equal arguments.  cs_device_bytes counts the fields. */
#define CS_HLP_FIELD 5u                 /* kind of a planner made by cs_register_hlp_field */
#define CS_HLP_FIELD_NEAREST  0u        /* the sample of the agent's own bin                */
#define CS_HLP_FIELD_BILINEAR 1u        /* between the four nearest bin centres             */
#define CS_STAT_HLP_FIELD_LAUNCHES 8u   /* cs_kernel_stat: launches of the field kernel so far */
#define CS_STAT_HLP_FIELD_NS 9u         /* ... and their device time in ns, by events, in an engine created while
                                         * CS_HLP_FIELD_TIME=1 was set (measurement; 0 otherwise); reading it waits */
/* Planner handle, or UINT32_MAX (cs_last_error says why). */
uint32_t cs_register_hlp_field(cs_engine*, const cs_field_desc* raster, uint32_t sampling, const float* vxy);
int cs_hlp_field_update(cs_engine*, uint32_t hlp, const float* vxy);
uint32_t cs_mesh_register_hlp_field(cs_mesh*, const cs_field_desc*, uint32_t sampling, const float* vxy);
int cs_mesh_hlp_field_update(cs_mesh*, uint32_t hlp, const float* vxy);

/* Solving a flow field on the device ("Solving a flow field"): from goal bins, walls, a slowness
 * raster and the crowd's density to the raster of preferred velocities a field planner samples, without a host solve and
 * without the raster crossing the bus.  The distances are shortest-path distances by a rule of single IEEE operations,
 * so they are the same f64 bits whatever order the relaxations run in: a host Dijkstra, sweeps, tiles on the device.
 *   - Inputs.  raster: a cs_field_desc (the checks of cs_agent_field), bin (ix, iy) at iy * nx + ix.  goals: uint8_t
 *     [nx * ny], required, non-zero = a goal.  blocked: uint8_t[nx * ny] or NULL (no walls), non-zero = a wall.
 *     slowness: float[nx * ny] or NULL (1 everywhere), every value finite and >= 0.  speed: finite, >= 0.
 *     density_weight: finite, 0 <= w <= 2^32 (so that w * count is finite for any u32 count).  density_filter: a
 *     cs_selection or NULL (every agent).  All arrays are HOST memory and are read before the call returns.
 *   - Every operation is ONE f64 operation rounded once: no contraction, no reciprocal, no hypot.
 *   - Lengths, computed once on the host: len(+-1, 0) = cell_w, len(0, +-1) = cell_h, and for the four diagonals
 *     len = sqrt(cell_w * cell_w + cell_h * cell_h).
 *   - Slowness.  s(bin) = (double)slowness[bin] * (1.0 + density_weight * (double)count[bin]), where count is exactly
 *     what cs_agent_field(raster, density_filter) would report now, the agents the index never took included.  With
 *     density_weight == 0 no raster of the crowd is made and the factor is left out: s = (double)slowness[bin], or
 *     exactly 1.0 without a slowness.
 *   - Moves.  The eight steps (dx, dy) are ordered dy = -1, 0, 1 outer and dx = -1, 0, 1 inner, (0, 0) skipped.  A step
 *     from (ix, iy) to (ix + dx, iy + dy) is allowed when the target is inside the raster, the target is not blocked,
 *     and, for a diagonal, neither (ix + dx, iy) nor (ix, iy + dy) is blocked (nobody cuts a wall's corner).  It costs
 *     len(dx, dy) * s(ix, iy): the slowness of the bin the walker leaves.
 *   - Distance.  dist = 0 at every bin that is a goal and not blocked, +inf at blocked bins; elsewhere dist(j) = min
 *     over the allowed steps from j to i of dist(i) + cost.  This is the least fixed point; IEEE addition is monotone
 *     (a <= b implies a + c <= b + c), so it is unique down to the bits.  Unreachable bins keep +inf.
 *   - Vector.  A goal bin (not blocked) gets (0, 0).  A blocked or unreachable bin gets (NaN, NaN) (the quiet NaN
 *     0x7FC00000: a wall to the samplers of cs_register_hlp_field).  Any other bin takes the FIRST step, in the order
 *     above, whose dist(target) + cost is smallest and finite, and gets ((float)((speed * sx) / n), (float)((speed * sy)
 *     / n)) with sx = dx * cell_w, sy = dy * cell_h, n = len(dx, dy): eight possible vectors, a table the host makes.
 *     Where slowness is 0, or where a cost is absorbed by a huge distance (d + c == d), two bins can point at one
 *     another: the rule promises the distances there, not progress.
 *   - hlp: a field planner of this engine whose raster equals desc->raster byte for byte, or UINT32_MAX.  With a planner
 *     the last kernel writes the vectors straight into the planner's device samples on the engine's stream: behind the
 *     steps already queued, in front of the next one (the ordering of cs_hlp_field_update; an update still in flight is
 *     ordered by the same stream).  Without out_vxy and out_dist no raster crosses the bus in either direction but the
 *     masks (and the slowness) going up.
 *   - The call WAITS for the device: the solve runs in rounds (separate launches, at most nx * ny + 1, a derived bound:
 *     beyond it the call returns 90) and the host reads one word per round.  What it saves is the host solve and the
 *     raster's round trips.  stats->reached: the bins with a finite distance; stats->rounds: the rounds launched up to and
 *     including the first that changed nothing (a measurement: it can differ between two runs, the results cannot).
 *   - Refused (3), nothing changed anywhere, the planner's samples untouched, the engine usable: a null desc or null
 *     goals, a raster cs_agent_field would refuse, an hlp that is not a field planner or is one of another raster, a
 *     slowness that is NaN, infinite or negative, a speed or density_weight outside the ranges above, a selection
 *     cs_agent_field would refuse, nothing to write to (hlp == UINT32_MAX and both outputs NULL).
 *   - On a mesh the call is collective with equal arguments.  The counts come by the path of cs_mesh_agent_field (the
 *     same bytes on every rank); then every tile solves the same problem and writes its own copy of the planner's
 *     samples.  Outputs are taken from the first local tile.  cs_device_bytes counts the solve's scratch. */
typedef struct cs_flow_desc {
  cs_field_desc raster;
  const uint8_t* goals; const uint8_t* blocked; const float* slowness;
  double speed, density_weight;
  const cs_selection* density_filter;
} cs_flow_desc;
typedef struct cs_flow_stats { uint64_t reached; uint32_t rounds; uint32_t reserved; } cs_flow_stats;
/* out_vxy (nx * ny float pairs), out_dist (nx * ny doubles), stats: each may be NULL.  0 = Ok. */
int cs_flow_field_solve(cs_engine*, const cs_flow_desc*, uint32_t hlp, float* out_vxy, double* out_dist, cs_flow_stats*);
int cs_mesh_flow_field_solve(cs_mesh*, const cs_flow_desc*, uint32_t hlp, float* out_vxy, double* out_dist, cs_flow_stats*);

#ifdef __cplusplus
}
#endif
#endif /* CROWDSTEP_STATE_H */
