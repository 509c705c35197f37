// cs_kernels_step.hip.inc — K4: the neighbour kernels (LDS-tiled and gather), their shared epilogue, the workgroup builders
// Part of the single translation unit crowdstep_hip.hip (included there, in order).

// ---------------------------------------------------------------------------
// Shared epilogue of the step kernels: integrate, re-bin, waypoint/sink test,
// histogram for the next scatter, source-occupancy marks.
// (lib.rs:295-346; commit lib.rs:350-359 is the write into the `out` arrays)
// ---------------------------------------------------------------------------
// set_target(&self.agents[&agent_id], waypoints[next], (r, r)): the agent as it was BEFORE the step
struct WpEvent {
  uint32_t id, group, next_wp, cell;
  float ox, oy;
  uint32_t slot, pad;  // slot of the agent in the step's output arrays
};

struct EpilogueCore {
  AgentArrays out;
  uint32_t* cell_count;
  Counters* ctr;
  const GroupDev* groups;
  const SinkDev* sinks;
  const double* waypoints;  // global f64 pairs
  double grid_off_x, grid_off_y, cell_size;
  uint2* destroyed;  // append list of (id, meta)
  uint32_t destroyed_cap;
  WpEvent* wp_events;  // waypoint advances of agents with a host planner (set_target, lib.rs:325-333)
  uint32_t wp_events_cap;
  // source occupancy for the next step's spawn phase
  const uint32_t* src_cell_start;  // per cell, into src_sorted
  const uint32_t* src_sorted;      // sink slots sorted by source cell
  uint32_t* src_occupied;
  // CS_HLP_ROUTE: per route (first waypoint, count) into route_xy (global f64 pairs); the route
  // book (start hash, goal hash) -> route and the SpatialHash resolution of every planner
  const uint2* route_desc;
  const double* route_xy;
  const RouteBookEntry* route_book;
  uint32_t route_book_mask;
  const double* hlp_route_scale;
  // velocities a host LocalPlanner returned for this step, by slot of the sorted arrays (lp_kind == 2: the slow path,
  // cs_register_lp_callback); null while no such planner exists
  const float2* lp_vel;
};

struct BlockDesc;
// ... plus what only ever lives in device memory (see k_step_tiled's CTX_BY_VALUE)
struct EpilogueCtx : EpilogueCore {
  // tile engines, one-phase halo exchange: the step kernels append the agents they have moved into
  // (or within) the band along a shared edge to the neighbours' send buffers themselves, so the
  // next exchange needs no pack launch.  halo_band = 0: no packing here.
  HaloBuffers8 halo_send;
  uint32_t halo_band;
  unsigned long long* peek;  // pinned host memory: (StepParams::peek_seq << 32 | n_alive), or null
  // Small crowds (cs_engine, "the window builder off the critical path"): the workgroups [build_first, build_first +
  // build_bands) of the neighbour kernel's launch do not step a window, they cut the NEXT step's band windows, from
  // this step's cell_start, into the other descriptor array.  build_bands = 0: no builder workgroups.
  // (both descriptor arrays and their counters, in address order: the two swap every step, and a context that named
  // "the other one" would differ from step to step and be stored again by a launch of its own, ~5 us on the critical
  // path; which of the two this launch's builders fill travels by value: TileCfg::build_sel)
  BlockDesc* build_desc[2];
  uint32_t* build_n_blocks[2];
  uint32_t* build_prefix;
  uint32_t build_first, build_bands, build_rows, build_target, build_stage_cap, build_max_cols, build_desc_cap, build_g_h;
  GridDev build_g;  // (the builder reads the grid from here: handing it the kernel's own copy would put that copy on the stack)
};

__device__ __forceinline__ void step_epilogue(const StepParams& P, const EpilogueCore& E,
                                              const EpilogueCtx* __restrict__ Ep, uint32_t i,
                                              uint32_t gx, uint32_t gy, float2 off, uint32_t id,
                                              uint32_t meta, const GroupDev& grp, float wx, float wy,
                                              uint32_t route_st, uint32_t late_check) {
  // waypoint / sink test on the OLD position (lib.rs:304-336)
  uint32_t next_wp = meta_waypoint(P.g, meta);
  bool destroyed = false;
  if (grp.sink >= 0) {
    const SinkDev& s = E.sinks[grp.sink];
    if (next_wp >= s.wp_count) {
      destroyed = true;  // "rogue agent", lib.rs:310-313
    } else {
      double wxg = E.waypoints[2 * (s.wp_begin + next_wp)];
      double wyg = E.waypoints[2 * (s.wp_begin + next_wp) + 1];
      // waypoint relative to this agent's cell origin, rounded once to f32
      float rx = (float)(wxg - (E.grid_off_x + (double)(P.g.org_x + gx) * E.cell_size));
      float ry = (float)(wyg - (E.grid_off_y + (double)(P.g.org_y + gy) * E.cell_size));
      float ddx = off.x - rx, ddy = off.y - ry;
      if (sqrtf(ddx * ddx + ddy * ddy) < s.radius_sink) {
        atomicAdd(&E.ctr->n_waypoint_hits, 1u);
        if (next_wp == s.wp_count - 1) {
          if (s.loop_forever)
            next_wp = 0;
          else
            destroyed = true;
        } else {
          next_wp += 1;
          bool to_host = grp.hlp_kind == CS_HLP_CALLBACK;
          if (grp.hlp_kind == CS_HLP_ROUTE) {
            // RMFPlanner::set_target(old agent, next waypoint), rmf/mod.rs:217-236: a (start, goal)
            // pair that is in the route book is answered here (agent_cache.insert(id, (route, 0)));
            // only a miss goes to the host, which plans the route and adds it to the book
            const double res = E.hlp_route_scale[grp.hlp];
            const double px = E.grid_off_x + ((double)(P.g.org_x + gx) * E.cell_size + (double)off.x);
            const double py = E.grid_off_y + ((double)(P.g.org_y + gy) * E.cell_size + (double)off.y);
            const double tx = E.waypoints[2 * (s.wp_begin + next_wp)], ty = E.waypoints[2 * (s.wp_begin + next_wp) + 1];
            const uint32_t r1 = route_book_find(E.route_book, E.route_book_mask, grp.hlp, route_spatial_hash(px, res),
                                                route_spatial_hash(py, res), route_spatial_hash(tx, res),
                                                route_spatial_hash(ty, res));
            if (r1) route_st = r1;  // (route, waypoint 0)
            else to_host = true;
          }
          if (to_host) {
            uint32_t k = atomicAdd(&E.ctr->n_wp_events, 1u);
            if (k < E.wp_events_cap)
              E.wp_events[k] = WpEvent{id, meta_group(P.g, meta), next_wp, gx * P.g.nx + gy, off.x, off.y, i, 0u};
          }
        }
      }
    }
  }

  // integrate (lib.rs:295-297): new_pos = pos + vel * dt, cell-relative
  float nox = off.x + wx * P.dt, noy = off.y + wy * P.dt;
  if (!(fabsf(nox) < f_inf() && fabsf(noy) < f_inf() && fabsf(wx) < f_inf() && fabsf(wy) < f_inf()))
    atomicAdd(&E.ctr->n_nonfinite, 1u);
  uint32_t ncell = rebin(P.g, gx, gy, nox, noy, E.ctr);

  if (destroyed) {
    uint32_t k = atomicAdd(&E.ctr->n_destroyed, 1u);
    if (k < E.destroyed_cap) E.destroyed[k] = make_uint2(id, meta);
    ncell = CS_INVALID_CELL;
  }
  const bool keep = ncell != CS_INVALID_CELL;
  if (keep) {
    E.out.off[i] = make_float2(nox, noy);
    E.out.vel[i] = make_float2(wx, wy);
    E.out.id[i] = id;
    E.out.meta[i] = meta_make(P.g, meta_group(P.g, meta), next_wp);
    if (E.out.route) E.out.route[i] = route_st;
  }
  E.out.cell[i] = ncell;
  // histogram for the next scatter: agents are in cell order and few change cell per step,
  // so the lanes of a wave hit a handful of counters; one atomic per distinct cell per wave
  const uint32_t rank = wave_histogram_rank(E.cell_count, ncell, keep);
  if (!keep) return;
  E.out.rank[i] = rank;
  if (Ep->halo_band) {
    if (late_check && halo_in_shared_band(P.g, Ep->halo_band, Ep->halo_send, ncell))
      atomicAdd(&E.ctr->n_halo_late, 1u);
    halo_pack_agent(P.g, Ep->halo_band, Ep->halo_send, ncell, nox, noy, wx, wy, id, meta_make(P.g, meta_group(P.g, meta), next_wp),
                    E.out.route ? route_st : 0u, E.ctr);
  }
  if (P.has_sinks) mark_sources(P.g, E.sinks, E.src_cell_start, E.src_sorted, E.src_occupied, ncell, nox, noy);
}

// writes a new value of the context (the kernel's argument) to its place in device memory
__global__ void k_store_ctx(EpilogueCtx value, EpilogueCtx* __restrict__ dst) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&value);
  uint32_t* out = reinterpret_cast<uint32_t*>(dst);
  for (uint32_t k = threadIdx.x; k < sizeof(EpilogueCtx) / sizeof(uint32_t); k += blockDim.x) out[k] = src[k];
}

// ---------------------------------------------------------------------------
// K4: the neighbour pass.  Phase B of Simulation::step for one agent
// (lib.rs:259-347): radius query (location_hash_2d.rs:240-258), Zanlungo
// (zanlungo.rs:201-217).  Two forms with the same arithmetic and the same visiting order (cells
// x-major / y-minor, members of a cell in ascending id: the canonical order of SURVEY.md §8a'),
// so their results are bitwise equal:
//   k_step_tiled   cell lists staged in LDS by the workgroup, per-lane neighbour lists (fast path)
//   GatherSrc      cell lists read from global memory (exact for any grid and any agent state:
//                  clamped, aliased, overfull tiles); k_step_gather and the fallback in k_step_tiled
// ---------------------------------------------------------------------------
#define CS_ROUTE_WP_SHIFT 22
#define CS_ROUTE_IDX_MASK 0x3FFFFFu

// RMFPlanner::get_desired_velocity, rmf/mod.rs:197-215, on the device: the agent's cached
// (route, waypoint) pair travels with it (AgentArrays::route); inside `arrive` of the current waypoint (and
// not at the last one) it moves on; the answer is the unit vector to the waypoint times speed
// (normalize() of a zero vector is NaN there too).  Waypoints are global f64; they are taken
// relative to the agent's cell origin and rounded once, like the sink test below.
__device__ __forceinline__ float2 route_velocity(const GroupDev& grp, const EpilogueCore& E, const GridDev& g,
                                                 uint32_t& st, uint32_t gx, uint32_t gy, float2 off) {
  if (st == 0u) return make_float2(0.0f, 0.0f);  // not in agent_cache: None
  const uint2 rd = E.route_desc[(st & CS_ROUTE_IDX_MASK) - 1u];
  uint32_t wp = st >> CS_ROUTE_WP_SHIFT;
  const double cx = E.grid_off_x + (double)(g.org_x + gx) * E.cell_size;
  const double cy = E.grid_off_y + (double)(g.org_y + gy) * E.cell_size;
  float ddx = (float)(E.route_xy[2 * (size_t)(rd.x + wp)] - cx) - off.x;
  float ddy = (float)(E.route_xy[2 * (size_t)(rd.x + wp) + 1] - cy) - off.y;
  float dist = sqrtf(ddx * ddx + ddy * ddy);
  if (dist < grp.hvy && wp + 1u < rd.y) {
    wp += 1u;
    st = (st & CS_ROUTE_IDX_MASK) | (wp << CS_ROUTE_WP_SHIFT);  // agent_cache.insert(id, (path, wp + 1))
    ddx = (float)(E.route_xy[2 * (size_t)(rd.x + wp)] - cx) - off.x;
    ddy = (float)(E.route_xy[2 * (size_t)(rd.x + wp) + 1] - cy) - off.y;
    dist = sqrtf(ddx * ddx + ddy * ddy);
  }
  const float k = grp.hvx / dist;
  return make_float2(ddx * k, ddy * k);
}

__device__ __forceinline__ float2 hlp_velocity(const GroupDev& grp, const EpilogueCore& E, const GridDev& g,
                                               uint32_t id, const float2* pref, uint32_t i, uint32_t gx,
                                               uint32_t gy, float2 off, uint32_t& route_st) {
  switch (grp.hlp_kind) {
    case CS_HLP_CONSTANT:
      return make_float2(grp.hvx, grp.hvy);
    case CS_HLP_ID_PARITY:  // rmf_crowdsim_viz/src/main.rs:26-29: even ids get -v
      return (id & 1u) ? make_float2(grp.hvx, grp.hvy) : make_float2(-grp.hvx, -grp.hvy);
    case CS_HLP_CALLBACK:
      return pref[i];
    case CS_HLP_ROUTE:
      return route_velocity(grp, E, g, route_st, gx, gy, off);
    default:
      return make_float2(0.0f, 0.0f);  // None: vel stays (0,0), lib.rs:263
  }
}

struct Own {
  float2 off, v, u;
  uint32_t id, gx, gy, slot;
};

// Members of one cell straight from the sorted global arrays.
struct GatherSrc {
  const AgentArrays& in;
  const uint32_t* __restrict__ cell_start;
  const GridDev& g;
  uint32_t self;
  __device__ __forceinline__ bool cell(long long x, long long y, uint32_t& b, uint32_t& e) const {
    if (x < 0 || y < 0) return false;  // signed_idx_to_data_idx, location_hash_2d.rs:74-85
    unsigned long long flat = (unsigned long long)x * g.nx + (unsigned long long)y;
    if (flat >= g.ncells) return false;
    b = cell_start[flat];
    e = cell_start[flat + 1];
    return true;
  }
  __device__ __forceinline__ bool is_self(uint32_t j) const { return j == self; }
  // offset of member j and the cell it is stored in, relative to the own cell (gx, gy); a member
  // reached through the aliasing of location_to_index (y beyond the stride) sits in another cell
  // than the (x, y) it was reached through
  __device__ __forceinline__ float2 off(uint32_t j, long long x, long long y, uint32_t gx, uint32_t gy, int& sx,
                                        int& sy) const {
    long long ax = x, ay = y;
    if (y >= (long long)g.nx) {  // reached through an aliased flat index
      const uint32_t c = in.cell[j];
      ax = c / g.nx;
      ay = c - (uint32_t)ax * g.nx;
    }
    const long long dx = ax - (long long)gx, dy = ay - (long long)gy;
    sx = (int)max(min(dx, 1000000ll), -1000000ll);
    sy = (int)max(min(dy, 1000000ll), -1000000ll);
    return in.off[j];
  }
  __device__ __forceinline__ float2 vel(uint32_t j) const { return in.vel[j]; }
  __device__ __forceinline__ uint32_t id(uint32_t j) const { return in.id[j]; }
  // k-th member of [b, e) in ascending id: storage order inside a cell is arrival order
  __device__ __forceinline__ uint32_t ordered(uint32_t b, uint32_t e, uint32_t k, uint32_t& last,
                                              bool& have_last) const {
    uint32_t best = 0xFFFFFFFFu, bj = b;
    bool found = false;
    for (uint32_t j = b; j < e; ++j) {
      uint32_t idj = in.id[j];
      if ((!have_last || idj > last) && (!found || idj < best)) {
        best = idj;
        bj = j;
        found = true;
      }
    }
    last = best;
    have_last = true;
    return bj;
  }
};

// Returns the new velocity w = u + F/m of agent `o` (zanlungo.rs:201-217).  Generic form:
// every candidate is processed where it is found.  Used by the gather kernel.
template <class Src>
__device__ __forceinline__ void zanlungo_velocity(const Own& o, const GroupDev& grp, const GridDev& g,
                                                  long long lx, long long hx, long long ly,
                                                  long long hy, const Src& src, float& wx, float& wy,
                                                  bool& tti_zero) {
  const float rs = grp.eyesight * g.fix_scale;
  const float nr2 = -(rs * rs);
  const float Rs = grp.R * g.fix_scale;
  const float R2 = Rs * Rs;  // fixed units, like the relative positions (cs_device_types: UNITS)
  // ---- compute_tti (zanlungo.rs:76-91): min over every neighbour in sight ----
  float T = f_inf();  // S * t_i
  uint32_t n_back = 0;
  for (long long x = lx; x <= hx; ++x) {
    for (long long y = ly; y <= hy; ++y) {
      uint32_t b, e;
      if (!src.cell(x, y, b, e)) continue;
      for (uint32_t j = b; j < e; ++j) {
        if (src.is_self(j)) continue;  // lib.rs:284
        int sx, sy;
        const float2 oj = src.off(j, x, y, o.gx, o.gy, sx, sy);
        float qx, qy;
        fix_rel(g, o.off, oj, sx, sy, qx, qy);  // p_j - p_i
        if (!(sight_margin(qx, qy, nr2) < 0.0f)) continue;  // strict `<`, location_hash_2d.rs:251
        const float d2 = __builtin_fmaf(qx, qx, qy * qy);
        const float2 vj = src.vel(j);
        const float t = ttc_pair_f32(vj.x - o.v.x, vj.y - o.v.y, qx, qy, d2, R2);
        T = (t < T) ? t : T;
        n_back += (src.id(j) < o.id) ? 1u : 0u;
      }
    }
  }
  tti_zero = (T == 0.0f);
  float fx = 0.0f, fy = 0.0f;
  if (T != f_inf()) {  // zanlungo.rs:211
    const ForceCtx fc = make_force_ctx(o.v.x, o.v.y, T, grp, g);
    for (long long x = lx; x <= hx; ++x) {
      for (long long y = ly; y <= hy; ++y) {
        uint32_t b, e;
        if (!src.cell(x, y, b, e)) continue;
        uint32_t last = 0;
        bool have_last = false;
        for (uint32_t k = 0; k < e - b; ++k) {
          const uint32_t j = src.ordered(b, e, k, last, have_last);
          if (!(src.id(j) > o.id)) continue;  // self and smaller ids: weight 0
          int sx, sy;
          const float2 oj = src.off(j, x, y, o.gx, o.gy, sx, sy);
          float qx, qy;
          fix_rel(g, o.off, oj, sx, sy, qx, qy);
          if (!(sight_margin(qx, qy, nr2) < 0.0f)) continue;
          const float d2 = __builtin_fmaf(qx, qx, qy * qy);
          zanlungo_forward_force(qx, qy, d2, fc, fx, fy);
        }
      }
    }
    // Neighbours with a smaller id have weight 0: their term is (d/|d|) * 0 = 0, except
    // with t_i == 0, where 0 * A * |dv| / 0 = NaN (zanlungo.rs:163; SURVEY.md KAT-Z3).
    if (T == 0.0f && n_back > 0) {
      fx = f_nan();
      fy = f_nan();
    }
  }
  wx = __builtin_fmaf(fx, grp.inv_mass, o.u.x);  // recommended + force * (1/m), zanlungo.rs:216
  wy = __builtin_fmaf(fy, grp.inv_mass, o.u.y);
}

// get_bounds (location_hash_2d.rs:103-122) from a cell-relative position: cell range
// [gx + lo, gx + hi] for radius r.  Saturating like Rust's `as i64`.  The range is widened by
// CS_BOUNDS_EPS cells on either side: membership is decided by the radius test on the fixed-point
// positions alone (both step kernels), and the range must hold every agent that passes it whatever
// the f32 rounding of this product (the reference's f64 bounds hold them all too); the tiled
// kernel's pair reads may then touch the slot before and after a run without a range test, because an
// agent outside the range cannot pass the radius test.
#define CS_BOUNDS_EPS 1e-5f
__device__ __forceinline__ void cell_bounds(float o, float r, float inv_cs, long long g, long long& lo,
                                            long long& hi) {
  float fl = floorf((o - r) * inv_cs - CS_BOUNDS_EPS), fh = floorf((o + r) * inv_cs + CS_BOUNDS_EPS);
  lo = g + (long long)fminf(fmaxf(fl, -4e9f), 4e9f);
  hi = g + (long long)fminf(fmaxf(fh, -4e9f), 4e9f);
}

__device__ __forceinline__ void gather_agent(const StepParams& P, const AgentArrays& in,
                                             const uint32_t* __restrict__ cell_start, const Own& o,
                                             const GroupDev& grp, float& wx, float& wy, bool& tz) {
  long long lx, hx, ly, hy;
  cell_bounds(o.off.x, grp.eyesight, P.g.inv_cs, o.gx, lx, hx);
  cell_bounds(o.off.y, grp.eyesight, P.g.inv_cs, o.gy, ly, hy);
  // rows and cells that cannot exist: negative ones are rejected by the reference,
  // flat indices beyond the grid too; y may run past the stride (aliasing) up to the
  // last flat index
  lx = max(lx, 0ll);
  ly = max(ly, 0ll);
  hx = min(hx, (long long)(P.g.ncells / P.g.nx));
  hy = min(hy, (long long)P.g.ncells);
  GatherSrc src{in, cell_start, P.g, o.slot};
  zanlungo_velocity(o, grp, P.g, lx, hx, ly, hy, src, wx, wy, tz);
}

// the second word behind EpilogueCtx::peek: the cumulative error counters as this step kernel finds them when it
// starts (those of the steps before it), for the host to look at without a wait (cs_engine: peek_errors)
__device__ __forceinline__ void step_peek_errors(unsigned long long* peek, const Counters* ctr) {
  const unsigned long long bad = (unsigned long long)ctr->n_out_of_bounds + ctr->n_halo_late + ctr->n_early_stalled + ctr->n_win_dropped + ctr->n_scan_stalled;
  __hip_atomic_store(peek + 1, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // the third word: the mesh's failure word as this step's halo unpack left it (Counters::mesh_fail_step)
  __hip_atomic_store(peek + 2, (unsigned long long)ctr->mesh_fail_step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void __launch_bounds__(256) k_step_gather(StepParams P, AgentArrays in,
                                                     const EpilogueCtx* __restrict__ Ep,
                                                     const uint32_t* __restrict__ cell_start,
                                                     const float2* __restrict__ pref) {
  const EpilogueCtx& E = *Ep;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && Ep->peek) {  // (tile engines: the host's slot bound, see StepParams::peek_seq)
    __hip_atomic_store(Ep->peek, ((unsigned long long)P.peek_seq << 32) | cell_start[P.g.ncells], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
    step_peek_errors(Ep->peek, E.ctr);
  }
  if (i >= P.n) return;
  if (i >= E.ctr->n_alive) {
    E.out.cell[i] = CS_INVALID_CELL;  // slot beyond the live population
    return;
  }
  if (E.ctr->n_out_of_bounds != 0u) return;  // the step has failed already (see k_step_tiled)
  const uint32_t cell = in.cell[i];
  Own o;
  o.gx = cell / P.g.nx;
  o.gy = cell - o.gx * P.g.nx;
  if (P.g.tile && (o.gx < P.g.own_x0 || o.gx >= P.g.own_x1 || o.gy < P.g.own_y0 || o.gy >= P.g.own_y1)) {
    E.out.cell[i] = CS_INVALID_CELL;  // a ghost: its owner steps it
    return;
  }
  o.off = in.off[i];
  o.v = in.vel[i];
  o.id = in.id[i];
  o.slot = i;
  const uint32_t meta = in.meta[i];
  const GroupDev grp = E.groups[meta_group(P.g, meta)];
  uint32_t route_st = in.route ? in.route[i] : 0u;
  o.u = hlp_velocity(grp, E, P.g, o.id, pref, i, o.gx, o.gy, o.off, route_st);
  float wx = o.u.x, wy = o.u.y;  // NoLocalPlan: identity, no_local_plan.rs:9-17
  if (grp.lp_kind == 2u && E.lp_vel) {  // a host LocalPlanner has answered for this agent (local_planner.rs:7-18)
    wx = E.lp_vel[i].x;
    wy = E.lp_vel[i].y;
  }
  if (grp.lp_kind == 1u && o.off.x == o.off.x && o.off.y == o.off.y) {
    bool tz;
    gather_agent(P, in, cell_start, o, grp, wx, wy, tz);
    if (tz) atomicAdd(&E.ctr->n_tti_zero, 1u);
  }
  step_epilogue(P, E, Ep, i, o.gx, o.gy, o.off, o.id, meta, grp, wx, wy, route_st, P.halo_late_check);
}

// Slow path of a host LocalPlanner: the velocity the high-level planner recommends (what the step kernels compute
// for themselves) for every agent of such a planner, by slot; the host reads it, asks the planner and writes the
// answers to the same array.  Route followers: the waypoint advance of route_velocity is NOT stored here (the step
// kernel makes it again and stores it).
__global__ void __launch_bounds__(256) k_lp_recommended(StepParams P, AgentArrays in, const EpilogueCtx* __restrict__ Ep,
                                                        const float2* __restrict__ pref, float2* __restrict__ out) {
  const EpilogueCtx& E = *Ep;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n || i >= E.ctr->n_alive) return;
  const uint32_t cell = in.cell[i];
  const uint32_t meta = in.meta[i];
  const GroupDev grp = E.groups[meta_group(P.g, meta)];
  if (grp.lp_kind != 2u) return;
  const uint32_t gx = cell / P.g.nx, gy = cell - gx * P.g.nx;
  uint32_t route_st = in.route ? in.route[i] : 0u;
  out[i] = hlp_velocity(grp, E, P.g, in.id[i], pref, i, gx, gy, in.off[i], route_st);
}

// ---------------------------------------------------------------------------
// Work decomposition for the tiled kernel: every workgroup gets up to 256
// consecutive agents of ONE grid row, so the cells it must see are (2h+1)
// contiguous ranges of the sorted arrays.  Built on the device after the scan.
// ---------------------------------------------------------------------------
#ifndef TILE_THREADS
#define TILE_THREADS 256  // agents (= threads) per workgroup of the tiled neighbour kernel
#endif

// A workgroup of the tiled kernel owns `nrows` consecutive grid rows x the cells [y0, y1].
// count != 0: a strip of one row cut at AGENT granularity (first, count <= TILE_THREADS).
// count == 0: a band window of nrows rows cut at CELL granularity (agents = the cells' members).
// cut != 0: a band window of one or two rows cut at AGENT granularity (build_band, plain windows): it owns the slots
// [first, first + count) of row row0 and [first1, first1 + count1) of row row0 + 1 (either may be empty), which need
// not be whole cells; y0 .. y1 are the columns of its first and last owned agent, the span it stages around.  The rest of
// a cell it owns only partly is staged like any ghost.
struct BlockDesc {
  uint32_t row0;
  unsigned short nrows, cut;
  uint32_t y0, y1, first, count, first1, count1;
};
static_assert(sizeof(BlockDesc) == 32, "a descriptor is two 16-byte scalar loads");

__global__ void __launch_bounds__(1024) k_build_blocks(GridDev g, const uint32_t* __restrict__ cell_start,
                                                       BlockDesc* __restrict__ desc, uint32_t desc_cap,
                                                       uint32_t* __restrict__ n_blocks,
                                                       Counters* __restrict__ ctr) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t s_carry, s_owned;
  if (threadIdx.x == 0) {
    s_carry = 0;
    s_owned = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // only the owned rows / columns get workgroups; ghosts are read, never stepped
  const uint32_t n_rows = g.own_x1 - g.own_x0;
  for (uint32_t base = 0; base < n_rows; base += blockDim.x) {
    uint32_t R = g.own_x0 + base + threadIdx.x;
    uint32_t first = 0, cnt = 0;
    if (R < g.own_x1) {
      first = cell_start[(unsigned long long)R * g.nx + g.own_y0];
      cnt = cell_start[(unsigned long long)R * g.nx + g.own_y1] - first;
    }
    uint32_t nb = (cnt + TILE_THREADS - 1u) / TILE_THREADS;
    uint32_t incl = wave_incl_scan(nb, lane);
    if (lane == 63) wsum[wave] = incl;
    if (cnt) atomicAdd(&s_owned, cnt);
    __syncthreads();
    uint32_t woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    uint32_t excl = s_carry + woff + incl - nb;
    for (uint32_t k = 0; k < nb; ++k) {
      if (excl + k < desc_cap) {
        BlockDesc d;
        d.row0 = R;
        d.nrows = 1;
        d.cut = 0;
        d.first1 = d.count1 = 0;
        d.y0 = d.y1 = 0;
        d.first = first + k * TILE_THREADS;
        d.count = min((uint32_t)TILE_THREADS, cnt - k * TILE_THREADS);
        desc[excl + k] = d;
      }
    }
    __syncthreads();
    if (threadIdx.x == blockDim.x - 1) s_carry = excl + nb;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *n_blocks = min(s_carry, desc_cap);
    ctr->n_owned = s_owned;
    // runs after the scatter, before the step kernel, which writes one slot per sorted agent
    ctr->n_pending = cell_start[g.ncells];
  }
}

// Band windows: one workgroup of this builder per band of `rb` owned rows.  The inclusive
// prefix of the per-column agent counts goes to LDS (or, for very wide bands, to `prefix`); a
// window is a run of columns.  A band never gets more than 2 * (its agents / target) + 1 windows
// (the launch of the step kernel is sized by that).  *n_blocks must be 0 on entry.
#define BAND_LDS_COLS 2048
__device__ __forceinline__ void build_band(const uint32_t band, const GridDev& g,
                                           const uint32_t* __restrict__ cell_start, uint32_t rb,
                                           uint32_t target, uint32_t h, uint32_t stage_cap,
                                           uint32_t max_cols, uint32_t split, uint32_t cover, uint32_t* __restrict__ prefix,
                                           BlockDesc* __restrict__ desc, uint32_t desc_cap,
                                           uint32_t* __restrict__ n_blocks, Counters* __restrict__ ctr) {
#define BAND_ARRAY(type, name, count) __shared__ type name[count];
#include "cs_kernel_band_builder.hip.inc"
#undef BAND_ARRAY
}

// ... with the large arrays in LDS the caller lends (BAND_SCRATCH_BYTES of it, 16-byte aligned): the builder workgroups
// of the neighbour kernel's launch
#define BAND_OFF_s_incl 0u
#define BAND_OFF_s_all (BAND_LDS_COLS * 4u)
#define BAND_OFF_s_end (BAND_LDS_COLS * 8u)
#define BAND_OFF_s_next (BAND_LDS_COLS * 10u)
#define BAND_OFF_s_win (BAND_LDS_COLS * 12u)
#define BAND_OFF_s_cls (BAND_LDS_COLS * 14u)
#define BAND_SCRATCH_BYTES (BAND_LDS_COLS * 16u)
__device__ __noinline__ void build_band_in(unsigned char* band_scratch, const uint32_t band, const GridDev& g,
                                           const uint32_t* __restrict__ cell_start, uint32_t rb,
                                           uint32_t target, uint32_t h, uint32_t stage_cap,
                                           uint32_t max_cols, uint32_t split, uint32_t cover, uint32_t* __restrict__ prefix,
                                           BlockDesc* __restrict__ desc, uint32_t desc_cap,
                                           uint32_t* __restrict__ n_blocks, Counters* __restrict__ ctr) {
#define BAND_ARRAY(type, name, count) type* const name = reinterpret_cast<type*>(band_scratch + BAND_OFF_##name);
#include "cs_kernel_band_builder.hip.inc"
#undef BAND_ARRAY
}


__global__ void __launch_bounds__(256) k_build_bands(GridDev g, const uint32_t* __restrict__ cell_start,
                                                     uint32_t rb, uint32_t target, uint32_t h,
                                                     uint32_t stage_cap, uint32_t max_cols, uint32_t split, uint32_t cover,
                                                     uint32_t* __restrict__ prefix,
                                                     BlockDesc* __restrict__ desc, uint32_t desc_cap,
                                                     uint32_t* __restrict__ n_blocks,
                                                     Counters* __restrict__ ctr) {
  build_band(blockIdx.x, g, cell_start, rb, target, h, stage_cap, max_cols, split, cover, prefix, desc, desc_cap, n_blocks, ctr);
}

// K3 and the band builder in one launch (both need only the finished cell_start): blocks
// [0, band_blocks) build one band each, the rest scatter records into cell order.  The builders
// come first because each is a chain of dependent LDS searches (~10 us): dispatched last they
// were the tail of the launch, dispatched first they finish under the scatter.  On a tile
// engine the scatter also marks every source slot dead: that buffer receives the step kernel's
// output next, and ghosts get no thread there.
__global__ void __launch_bounds__(256) k_scatter_and_bands(AgentArrays src, AgentArrays dst, uint32_t n,
                                                           const uint32_t* __restrict__ cell_start,
                                                           uint32_t band_blocks, GridDev g, uint32_t rb,
                                                           uint32_t target, uint32_t h, uint32_t stage_cap,
                                                           uint32_t max_cols, uint32_t split, uint32_t cover,
                                                           uint32_t* __restrict__ prefix,
                                                           BlockDesc* __restrict__ desc, uint32_t desc_cap,
                                                           uint32_t* __restrict__ n_blocks,
                                                           Counters* __restrict__ ctr) {
  if (blockIdx.x < band_blocks) {
    build_band(blockIdx.x, g, cell_start, rb, target, h, stage_cap, max_cols, split, cover, prefix, desc, desc_cap, n_blocks, ctr);
    return;
  }
  const uint32_t i = (blockIdx.x - band_blocks) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i >= cell_start[g.ncells]) dst.cell[i] = CS_INVALID_CELL;  // stale slots beyond the live records (see k_scatter)
  if (g.tile) {
    const bool live = i < ctr->n_pending;  // slots beyond the device-side count hold stale records
    const uint32_t c0 = live ? src.cell[i] : CS_INVALID_CELL;
    src.cell[i] = CS_INVALID_CELL;
    if (c0 == CS_INVALID_CELL) return;
    const uint32_t d0 = cell_start[c0] + src.rank[i];
    dst.off[d0] = src.off[i];
    dst.vel[d0] = src.vel[i];
    dst.id[d0] = src.id[i];
    dst.cell[d0] = c0;
    dst.meta[d0] = src.meta[i];
    if (src.route) dst.route[d0] = src.route[i];
    return;
  }
  const uint32_t c = src.cell[i];
  if (c == CS_INVALID_CELL) return;
  const uint32_t d = cell_start[c] + src.rank[i];
  dst.off[d] = src.off[i];
  dst.vel[d] = src.vel[i];
  dst.id[d] = src.id[i];
  dst.cell[d] = c;
  dst.meta[d] = src.meta[i];
  if (src.route) dst.route[d] = src.route[i];
}

// Profiling build only (-DCS_PHASE_CLOCKS, tools/phase_clocks.py): wave cycles per phase of the
// tiled kernel, summed over all waves.  0 descriptor, 1 geometry, 2 staging loads, 3 first staging
// barrier, 4 placement, 5 second staging barrier, 6 per-agent setup, 7 filter, 8 time-to-collision,
// 9 forces, 10 epilogue.
#ifdef CS_PHASE_CLOCKS
#define PHASE_SLOTS 256  // spread the final atomics over many addresses
#define PHASE_COUNT 12
__device__ unsigned long long g_phase_cycles[PHASE_SLOTS][PHASE_COUNT];
#define PHASE_BEGIN()                  \
  unsigned long long ph_last = clock64(); \
  unsigned long long ph_acc[PHASE_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define PHASE_MARK(p)                            \
  do {                                           \
    const unsigned long long ph_now = clock64(); \
    ph_acc[p] += ph_now - ph_last;               \
    ph_last = ph_now;                            \
  } while (0)
#define PHASE_END()                                                                      \
  do {                                                                                   \
    if ((threadIdx.x & 63) == 0)                                                         \
      for (int ph_k = 0; ph_k < PHASE_COUNT; ++ph_k)                                               \
        atomicAdd(&g_phase_cycles[(blockIdx.x * 4 + (threadIdx.x >> 6)) % PHASE_SLOTS][ph_k], ph_acc[ph_k]); \
  } while (0)
#else
#define PHASE_BEGIN() do { } while (0)
#define PHASE_MARK(p) do { } while (0)
#define PHASE_END() do { } while (0)
#endif

#ifndef CS_K4_WAVES
#define CS_K4_WAVES 4  // workgroups per CU the register allocation of the tiled kernel aims at
#endif
#define TILE_MAX_ROWS 24  // owned rows (<= 8) + 2 * 8 ghost rows: eyesight up to 8 cells
#define TILE_LIST_SPARE 1u  // list rows behind the last one (branch-free appends; an odd list's repeated last entry)
#define TILE_MAX_OWN_ROWS 8
#define TILE_AGENTS_MAX 6144u  // most LDS slots for staged agents a window may be given (cs_engine: tile_agents_cap)

struct TileCfg {
  int h;                // ceil(max eyesight / cell)
  uint32_t agents_cap;  // LDS slots for staged agents
  uint32_t table_cap;   // u16 entries of the cell table
  uint32_t list_cap;    // neighbour-list entries per thread in LDS (even)
  uint32_t debug;       // ablation switches, read only by a -DCS_TILE_ABLATION build (bench.py --debug)
  // Entries list_cap .. list_cap + spill_rows - 1 of a lane's list live in global memory:
  // spill[(workgroup * spill_rows + row) * TILE_THREADS + thread], 32-bit each.  A crowd whose
  // neighbour counts scatter (anything but a lattice) has a few lanes per wave beyond list_cap;
  // without the spill the whole wave would run the filter twice.  list_cap + spill_rows <= 128
  // (the right-of-way masks of pass 2 have 64 bits for the LDS rows + 64 for spilled ones).
  uint32_t* spill;
  uint32_t spill_rows;
  // which window list this launch walks: 0 = desc[0 .. n_blocks[0]), 1 = the border windows
  // desc[desc_cap - 1 - k], k < n_blocks[1] (build_band, split != 0)
  uint32_t part;
  uint32_t desc_cap;
  // the descriptor array holds two lists (build_band, split != 0), each of desc_cap / 2.  2: this ONE launch walks both,
  // the border windows in its first workgroups; the last border window to finish stores flag_seq in
  // Counters::border_flag (the "early exchange" form of CS_CFG_TILE_OVERLAP, cs_engine)
  uint32_t split;
  uint32_t flag_seq;
  uint32_t build_sel;  // builder workgroups (k_step_tiled<..., true>): which of EpilogueCtx::build_desc they fill
};

#if defined(CS_TILE_ABL)  // compile-time ablation (tools/abl_variants.sh): the switched-off parts are not even compiled
#define TILE_DEBUG(bit) (((CS_TILE_ABL) & (bit)) != 0)
#elif defined(CS_TILE_ABLATION)
#define TILE_DEBUG(bit) (cfg.debug & (bit))
#else
#define TILE_DEBUG(bit) false
#endif

// K4 (tiled form): one workgroup = one BlockDesc = a band window (a few owned grid rows x a run
// of columns holding up to 256 agents) or, with 1-row strips, up to 256 consecutive agents of one
// row.  The cell-row segments around the window (owned rows + h ghost rows on either side) are
// staged in LDS once: members of a cell in ascending id, positions in WINDOW-RELATIVE fixed point
// (fix_rel: the difference of two staged positions is the exact p_j - p_i whatever the window),
// every staged row starting at an even slot.  Then every thread runs the neighbour pass of its agent:
//   1. distance filter: per staged row in reach ONE contiguous run of slots (the cells in reach
//      are neighbours in the sorted order), two candidates per 16-byte LDS read -> compacted
//      list of slots (LDS rows, further rows spilled to global memory)
//   2. time-to-collision over the list (min -> t_i); the neighbours with right of way
//      (larger id) are remembered in lane masks (64 bits, 128 with CS_CFG_DENSE)
//   3. forces over the marked entries, in list (= canonical) order
// A lane that needs more entries than list + spilled rows hold makes its wave process what it
// has and carry on (pass 3 then re-runs the filter, since the list was recycled).
// 4 waves per SIMD = 4 workgroups per CU is what the LDS budget allows; pinning it keeps the
// register allocator at <= 128 VGPRs (one more and a CU holds 3 workgroups).
// CTX_BY_VALUE = false: the epilogue's tables (~50 dwords, most of them read once per agent at
// most) stay in device memory (Ep); as kernel arguments they sat in SGPRs across the whole kernel
// and spilled into VGPR lanes (753 v_readlane / v_writelane sites, 162 -> 157 us on the bench
// scene).  CTX_BY_VALUE = true: crowds with source-sinks or route followers, whose every agent runs
// the waypoint test: there each table read from memory is a scalar load the agent waits for
// (178 us against 141 us with the tables in registers, 850k agents of 25,000 sinks).
// WITH_BUILDERS = true: the instantiation small crowds run (cs_engine, "the window builder off the critical path"): the
// first Ep->build_bands workgroups cut the next step's band windows.  A kernel of its own because the mere presence of
// that branch (an out-of-line call: a stack frame, other spill decisions) cost the plain kernel 2 % at 1M agents.
// EARLY = true: the early-exchange form of CS_CFG_TILE_OVERLAP (TileCfg::split == 2: one launch over both window lists, the
// border windows first, counting themselves off).  An instantiation of its own for the reason WITH_BUILDERS is one: with
// the code merely present the plain kernel lost 1.1 % at 1M agents (profiles/r05/variants_early.txt).
// XF = true: windows that stage at most TILE_XF_ROWS rows (h = 1 with one- or two-row bands, strips: the host's choice,
// cs_engine) keep a staged x as the BITS OF A FLOAT.  Such an x is (k - kc) cs_fix + fix_coord with k - kc in [-2, 1] and
// cs_fix <= 2^23, an integer of magnitude <= 2^24 = TILE_XF_LIM and so exact in f32; for two exact operands the f32
// difference x_j - x_i is the correctly rounded exact difference, which is what (float)(x_j - x_i) of the integer form is,
// +0 for equal operands included (tests/test_staged_x_exact.py).  The loops below then form x_j - x_i with one full-rate
// subtraction where the integer form needs a subtraction and a half-rate conversion.  The range is enforced while placing
// (s_huge, bit 1): a record beyond it, an agent clamped or aliased outside its cell, sends the window down the gather path for
// this step.  y runs along the window (up to 2^26 units) and stays an integer.  XF = false is the integer form throughout.
#define TILE_XF_ROWS 4
#define TILE_XF_LIM 0x1000000  /* 2^24 */
template <bool CTX_BY_VALUE, bool WITH_BUILDERS, bool EARLY = false, bool XF = false>
__global__ void __launch_bounds__(TILE_THREADS, CS_K4_WAVES) k_step_tiled(
    StepParams P, AgentArrays in, const EpilogueCtx* __restrict__ Ep, EpilogueCore Ev,
    const uint32_t* __restrict__ cell_start, const float2* __restrict__ pref, const BlockDesc* __restrict__ desc,
    const uint32_t* __restrict__ n_blocks, TileCfg cfg) {
  const EpilogueCore& E = CTX_BY_VALUE ? Ev : static_cast<const EpilogueCore&>(*Ep);
  typedef unsigned short entry_t;  // a list entry is the LDS slot of the neighbour
  // the lean filter advances its list cursor by one ROW through a bit mask (`& row_bytes`), stores entries with 16-bit
  // LDS writes, and the lean time-to-collision pass walks at most 64 entries of a lane: all three hang on this layout
  static_assert(sizeof(entry_t) == 2, "list entries are 16-bit LDS slots (lds_st_u16)");
  static_assert(TILE_THREADS * sizeof(entry_t) == 512, "a list row is 512 bytes: the filter's cursor arithmetic needs a power of two it knows");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // per staged row: first global index, real prefix (agents), padded prefix (LDS slots, even)
  __shared__ uint32_t s_g0[TILE_MAX_ROWS], s_rc[TILE_MAX_ROWS + 1], s_base[TILE_MAX_ROWS + 1];
  {  // slots beyond the live population must not look alive to the next scatter
    const uint32_t t = E.ctr->n_alive + blockIdx.x * TILE_THREADS + threadIdx.x;
    if (t < P.n) E.out.cell[t] = CS_INVALID_CELL;
    // the step writes one slot per sorted agent: the slot count the halo kernels start from
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const uint32_t n_sorted = cell_start[P.g.ncells];
      E.ctr->n_pending = n_sorted;
      if (Ep->peek) {
        __hip_atomic_store(Ep->peek, ((unsigned long long)P.peek_seq << 32) | n_sorted, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        step_peek_errors(Ep->peek, E.ctr);
      }
    }
  }
  // Small crowds: the first build_bands workgroups of the launch cut the NEXT step's band windows (one band each, into the
  // other descriptor array, in the dynamic LDS a window would use); the windows of this step follow behind them.
  uint32_t n_builders = 0u;
  if constexpr (WITH_BUILDERS) {
    n_builders = Ep->build_bands;
    if (blockIdx.x < n_builders) {  // (block-uniform)
      build_band_in(smem, blockIdx.x, Ep->build_g, cell_start, Ep->build_rows, Ep->build_target, (uint32_t)Ep->build_g_h, Ep->build_stage_cap,
                    Ep->build_max_cols, 0u, 1u, Ep->build_prefix, Ep->build_desc[cfg.build_sel & 1u], Ep->build_desc_cap,
                    Ep->build_n_blocks[cfg.build_sel & 1u], E.ctr);
      return;
    }
  }
  const uint32_t lidx = blockIdx.x - n_builders;  // this workgroup's place in the launch (its spill area)
  uint32_t widx = lidx, part = cfg.part, n_first = 0u;  // its window, and the list the window is in
  if (EARLY && cfg.split == 2u) {  // one launch over both lists, the border windows first (TileCfg::split)
    n_first = min(n_blocks[1], cfg.desc_cap >> 1);
    part = lidx < n_first ? 1u : 0u;
    widx = part ? lidx : lidx - n_first;
    if (lidx == 0 && threadIdx.x == 0 && n_first + min(n_blocks[0], cfg.desc_cap >> 1) > gridDim.x - n_builders)
      atomicAdd(&E.ctr->n_win_dropped, 1u);
    if (lidx == 0 && threadIdx.x == 0 && n_first == 0u)  // (no border windows at all: nobody else would publish)
      __hip_atomic_store(&E.ctr->border_flag, cfg.flag_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
  // (never beyond what the descriptor lists hold, whatever the builder counted; windows this launch has no
  // workgroup for are reported: their agents go unstepped)
  if (!(EARLY && cfg.split == 2u) && widx == 0 && threadIdx.x == 0 && n_blocks[part] > min(gridDim.x - n_builders, cfg.desc_cap >> (cfg.split ? 1 : 0)))
    atomicAdd(&E.ctr->n_win_dropped, 1u);
  if (widx >= min(n_blocks[part], cfg.desc_cap >> (cfg.split ? 1 : 0))) return;
  const uint32_t late_check = (EARLY && cfg.split == 2u && part) ? 0u : P.halo_late_check;
  // a border window of such a launch counts itself off wherever it leaves: the last one publishes the launch's number
  // (everything the workgroup has written, the halo records it packed among it, is released at agent scope first)
#define BORDER_DONE()                                                                                              \
  do {                                                                                                             \
    if (EARLY && cfg.split == 2u && part) {                                                                        \
      __syncthreads();                                                                                             \
      if (threadIdx.x == 0) {                                                                                      \
        __threadfence();                                                                                           \
        if (atomicAdd(&E.ctr->border_done, 1u) + 1u == n_first) {                                                  \
          E.ctr->border_done = 0u;                                                                                 \
          __hip_atomic_store(&E.ctr->border_flag, cfg.flag_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);      \
        }                                                                                                          \
      }                                                                                                            \
    }                                                                                                              \
  } while (0)
  PHASE_BEGIN();
  // Staging is a chain of memory round trips with few instructions in between: they issue ahead
  // of the other workgroups' arithmetic (their loops do not notice, the chain gets shorter:
  // 156 -> 153 us).  Back to the default priority once the tile is in LDS.
  __builtin_amdgcn_s_setprio(3);
  const BlockDesc d = desc[part ? cfg.desc_cap - 1u - widx : widx];
#ifdef CS_PHASE_CLOCKS
  if (d.row0 == 0xFFFFFFF0u) return;  // (waits for the descriptor)
#endif
  PHASE_MARK(0);
  const GridDev g = P.g;
  const int tid = threadIdx.x;
  int2* __restrict__ s_pos = reinterpret_cast<int2*>(smem);
  float2* __restrict__ s_vel = reinterpret_cast<float2*>(s_pos + cfg.agents_cap);
  uint32_t* __restrict__ s_id = reinterpret_cast<uint32_t*>(s_vel + cfg.agents_cap);
  entry_t* __restrict__ s_list = reinterpret_cast<entry_t*>(s_id + cfg.agents_cap);  // [cap][256]
  // ids in arrival order, needed only while staging: they borrow the (still unused) list area
  uint32_t* __restrict__ s_idtmp = reinterpret_cast<uint32_t*>(s_list);
  unsigned short* __restrict__ s_tab =  // after the list rows and their spare row
      reinterpret_cast<unsigned short*>(s_list + (cfg.list_cap + TILE_LIST_SPARE) * TILE_THREADS);

  // ---- geometry of the owned rows x cells and their halo ----
  __shared__ uint32_t s_rfirst[TILE_MAX_OWN_ROWS], s_rpref[TILE_MAX_OWN_ROWS + 1];
  __shared__ unsigned short s_self[TILE_THREADS];  // LDS slot of the first chunk's owned agents
  // some staged agent moves at 2^31 m/s or more (the model has thrown it, zanlungo.rs:165-167): the workgroup's
  // time-to-collision passes then take the guarded form, which rescales such pairs (ttc_huge)
  // XF: bit 1 of the same word (no LDS of its own: the host prices a workgroup's static arrays) says that some staged
  // record's x lies beyond +-TILE_XF_LIM, so is not exact as a float: the window leaves the LDS path for this step.  Both
  // bits are set while placing (there with atomicOr, so that neither write loses the other) and read behind the barrier
  // that ends the staging.
  __shared__ uint32_t s_huge;
  // An agent has left the grid (this step or, with nobody waiting for reports, an earlier one): the step has failed,
  // the engine is poisoned at the next synchronisation, and whatever this launch computed would be thrown away.
  // Without this, a crowd whose model has blown up (everybody NaN in cell 0) costs tens of seconds per step until
  // somebody looks (tools/fuzz_more.py kernels, seed 1010: 35 s per step).  ONE thread reads the counter and the
  // workgroup decides together behind the first barrier below: waves that read it themselves could disagree (another
  // workgroup's epilogue may raise it in between), and a wave that left alone would leave the rest with a half-built tile.
  __shared__ uint32_t s_dead;
  if (threadIdx.x == 0) {
    s_huge = 0u;
    s_dead = E.ctr->n_out_of_bounds;
  }
  const int n_rows = (int)(g.ncells / g.nx);
  const int row0 = (int)d.row0, nown = (int)d.nrows;
  const bool strip = d.count != 0 && !d.cut;  // a one-row strip (k_build_blocks), else a band window
  int ylo, yhi;
  if (strip) {
    const uint32_t c_lo = in.cell[d.first], c_hi = in.cell[d.first + d.count - 1];
    ylo = (int)(c_lo - (uint32_t)row0 * g.nx);
    yhi = (int)(c_hi - (uint32_t)row0 * g.nx);
  } else {
    ylo = (int)d.y0;
    yhi = (int)d.y1;
  }
  const int sy0 = max(ylo - cfg.h, 0), sy1 = min(yhi + cfg.h, (int)g.nx - 1);
  const int W1 = sy1 - sy0 + 2;
  const int r0 = max(row0 - cfg.h, 0), r1 = min(row0 + nown - 1 + cfg.h, n_rows - 1);
  const int nr = r1 - r0 + 1;
  if (tid < nr) {
    unsigned long long rowbase = (unsigned long long)(r0 + tid) * g.nx;
    uint32_t g0 = cell_start[rowbase + sy0], g1 = cell_start[rowbase + sy1 + 1];
    s_g0[tid] = g0;
    s_rc[tid + 1] = g1 - g0;
  }
  if (tid >= 64 && tid < 64 + nown) {  // the owned agents of each owned row (another wave)
    const int r = tid - 64;
    if (strip) {
      s_rfirst[0] = d.first;
      s_rpref[1] = d.count;
    } else if (d.cut) {  // a band window cut at agent granularity: the builder has named the slots (nown <= 2)
      s_rfirst[r] = r ? d.first1 : d.first;
      s_rpref[r + 1] = r ? d.count1 : d.count;
    } else {
      const unsigned long long rowbase = (unsigned long long)(row0 + r) * g.nx;
      const uint32_t f = cell_start[rowbase + ylo];
      s_rfirst[r] = f;
      s_rpref[r + 1] = cell_start[rowbase + yhi + 1] - f;
    }
  }
  __syncthreads();
  if (s_dead != 0u) {  // (the whole workgroup: see s_dead)
    BORDER_DONE();
    return;
  }
  if (tid == 0) {
    uint32_t acc = 0, pad = 0;
    s_rc[0] = 0;
    s_base[0] = 0;
    for (int k = 0; k < nr; ++k) {
      const uint32_t c = s_rc[k + 1];
      acc += c;
      // every staged row starts at an even slot (16-byte pair reads) and ends with at least one slot
      // nobody can see: a pair read may run one slot past a run, never into the next row
      pad += (c + 2u) & ~1u;
      s_rc[k + 1] = acc;
      s_base[k + 1] = pad;
    }
    acc = 0;
    s_rpref[0] = 0;
    for (int k = 0; k < nown; ++k) {
      uint32_t c = s_rpref[k + 1];
      s_rpref[k + 1] = acc + c;
      acc += c;
    }
  }
  __syncthreads();
  const uint32_t S_real = s_rc[nr];
  const uint32_t S = s_base[nr];  // LDS slots in use (even)
  const uint32_t n_own = s_rpref[nown];
  // A window nobody stands in (a filler of a kept list, cs_engine "windows kept", whose cells are still empty) has nothing
  // to do.  Read from LDS behind the barrier: the whole workgroup leaves.  (Only in the instantiation that runs kept
  // lists step after step; the plain kernel meets fillers in the one step that cuts such a list.)
  if constexpr (WITH_BUILDERS) {
    if (n_own == 0u) {
      BORDER_DONE();
      return;
    }
  }
  // the staged tile must fit the LDS slots, the u16 list entries and table, and the fixed-point
  // range of window-relative positions (W1 columns, nr rows of cs_fix units each)
  // (positions are measured from the middle of the staged tile: |p| <= (W1 / 2 + 2) cells)
  const int kc = nr / 2, cyc = W1 / 2;
  // (+ 2: an aligned pair of invisible slots behind the tile, where lanes past their run look)
  const bool tiled_ok = S + 2u <= cfg.agents_cap && S < 65533u && (uint32_t)(nr * W1) <= cfg.table_cap &&
                        (long long)(W1 / 2 + 2) * g.cs_fix <= (long long)FIX_LIM &&
                        (long long)(nr / 2 + 2) * g.cs_fix <= (long long)FIX_LIM && (!XF || nr <= TILE_XF_ROWS);

  // The first chunk's own agents: their loads do not depend on the tile, so they are issued
  // before the staging round trips and travel together with them.
  struct OwnIn {
    uint32_t i, cell, id, meta, route;
    float2 off, v;
    GroupDev grp;
    int own_r;
    bool active;
  };
  auto load_own = [&](uint32_t chunk) {
    OwnIn L;
    const uint32_t a_idx = chunk + (uint32_t)tid;
    L.active = a_idx < n_own;
    L.own_r = 0;
    if (L.active)
      while (L.own_r + 1 < nown && a_idx >= s_rpref[L.own_r + 1]) ++L.own_r;
    L.i = L.active ? s_rfirst[L.own_r] + (a_idx - s_rpref[L.own_r]) : (n_own ? s_rfirst[0] : 0u);
    L.cell = in.cell[L.i];
    L.off = in.off[L.i];
    L.v = in.vel[L.i];
    L.id = in.id[L.i];
    L.meta = in.meta[L.i];
    L.route = in.route ? in.route[L.i] : 0u;
    // (an idle lane looks at slot 0 or at the window's first agent; slot 0 holds no record when the engine is empty, a
    // tile the crowd has not reached whose slot count is a host-side upper bound: whatever group number lay there must
    // not index the table)
    L.grp = E.groups[L.active ? meta_group(P.g, L.meta) : 0u];
    return L;
  };
  if (tid == 0 && (!tiled_ok || n_own > (uint32_t)TILE_THREADS)) {  // (rare: cs_kernel_stat)
    if (!tiled_ok) atomicAdd(&E.ctr->n_win_off_lds, 1u);
    if (n_own > (uint32_t)TILE_THREADS) atomicAdd(&E.ctr->n_win_chunked, 1u);
  }
  PHASE_MARK(1);
#ifdef CS_PHASE_CLOCKS
  // slot 11: waves of windows that leave the LDS path (low word) or are walked in chunks (high word)
  ph_acc[11] += (tiled_ok ? 0ull : 1ull) + (n_own > (uint32_t)TILE_THREADS ? (1ull << 32) : 0ull);
#endif
  const OwnIn first_own = load_own(0);

  // window-relative fixed-point position of an agent of staged row k, staged column cy
  auto window_pos = [&](float2 off, int k, int cy) {
    int2 p;
    const bool ok = fix_ok(off.x, g) && fix_ok(off.y, g);
    p.x = ok ? fix_coord(off.x, g) + (k - kc) * g.cs_fix : FIX_FAR;
    p.y = ok ? fix_coord(off.y, g) + (cy - cyc) * g.cs_fix : FIX_FAR;
    return p;
  };
  // the x of a staged slot: XF, the bits of the float (FIX_FAR = 2^30 is exact too); else the integer
  auto stage_x = [&](int x) {
    if constexpr (XF) return __float_as_int((float)x);
    else return x;
  };
  const int far_x = stage_x(FIX_FAR);

  if (tiled_ok) {
    // Staged agent s of the tile = member (s - s_rc[k]) of staged row k; its id goes to a
    // scratch array in arrival (= global) order, so that its rank inside its cell can be
    // counted from LDS, and the record is then placed at the cell's first slot + that rank.
    constexpr int STAGE_REGS = 4;
    // an owned agent of the first chunk: its thread finds its own slot in s_self
    auto note_self = [&](int k, uint32_t gj, uint32_t slot) {
      const int r = (r0 + k) - row0;
      if (r >= 0 && r < nown) {
        const uint32_t first = s_rfirst[r], a_idx = s_rpref[r] + (gj - first);
        if (gj >= first && a_idx < s_rpref[r + 1] && a_idx < (uint32_t)TILE_THREADS) s_self[a_idx] = (unsigned short)slot;
      }
    };
    auto place = [&](int k, uint32_t gj, uint32_t cellj, uint32_t idj, float2 offj, float2 velj) {
      const int cy = (int)(cellj - (uint32_t)(r0 + k) * g.nx) - sy0;
      const unsigned short* t = s_tab + k * W1 + cy;
      const uint32_t tb = t[0], te = t[1];
      uint32_t rank = 0;
      {  // four ids per trip: their reads are in flight together (the build does not unroll)
        uint32_t q = tb;
        for (; q + 4u <= te; q += 4u) {
          const uint32_t a0 = s_idtmp[q], a1 = s_idtmp[q + 1u], a2 = s_idtmp[q + 2u], a3 = s_idtmp[q + 3u];
          rank += ((a0 < idj) ? 1u : 0u) + ((a1 < idj) ? 1u : 0u) + ((a2 < idj) ? 1u : 0u) + ((a3 < idj) ? 1u : 0u);
        }
        for (; q < te; ++q) rank += (s_idtmp[q] < idj) ? 1u : 0u;
      }
      const uint32_t slot = tb + rank;
      int2 p = window_pos(offj, k, cy);
      if constexpr (XF) {  // (an agent staged at FIX_FAR is out of everybody's sight in either form)
        if (p.x != FIX_FAR && (uint32_t)(p.x + TILE_XF_LIM) > 2u * (uint32_t)TILE_XF_LIM) atomicOr(&s_huge, 2u);
        p.x = stage_x(p.x);
      }
      s_pos[slot] = p;
      s_vel[slot] = velj;
      s_id[slot] = idj;
      if (fmaxf(fabsf(velj.x), fabsf(velj.y)) >= 0.5f * TTC_HUGE_SPEED) {
        if constexpr (XF) atomicOr(&s_huge, 1u);
        else s_huge = 1u;
      }
      note_self(k, gj, slot);
    };
    auto fill_table = [&]() {  // first LDS slot of every staged cell (+ one end marker per row)
      // (a wave per staged row, a lane per column: the usual 4 rows x ~15 columns are one pass)
      for (int k = tid >> 6; k < nr; k += TILE_THREADS / 64) {
        const unsigned long long rowbase = (unsigned long long)(r0 + k) * g.nx + sy0;
        for (int y = tid & 63; y < W1; y += 64)
          s_tab[k * W1 + y] = (unsigned short)(s_base[k] + (cell_start[rowbase + y] - s_g0[k]));
      }
      if (tid >= TILE_THREADS - 2) {  // the invisible pair behind the tile (slots S, S + 1)
        const uint32_t q = S + (uint32_t)(tid - (TILE_THREADS - 2));
        s_pos[q] = make_int2(far_x, FIX_FAR);
        s_vel[q] = make_float2(0.f, 0.f);
        s_id[q] = 0u;
      }
      // the one or two slots that pad a row to an even length: agents nobody can see
      if (tid < 2 * nr) {
        const int k = tid >> 1;
        const uint32_t c = s_rc[k + 1] - s_rc[k], q = c + (uint32_t)(tid & 1);
        if (s_base[k] + q < s_base[k + 1]) {
          s_pos[s_base[k] + q] = make_int2(far_x, FIX_FAR);
          s_vel[s_base[k] + q] = make_float2(0.f, 0.f);
          s_id[s_base[k] + q] = 0u;
        }
      }
    };
    // the staged row of record s0: rows' first records are s_rc[1 .. nr - 1] (wave-uniform, read once)
    uint32_t rc_b[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) rc_b[q] = q + 1 < nr ? s_rc[q + 1] : 0xFFFFFFFFu;
    auto row_of = [&](uint32_t s0) {
      int k = 0;
      if (nr <= 6) {
#pragma unroll
        for (int q = 0; q < 5; ++q) k += (s0 >= rc_b[q]) ? 1 : 0;
      } else {
        while (s0 >= s_rc[k + 1]) ++k;
      }
      return k;
    };
    if (S_real <= STAGE_REGS * TILE_THREADS) {
      // common case: every thread holds its (<= 4) records in registers, so ids, cells,
      // offsets, velocities and the cell table are ONE round trip to memory
      uint32_t rid[STAGE_REGS], rcell[STAGE_REGS], rj[STAGE_REGS];
      int rk[STAGE_REGS];
      float2 roff[STAGE_REGS], rvel[STAGE_REGS];
#pragma unroll
      for (int m = 0; m < STAGE_REGS; ++m) {
        const uint32_t s0 = (uint32_t)tid + (uint32_t)m * TILE_THREADS;
        rk[m] = 0;
        rid[m] = 0;
        rj[m] = 0;
        rcell[m] = 0;
        roff[m] = make_float2(0.f, 0.f);
        rvel[m] = make_float2(0.f, 0.f);
        if (s0 < S_real) {
          const int k = row_of(s0);
          const uint32_t j = s_g0[k] + (s0 - s_rc[k]);
          rk[m] = k;
          rj[m] = j;
          rid[m] = in.id[j];
          rcell[m] = in.cell[j];
          roff[m] = in.off[j];
          rvel[m] = in.vel[j];
        }
      }
      fill_table();
#pragma unroll
      for (int m = 0; m < STAGE_REGS; ++m) {
        const uint32_t s0 = (uint32_t)tid + (uint32_t)m * TILE_THREADS;
        if (s0 < S_real) s_idtmp[s_base[rk[m]] + (s0 - s_rc[rk[m]])] = rid[m];
      }
      PHASE_MARK(2);
      __syncthreads();
      PHASE_MARK(3);
#pragma unroll
      for (int m = 0; m < STAGE_REGS; ++m) {
        const uint32_t s0 = (uint32_t)tid + (uint32_t)m * TILE_THREADS;
        if (s0 < S_real) place(rk[m], rj[m], rcell[m], rid[m], roff[m], rvel[m]);
      }
    } else {
      fill_table();
      for (uint32_t s0 = tid; s0 < S_real; s0 += TILE_THREADS) {
        int k = 0;
        while (s0 >= s_rc[k + 1]) ++k;
        s_idtmp[s_base[k] + (s0 - s_rc[k])] = in.id[s_g0[k] + (s0 - s_rc[k])];
      }
      __syncthreads();
      for (uint32_t s0 = tid; s0 < S_real; s0 += TILE_THREADS) {
        int k = 0;
        while (s0 >= s_rc[k + 1]) ++k;
        const uint32_t j = s_g0[k] + (s0 - s_rc[k]);
        place(k, j, in.cell[j], s_idtmp[s_base[k] + (s0 - s_rc[k])], in.off[j], in.vel[j]);
      }
    }
  }
  PHASE_MARK(4);
  __syncthreads();
  __builtin_amdgcn_s_setprio(0);

  PHASE_MARK(5);
  const uint32_t tile_flags = s_huge;  // (after the barrier that ends the staging)
  const bool tile_huge = XF ? (tile_flags & 1u) != 0u : tile_flags != 0u;
  // the window's agents take the LDS path (block-uniform); XF: not with a staged x beyond the exact range
  bool lds_ok = tiled_ok;
  if constexpr (XF) {
    if (tiled_ok && (tile_flags & 2u) != 0u) {
      lds_ok = false;
      if (tid == 0) atomicAdd(&E.ctr->n_win_off_lds, 1u);
    }
  }
  // ---- one thread = one agent; idle lanes keep the wave-uniform loops going.  A window that
  // holds more than TILE_THREADS agents (dense spots) is walked in chunks. ----
  for (uint32_t chunk = 0; chunk < n_own; chunk += TILE_THREADS) {
  const OwnIn L = chunk == 0 ? first_own : load_own(chunk);
  const bool active = L.active;
  const int R = row0 + L.own_r;
  const uint32_t i = L.i;
  Own o;
  o.gx = (uint32_t)R;
  o.gy = L.cell - (uint32_t)R * g.nx;
  o.off = L.off;
  o.v = L.v;
  o.id = L.id;
  o.slot = i;
  const uint32_t meta = L.meta;
  const GroupDev grp = L.grp;
  uint32_t route_st = L.route;
  o.u = active ? hlp_velocity(grp, E, g, o.id, pref, i, o.gx, o.gy, o.off, route_st) : make_float2(0.0f, 0.0f);
  float wx = o.u.x, wy = o.u.y;  // NoLocalPlan: identity, no_local_plan.rs:9-17
  if (active && grp.lp_kind == 2u && E.lp_vel) {  // a host LocalPlanner has answered for this agent
    wx = E.lp_vel[i].x;
    wy = E.lp_vel[i].y;
  }
  const bool zan = active && grp.lp_kind == 1u && o.off.x == o.off.x && o.off.y == o.off.y;
  // (an eyesight that is NaN or infinite goes down the gather path: the lean filter's radius test is one sign bit, which
  // for a NaN radius would be the NaN's sign; the gather path compares, and a comparison with NaN is false as in the reference)
  const bool sight_ok = fabsf(grp.eyesight) < f_inf();

  // an agent whose offset left its cell (clamped below the grid, aliased above it), or whose
  // reach crosses the row stride (where the reference aliases into the next row), needs
  // cells the strip did not stage: exact gather path
  int lx = 1, hx = 0, ly = 1, hy = 0;  // empty by default
  bool use_tile = false;
  if (zan) {
    const float slack = 0.01f * g.cs;
    const bool regular = o.off.x >= -slack && o.off.x <= g.cs + slack && o.off.y >= -slack &&
                         o.off.y <= g.cs + slack;
    if (lds_ok && regular && sight_ok) {
      // get_bounds relative to the own cell (cell_bounds with g = 0), in 32-bit integers: the same
      // floors, saturated at +-1e9 cells instead of +-4e9 (an eyesight of any size only matters up
      // to the h cells the tile reaches)
      const float e = grp.eyesight, ics = g.inv_cs;
      const int blx = (int)fminf(fmaxf(floorf((o.off.x - e) * ics - CS_BOUNDS_EPS), -1e9f), 1e9f);
      const int bhx = (int)fminf(fmaxf(floorf((o.off.x + e) * ics + CS_BOUNDS_EPS), -1e9f), 1e9f);
      const int bly = (int)fminf(fmaxf(floorf((o.off.y - e) * ics - CS_BOUNDS_EPS), -1e9f), 1e9f);
      const int bhy = (int)fminf(fmaxf(floorf((o.off.y + e) * ics + CS_BOUNDS_EPS), -1e9f), 1e9f);
      use_tile = (long long)o.gy + bhy < (long long)g.nx;
      // f32 rounding at a cell edge can ask for one cell beyond ceil(r / cell); that cell
      // lies entirely out of reach
      lx = max(blx, -cfg.h);
      hx = min(bhx, cfg.h);
      ly = max(bly, -cfg.h);
      hy = min(bhy, cfg.h);
    }
  }
  if (zan && !use_tile) {
    bool tz;
    gather_agent(P, in, cell_start, o, grp, wx, wy, tz);
    if (tz) atomicAdd(&E.ctr->n_tti_zero, 1u);
  }

  if (lds_ok && !TILE_DEBUG(1u)) {  // block-uniform; lanes without tile work idle through
    const bool mine = zan && use_tile;
    if (!mine) {
      lx = 1; hx = 0; ly = 1; hy = 0;
    }
    const float rs = grp.eyesight * g.fix_scale;
    const float nr2 = -(rs * rs);  // the radius test in fixed units (sight_margin)
    const float Rs = grp.R * g.fix_scale;
    const float R2 = Rs * Rs;  // fixed units too (cs_device_types: UNITS)
    const int own_row = R - r0;
    const int own_col = (int)o.gy - sy0;
    const int2 pi = window_pos(o.off, own_row, own_col);
    // x_j - x_i of a staged x in fixed units.  XF: both are exact floats, one subtraction gives the bits of the integer
    // form's subtraction + conversion (see the template's note); the own x is a staged record's, so within the range.
    const float pix = (float)pi.x;
    auto rel_x = [&](int xj) {
      if constexpr (XF) return __int_as_float(xj) - pix;
      else return (float)(xj - pi.x);
    };
    // own LDS slot, to skip self without touching ids
    uint32_t self_slot = 0xFFFFFFFFu;
    if (mine) {
      if (chunk == 0) {
        self_slot = s_self[tid];  // written by whoever staged this agent
      } else {
        const unsigned short* t = s_tab + own_row * W1 + own_col;
        for (uint32_t j = t[0]; j < t[1]; ++j)
          if (s_id[j] == o.id) self_slot = j;
      }
    }
    entry_t* __restrict__ my_list = s_list + tid;
    const uint32_t CAP = cfg.list_cap;
    const uint32_t CAP_ALL = CAP + cfg.spill_rows;  // LDS rows + spilled rows
    uint32_t* __restrict__ my_spill =
        cfg.spill + ((size_t)lidx * cfg.spill_rows) * TILE_THREADS + tid;  // (lidx: the launch's builder workgroups have no spill area)
    bool spilling = false;  // wave-uniform: some lane of this wave went beyond CAP
    // entry k of this lane's list (k < CAP_ALL): LDS row, or a spilled row (global memory, written by this lane)
    auto entry_at = [&](uint32_t k) -> uint32_t {
      if (k < CAP) return my_list[k * TILE_THREADS];
      return my_spill[(size_t)(k - CAP) * TILE_THREADS];  // (written by this very lane: program order suffices)
    };
    uint32_t cnt = 0, n_back = 0;
    unsigned long long fwd = 0;   // bit k: list entry k has right of way over this agent
    unsigned long long fwd2 = 0;  // the same for entries 64..127 (spilled rows only)
    float T = f_inf();
    bool flushed = false;  // wave-uniform
    bool self_listed = false;  // the lean filter has put the agent itself on its list (it is nobody's neighbour)

    // p_j - p_i of a staged neighbour in fixed units: exact integer difference, one conversion
    auto rel = [&](uint32_t j, float& rpx, float& rpy) {
      const int2 pj = s_pos[j];
      rpx = rel_x(pj.x);
      rpy = (float)(pj.y - pi.y);
    };
    // pass 2 over the first `n` entries of the list: t_i and the right-of-way mask.
    // Two entries per trip (their LDS reads are issued together, one latency covers both); the
    // trip count is the wave's maximum, so the loop is a scalar one: a lane past its own `n`
    // works on stale entries (slot clamped into the tile) and drops the result.
    const uint32_t slot_max = S ? S - 1u : 0u;
    auto run_ttc_impl = [&](uint32_t n, uint32_t k0, auto spill_tag) {  // entries [k0, n), k0 even and wave-uniform
      constexpr bool SPILL = decltype(spill_tag)::value;
      uint32_t m_lo = 0, m_hi = 0, m_2 = 0, m_3 = 0;
      for (uint32_t k = k0; __any(k < n); k += 2) {
        const bool v0 = k < n, v1 = k + 1u < n;
        uint32_t j0, j1;
        if (!SPILL || k < CAP) {
          j0 = my_list[k * TILE_THREADS];
          j1 = my_list[(k + 1) * TILE_THREADS];
        } else {  // spilled rows (wave-uniform branch: CAP is even)
          j0 = v0 ? entry_at(k) : 0u;
          j1 = v1 ? entry_at(k + 1u) : 0u;
        }
        j0 = min(j0, slot_max);
        j1 = min(j1, slot_max);
        const int2 pj0 = s_pos[j0], pj1 = s_pos[j1];
        const float2 vj0 = s_vel[j0], vj1 = s_vel[j1];
        const uint32_t id0 = s_id[j0], id1 = s_id[j1];
        const float rpx0 = rel_x(pj0.x), rpy0 = (float)(pj0.y - pi.y);
        const float rpx1 = rel_x(pj1.x), rpy1 = (float)(pj1.y - pi.y);
        const float rvx0 = vj0.x - o.v.x, rvy0 = vj0.y - o.v.y, rvx1 = vj1.x - o.v.x, rvy1 = vj1.y - o.v.y;
        const float d20 = __builtin_fmaf(rpx0, rpx0, rpy0 * rpy0), d21 = __builtin_fmaf(rpx1, rpx1, rpy1 * rpy1);
        float t0, t1;
        // overlapping pairs take the guarded form (ttc_pair_f32); they are rare, so the test is one
        // wave-uniform branch per pair of entries
        if (tile_huge || __any(min(ttc_overlap_key(d20), ttc_overlap_key(d21)) < __float_as_uint(R2))) {
          t0 = ttc_pair_f32(rvx0, rvy0, rpx0, rpy0, d20, R2);
          t1 = ttc_pair_f32(rvx1, rvy1, rpx1, rpy1, d21, R2);
        } else {
          t0 = ttc_core_f32(rvx0, rvy0, rpx0, rpy0, d20, R2);
          t1 = ttc_core_f32(rvx1, rvy1, rpx1, rpy1, d21, R2);
        }
        t0 = v0 ? t0 : f_inf();
        t1 = v1 ? t1 : f_inf();
        T = fminf(T, fminf(t0, t1));  // a time to collision is never NaN (ttc_core_f32)
        const bool f0 = v0 && id0 > o.id, f1 = v1 && id1 > o.id;
        // k is wave-uniform and even: the pair lands in one 32-bit half of the mask
        if (k < 32u) m_lo |= (f0 ? (1u << k) : 0u) | (f1 ? (2u << k) : 0u);
        else if (!SPILL || k < 64u) m_hi |= (f0 ? (1u << (k - 32u)) : 0u) | (f1 ? (2u << (k - 32u)) : 0u);
        else if (k < 96u) m_2 |= (f0 ? (1u << (k - 64u)) : 0u) | (f1 ? (2u << (k - 64u)) : 0u);
        else m_3 |= (f0 ? (1u << (k - 96u)) : 0u) | (f1 ? (2u << (k - 96u)) : 0u);
      }
      const unsigned long long m = ((unsigned long long)m_hi << 32) | m_lo;
      const unsigned long long mm = SPILL ? (((unsigned long long)m_3 << 32) | m_2) : 0ull;
      // neighbours without right of way: only their number matters (and only when t_i = 0)
      n_back += (n > k0 ? n - k0 : 0u) - (uint32_t)__popcll(m) - (uint32_t)__popcll(mm);
      if (!k0) fwd = 0ull;
      fwd |= m;
      fwd2 = mm;
    };
    // The same pass for a wave whose lists lie entirely in their LDS rows (n <= CAP: the usual case), with fewer
    // instructions per entry.  The kernel's time is its instruction count (every instruction of a wave, vector or
    // scalar, costs the SIMD ~2.2 clocks at four waves, conversions / compares / selects / three-operand integer
    // forms 4.4, v_sqrt / v_rcp 8.3: tools/valu_ceiling.hip, DESIGN.md section 4), so:
    //  * a trip is switched off per lane by EXEC (one compare per pair of entries) instead of masking each
    //    entry's result; an odd list repeats its last entry first (a minimum does not mind, and the repeated
    //    right-of-way bit is cut off below), so no entry is clamped or selected;
    //  * the right-of-way bit of an entry is the sign of (own id - neighbour's id) (ids < 2^31), shifted in with
    //    one v_alignbit: no compare / select / or;
    //  * overlapping pairs (the only ones that need the guarded quadratic, ttc_pair_f32) are only looked for
    //    (one v_min3 per pair of entries over the overlap keys); a wave that saw one repeats the pass in the
    //    guarded form.
    //  * the tail of the quadratic (v_sqrt, v_rcp, two multiply-subtracts, the selects of ttc_select: more than half an
    //    entry's cost) is only run for the entries whose result can be finite.  The pass over all entries stops at the
    //    discriminant and shifts one more sign bit per entry into a second pair of words: set when ttc_core_c_f32
    //    returns +inf whatever its root and reciprocal come out as (ttc_skip_key: disc < 0, or disc == 0 with bh == 0;
    //    same velocities, or a miss by more than R, which is most of any list).  A second loop pops the other entries'
    //    bits one 32-bit word at a time, as forward_terms_vanish does, reads each such entry again and runs the parent
    //    expressions on the same operands, so the bits are those of the one-pass form; the minimum does not mind
    //    the order (T is never NaN).  Re-reading an entry costs three times what its tail costs in the one-pass loop
    //    (35 VALU against 12), and the second loop's trip count is the wave's LARGEST number of entries left, so the split
    //    pays only below ~0.45 entries left per trip of the first pass (profiles/K4_LEVERS.md: walk 0.21, random 0.44,
    //    creep 0.67), which is only known once the first pass has been paid for.  The form is therefore chosen per
    //    wave BEFORE the pass, by what makes entries drop out in numbers: a wave all of whose agents walk at exactly
    //    their preferred velocity (nobody pushed them in the last step: a crowd in free flow, whose groups share a
    //    velocity to the bit, rv == 0) takes the split form, every other wave the one-pass loop.  Either form gives
    //    the same bits, so the choice is one of speed alone.  (Only the pass over a complete list has the split form:
    //    the two calls that drain a full list in mid-filter are rare and keep the one-pass loop, a third of the code.)
    auto run_ttc_lds = [&](uint32_t n, auto may_split_tag) {
      constexpr bool MAY_SPLIT = decltype(may_split_tag)::value;
      if (n & 1u) my_list[n * TILE_THREADS] = my_list[(n - 1u) * TILE_THREADS];  // (row n <= CAP: the spare row at most)
      const float T_in = T;
      const bool split = MAY_SPLIT && !wave_any(n != 0u && (o.v.x != o.u.x || o.v.y != o.u.y));  // (a NaN velocity: one-pass)
      uint32_t w0 = 0u, w1 = 0u;
      uint32_t l0 = 0u, l1 = 0u;    // split form, per entry: 1 = its time to collision is +inf, no need to finish it
      uint32_t kmin = 0xFFFFFFFFu;  // smallest overlap key of the pairs: < bits(R2) = some pair overlaps
      auto pass = [&](auto form_tag) {
        constexpr int FORM = decltype(form_tag)::value;  // 0: the whole quadratic, 1: guarded, 2: up to the discriminant
        constexpr bool GUARDED = FORM == 1;
        const entry_t* __restrict__ lp = my_list;
        // bottom-tested loops (scalar loop control costs issue time: see the filter), one word of right-of-way
        // bits per 32 entries (k is wave-uniform)
        for (uint32_t kb = 0; kb < 64u; kb += 32u) {
        uint32_t word = 0u, lword = 0u, k = kb;
        const uint32_t k_end = min(n, kb + 32u);  // (one per-lane bound, so that the loop's exit is ONE vector test)
        bool v = k < k_end;
        if (wave_any(v)) do {
          if (v) {
            const uint32_t j0 = lp[0], j1 = lp[TILE_THREADS];
            lp += 2 * TILE_THREADS;
            const int2 pj0 = s_pos[j0], pj1 = s_pos[j1];
            const float2 vj0 = s_vel[j0], vj1 = s_vel[j1];
            const uint32_t id0 = s_id[j0], id1 = s_id[j1];
            const float rpx0 = rel_x(pj0.x), rpy0 = (float)(pj0.y - pi.y);
            const float rpx1 = rel_x(pj1.x), rpy1 = (float)(pj1.y - pi.y);
            const float rvx0 = vj0.x - o.v.x, rvy0 = vj0.y - o.v.y, rvx1 = vj1.x - o.v.x, rvy1 = vj1.y - o.v.y;
            const float d20 = __builtin_fmaf(rpx0, rpx0, rpy0 * rpy0), d21 = __builtin_fmaf(rpx1, rpx1, rpy1 * rpy1);
            if (GUARDED) {
              const float t0 = ttc_pair_f32(rvx0, rvy0, rpx0, rpy0, d20, R2);
              const float t1 = ttc_pair_f32(rvx1, rvy1, rpx1, rpy1, d21, R2);
              T = fminf(T, fminf(t0, t1));  // a time to collision is never NaN (ttc_select)
            } else {
              kmin = min(kmin, min(ttc_overlap_key(d20), ttc_overlap_key(d21)));
              if (FORM == 0) {
                const float t0 = ttc_core_f32(rvx0, rvy0, rpx0, rpy0, d20, R2);
                const float t1 = ttc_core_f32(rvx1, rvy1, rpx1, rpy1, d21, R2);
                T = fminf(T, fminf(t0, t1));
              } else {  // (leaves T alone)
                lword = __builtin_amdgcn_alignbit(lword, ttc_skip_key(rvx0, rvy0, rpx0, rpy0, d20 - R2), 31);
                lword = __builtin_amdgcn_alignbit(lword, ttc_skip_key(rvx1, rvy1, rpx1, rpy1, d21 - R2), 31);
              }
              word = __builtin_amdgcn_alignbit(word, o.id - id0, 31);
              word = __builtin_amdgcn_alignbit(word, o.id - id1, 31);
            }
          }
          k += 2u;
          v = k < k_end;
        } while (wave_any(v));
        if (!GUARDED) {  // (as selects: written as branches the words end up in scratch memory)
          w0 = (kb == 0u) ? word : w0;
          w1 = (kb == 0u) ? w1 : word;
          if (FORM == 2) {
            l0 = (kb == 0u) ? lword : l0;
            l1 = (kb == 0u) ? l1 : lword;
          }
        }
        if (!wave_any(kb + 32u < n)) break;
        }
      };
      if constexpr (MAY_SPLIT) {
        if (split) pass(std::integral_constant<int, 2>{});
        else pass(std::integral_constant<int, 0>{});
      } else {
        pass(std::integral_constant<int, 0>{});
      }
#ifdef CS_TILE_TRIPS
      if ((tid & 63u) == 0u && split) atomicAdd(&E.ctr->dbg[19], 1u);
      if ((tid & 63u) == 0u && wave_any(kmin < __float_as_uint(R2))) atomicAdd(&E.ctr->dbg[8], 1u);
#endif
      // entry k's bit is now bit (entries shifted in - 1 - k) of its word: to bit k (k < 32) / bit k - 32, and
      // only the first n entries count
      const uint32_t n2 = (n + 1u) & ~1u;
      const uint32_t b0 = min(n2, 32u), b1 = n2 > 32u ? n2 - 32u : 0u;
      const unsigned long long valid = n >= 64u ? ~0ull : ((1ull << n) - 1ull);
      if (wave_any(kmin < __float_as_uint(R2)) || tile_huge) {  // (rare) some pair overlaps, or somebody in the tile
                                                                // has been thrown: every entry, in the guarded form
        T = T_in;
        pass(std::integral_constant<int, 1>{});
      } else if (split) {
        if constexpr (MAY_SPLIT) {
          // the entries that are left: list row k of the word's 32, read again
          auto finish = [&](uint32_t w, uint32_t row0) {
            const entry_t* __restrict__ lp = my_list + row0 * TILE_THREADS;
            while (w) {
              const uint32_t k = (uint32_t)__builtin_ctz(w);
              w &= w - 1u;
              const uint32_t j = lp[k * TILE_THREADS];
              const float2 vj = s_vel[j];
              float rpx, rpy;
              rel(j, rpx, rpy);
              const float d2 = __builtin_fmaf(rpx, rpx, rpy * rpy);
              T = fminf(T, ttc_core_f32(vj.x - o.v.x, vj.y - o.v.y, rpx, rpy, d2, R2));
            }
          };
          const uint32_t live_lo = ~__builtin_bitreverse32(l0 << ((32u - b0) & 31u)) & (uint32_t)valid;
          const uint32_t live_hi = ~__builtin_bitreverse32(l1 << ((32u - b1) & 31u)) & (uint32_t)(valid >> 32);
#ifdef CS_TILE_TRIPS
          {
            const uint32_t pc = (uint32_t)__popc(live_lo) + (uint32_t)__popc(live_hi);
            uint32_t t = 0;
            while (wave_any(t < pc)) ++t;
            uint32_t sum = pc;
            for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
            if ((tid & 63u) == 0u) {
              atomicAdd(&E.ctr->dbg[17], t);
              atomicAdd(&E.ctr->dbg[18], sum);
            }
          }
#endif
          finish(live_lo, 0u);
          if (wave_any(live_hi != 0u)) finish(live_hi, 32u);
        }
      }
      uint32_t m_lo = b0 ? __builtin_bitreverse32(w0 << ((32u - b0) & 31u)) : 0u;
      uint32_t m_hi = b1 ? __builtin_bitreverse32(w1 << ((32u - b1) & 31u)) : 0u;
      const unsigned long long m = ((((unsigned long long)m_hi) << 32) | m_lo) & valid;
      // neighbours without right of way: only their number matters (and only when t_i = 0)
      n_back += n - (uint32_t)__popcll(m);
      fwd = m;
      fwd2 = 0ull;
    };
    // a wave that never went beyond the LDS rows runs the lean form alone; one that did, the lean form over
    // the LDS rows and the general one over the few spilled entries behind them
    auto run_ttc = [&](uint32_t n, auto may_split_tag) {
#ifdef CS_TILE_TRIPS
      {
        uint32_t t = 0;
        while (wave_any(2u * t < n)) ++t;
        uint32_t sum = n;
        for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
        if ((tid & 63u) == 0u) {
          atomicAdd(&E.ctr->dbg[4], t);
          atomicAdd(&E.ctr->dbg[7], sum);
        }
      }
#endif
      if (TILE_DEBUG(32u)) {
        if (!spilling) run_ttc_impl(n, 0u, std::false_type{});
        else run_ttc_impl(n, 0u, std::true_type{});
      } else {
        run_ttc_lds(min(n, CAP), may_split_tag);
        if (spilling && wave_any(n > CAP)) run_ttc_impl(n, CAP, std::true_type{});
      }
    };
    // pass 3: forces of the listed neighbours selected by `mask`, in list order
    float fx = 0.0f, fy = 0.0f;
    ForceCtx fc;
    auto run_force_impl = [&](unsigned long long mask, unsigned long long mask2, auto spill_tag) {
      constexpr bool SPILL = decltype(spill_tag)::value;
      while (mask) {
        const int k = __ffsll((long long)mask) - 1;
        mask &= mask - 1ull;
        float rpx, rpy;
        rel(SPILL ? entry_at((uint32_t)k) : (uint32_t)my_list[k * TILE_THREADS], rpx, rpy);
        const float d2 = __builtin_fmaf(rpx, rpx, rpy * rpy);
        zanlungo_forward_force(rpx, rpy, d2, fc, fx, fy);
      }
      if (SPILL)
        while (mask2) {  // entries 64..127: spilled rows
          const int k = __ffsll((long long)mask2) - 1;
          mask2 &= mask2 - 1ull;
          float rpx, rpy;
          rel(entry_at(64u + (uint32_t)k), rpx, rpy);
          const float d2 = __builtin_fmaf(rpx, rpx, rpy * rpy);
          zanlungo_forward_force(rpx, rpy, d2, fc, fx, fy);
        }
    };
    auto run_force = [&](unsigned long long mask, unsigned long long mask2) {
#ifdef CS_TILE_TRIPS
      {
        const uint32_t pc = (uint32_t)__popcll(mask) + (uint32_t)__popcll(mask2);
        uint32_t t = 0;
        while (wave_any(t < pc)) ++t;
        uint32_t sum = pc;
        for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
        if ((tid & 63u) == 0u) {
          atomicAdd(&E.ctr->dbg[3], t);
          atomicAdd(&E.ctr->dbg[6], sum);
        }
      }
#endif
      if (!spilling) {
        run_force_impl(mask, 0ull, std::false_type{});
      } else {  // list order = the entries in LDS first, then the spilled ones
        const unsigned long long in_lds = CAP >= 64u ? ~0ull : ((1ull << CAP) - 1ull);
        run_force_impl(mask & in_lds, 0ull, std::false_type{});
        if (wave_any(((mask & ~in_lds) | mask2) != 0ull)) run_force_impl(mask & ~in_lds, mask2, std::true_type{});
      }
    };
    // The check of a lane that passed the force pre-test (zanlungo_forward_vanishes): true when none of the entries of
    // `mask` (LDS rows only) has the NaN direction.  Each term's exp2 is then +0, so the term leaves fx, fy at +0.  The
    // s is bit for bit the one of zanlungo_forward_force: there s = |fma(px, dy, -(py dx))| with (px, py) = +-(rpy, -rpx).
    // Unflipped that is |fma(rpy, dy, c)| with c = rpx dx rounded (-((-rpx) dx) = c: negations are exact); flipped it is
    // |fma(-rpy, dy, -c)| = |-fma(rpy, dy, c)| (negating a factor and the addend negates the exact result, and rounding
    // to nearest is symmetric).  No sqrt, rsq or exp here: that is the saving.  A forward entry at the agent's own
    // position (rp = 0) has s = 0 (or NaN) and fails.
    // `s > 0` fails for +-0 and NaN: exactly when (bits(s) << 1) - 1 exceeds 0xFEFFFFFF (+-inf passes, as there), kept
    // as a running maximum in a register.  s is never a denormal: rpx, rpy are integers; for rpx != 0, dx = futx - rpx is 0
    // or at least 2^-24 in magnitude (near an integer of magnitude >= 1 a float is a multiple of 2^-24), so rpx dx and its
    // rounding are 0 or multiples of 2^-47; for rpx == 0 that term is 0 (or NaN for an infinite dx).  The same holds for
    // rpy dy, so a non-zero finite s is at least 2^-47, and the bit test agrees with the comparison in any denormal mode.
    // The mask is walked one 32-bit word at a time (a 64-bit lowest-bit search and clear cost 7 VALU per entry, a 32-bit
    // one 3); entries 32..63 are the few beyond the first word.  (Two entries per trip, and a lane mask for the result,
    // measured slower: more scalar instructions per entry.)
    auto forward_terms_vanish = [&](unsigned long long mask) {
      uint32_t worst = 0u;
      auto word = [&](uint32_t w, uint32_t row0) {
        const entry_t* __restrict__ lp = my_list + row0 * TILE_THREADS;
        while (w) {
          const uint32_t k = (uint32_t)__builtin_ctz(w);
          w &= w - 1u;
          float rpx, rpy;
          rel((uint32_t)lp[k * TILE_THREADS], rpx, rpy);
          const float s = __builtin_fmaf(rpy, fc.futy - rpy, rpx * (fc.futx - rpx));
          worst = max(worst, (__float_as_uint(s) << 1) - 1u);
        }
      };
      word((uint32_t)mask, 0u);
      word((uint32_t)(mask >> 32), 32u);
      return worst <= 0xFEFFFFFFu;
    };
    // masks of the first c list entries
    auto run_force_first = [&](uint32_t c) {
      const unsigned long long lo = c >= 64u ? ~0ull : ((1ull << c) - 1ull);
      const unsigned long long hi = c <= 64u ? 0ull : (c >= 128u ? ~0ull : ((1ull << (c - 64u)) - 1ull));
      run_force(lo, hi);
    };
    // pass 1: the filter.  FORCE = false collects every neighbour in sight, FORCE = true only
    // those with a larger id (used when the list had to be recycled).
    auto sweep = [&](bool FORCE) {
      for (int dx = -cfg.h; dx <= cfg.h; ++dx) {
        const int rr = own_row + dx;  // staged row index (per lane: lanes own different rows)
        // the cells [own_col + ly, own_col + hy] of staged row rr are ONE run of slots
        uint32_t j0 = 0, e = 0;
        if (dx >= lx && dx <= hx && rr >= 0 && rr < nr) {
          const int c_lo = max(own_col + ly, 0), c_hi = min(own_col + hy, W1 - 2);
          if (c_lo <= c_hi) {
            j0 = s_tab[rr * W1 + c_lo];
            e = s_tab[rr * W1 + c_hi + 1];
          }
        }
        if (TILE_DEBUG(16u)) j0 = e;
        const uint32_t n_run = e - j0;
        // candidate index relative to the run, starting on an even SLOT: k = -1 is the slot
        // before the run (another cell's member, or the previous row's pad) and fails `k < n_run`
        // as an unsigned number like every index past the end
        const uint32_t k_first = 0u - (j0 & 1u);
        {
          // Fast form: no capacity test inside the loop and a wave-uniform number of trips.
          // Appends beyond the LDS rows go to a spare row.  If some lane did run over, the wave
          // switches (for good) to the form that also writes the appends beyond CAP to the
          // lane's spilled rows in global memory, and redoes the run.  Only a lane beyond
          // CAP_ALL sends the wave to the careful loop below.
          const uint32_t cnt0 = cnt;
          bool fits;
          if (!FORCE && !TILE_DEBUG(32u)) {
            // The usual case in its leanest form (the kernel's time is its instruction count, DESIGN.md section 4):
            //  * no range test per candidate: a lane past its run reads the invisible pair behind the tile (one
            //    compare and one select per PAIR, shared with the loop's exit test); the slot before and the slot
            //    after a run belong to cells out of reach and cannot pass the radius test (CS_BOUNDS_EPS);
            //  * an accepted candidate advances the list cursor, an LDS address, by one row through the sign bit
            //    of the radius test (v_lshrrev, v_and, v_add: full-rate instructions; no compare / select / count);
            //  * the agent itself is not filtered out: its time to collision with itself is +inf (0 * inf = NaN fails
            //    every comparison), its id is not larger than its own, so neither t_i nor the forces see it; the
            //    count of neighbours without right of way is corrected once (self_listed).
            // A wave that has gone beyond the LDS rows (SPILL) runs the same loop with one more compare per pair:
            // "did a lane accept a candidate whose entry lies beyond CAP"; only then (a few trips per wave) the
            // entries concerned go to the lane's spilled rows.
            const uint32_t lbase = lds_addr(my_list), row_bytes = TILE_THREADS * (uint32_t)sizeof(entry_t);
            const uint32_t lim = lbase + CAP * row_bytes;
            const uint32_t far = lds_addr(s_pos + S);
            auto lean_run = [&](auto spill_tag) {
              constexpr bool SPILL = decltype(spill_tag)::value;
              const uint32_t span = cfg.spill_rows * row_bytes;
              uint32_t lp = lbase + cnt * row_bytes;
              uint32_t spilled_to = max(lp, lim);  // the cursor up to which this lane's spilled rows are written
              uint32_t ja = j0 & ~1u;
              uint32_t src = lds_addr(s_pos + ja);
              // (a bottom-tested loop: the compiler turns `for (;;) { if (!any) break; ... }` into six scalar
              // instructions of loop control per trip, this form into one; scalar instructions cost issue time too:
              // 131.5 -> 127.5 us)
              bool v = ja < e;
              if (wave_any(v)) do {
#ifdef CS_TILE_TRIPS
                if ((tid & 63u) == 0u) atomicAdd(&E.ctr->dbg[5], 1u);
#endif
                const int4 pp = lds_ld_i4(v ? src : far);  // two candidates: slots ja and ja + 1
                const float ax = rel_x(pp.x), ay = (float)(pp.y - pi.y);
                const float bx = rel_x(pp.z), by = (float)(pp.w - pi.y);
                const float sa = sight_margin(ax, ay, nr2), sb = sight_margin(bx, by, nr2);
                // branch-free append: a rejected entry is overwritten by the next store
                const uint32_t la = lp;
                lds_st_u16(min(lp, lim), ja);
                lp += (__float_as_uint(sa) >> 22) & row_bytes;
                const uint32_t lb = lp;
                lds_st_u16(min(lp, lim), ja + 1u);
                lp += (__float_as_uint(sb) >> 22) & row_bytes;
                if (SPILL) {
                  const bool late = lp > spilled_to;  // accepted an entry at or beyond row CAP
                  if (wave_any(late)) {
                    if (late) {
                      // (entry c of the list, c >= CAP, is word (c - CAP) * TILE_THREADS of the lane's spill column)
                      if (lb != la && la >= lim && la - lim < span) my_spill[(la - lim) / sizeof(entry_t)] = ja;
                      if (lp != lb && lb >= lim && lb - lim < span) my_spill[(lb - lim) / sizeof(entry_t)] = ja + 1u;
                      spilled_to = lp;
                    }
                  }
                }
                ja += 2u;
                src += 2u * (uint32_t)sizeof(int2);
                v = ja < e;
              } while (wave_any(v));
              cnt = (lp - lbase) / row_bytes;
            };
            fits = true;
            if (!spilling) {
              lean_run(std::false_type{});
              if (dx == 0) self_listed = mine && nr2 < 0.0f;
              if (!wave_any(cnt > CAP)) continue;
              if (cfg.spill_rows) {  // the wave switches (for good) to the form with spilled rows and redoes the run
                spilling = true;
                cnt = cnt0;
              } else {
                fits = false;
              }
            }
            if (spilling) {
              lean_run(std::true_type{});
              if (dx == 0) self_listed = mine && nr2 < 0.0f;
              fits = !wave_any(cnt > CAP_ALL);
            }
            if (!fits && dx == 0) self_listed = false;  // (the run is done again below, where the agent is left out)
          } else if (!spilling) {
            // only the own row's run can hold the agent itself: the others skip that test
            auto pairs = [&](auto centre_tag) {
              constexpr bool CENTRE = decltype(centre_tag)::value;
              uint32_t k = k_first;
              const int4* __restrict__ src = reinterpret_cast<const int4*>(s_pos + (j0 & ~1u));
              while (__any((int)k < (int)n_run)) {
                const int4 pp = *src;  // two candidates: slots j0 + k and j0 + k + 1
                const float ax = rel_x(pp.x), ay = (float)(pp.y - pi.y);
                const float bx = rel_x(pp.z), by = (float)(pp.w - pi.y);
                bool ta = sight_margin(ax, ay, nr2) < 0.0f && k < n_run;
                bool tb = sight_margin(bx, by, nr2) < 0.0f && k + 1u < n_run;
                const uint32_t ja = j0 + k;
                if (CENTRE) {
                  ta = ta && ja != self_slot;
                  tb = tb && ja + 1u != self_slot;
                }
                if (FORCE) {
                  if (ta) ta = s_id[ja] > o.id;
                  if (tb) tb = s_id[ja + 1u] > o.id;
                }
                // branch-free append: a rejected entry is overwritten by the next store
                my_list[min(cnt, CAP) * TILE_THREADS] = (entry_t)ja;
                cnt += ta ? 1u : 0u;
                my_list[min(cnt, CAP) * TILE_THREADS] = (entry_t)(ja + 1u);
                cnt += tb ? 1u : 0u;
                k += 2u;
                src += 1;
              }
            };
            if (dx == 0) pairs(std::true_type{});
            else pairs(std::false_type{});
            if (!__any(cnt > CAP)) continue;
            fits = false;
            if (cfg.spill_rows) {
              spilling = true;
              cnt = cnt0;
            }
          }
          if (spilling && (FORCE || TILE_DEBUG(32u))) {
            uint32_t k = k_first;
            const int4* __restrict__ src = reinterpret_cast<const int4*>(s_pos + (j0 & ~1u));
            while (__any((int)k < (int)n_run)) {
              const int4 pp = *src;
              const float ax = rel_x(pp.x), ay = (float)(pp.y - pi.y);
              const float bx = rel_x(pp.z), by = (float)(pp.w - pi.y);
              const uint32_t ja = j0 + k;
              bool ta = sight_margin(ax, ay, nr2) < 0.0f && ja != self_slot && k < n_run;
              bool tb = sight_margin(bx, by, nr2) < 0.0f && ja + 1u != self_slot && k + 1u < n_run;
              if (FORCE) {
                if (ta) ta = s_id[ja] > o.id;
                if (tb) tb = s_id[ja + 1u] > o.id;
              }
              my_list[min(cnt, CAP) * TILE_THREADS] = (entry_t)ja;
              if (ta && cnt >= CAP && cnt < CAP_ALL) my_spill[(size_t)(cnt - CAP) * TILE_THREADS] = ja;
              cnt += ta ? 1u : 0u;
              my_list[min(cnt, CAP) * TILE_THREADS] = (entry_t)(ja + 1u);
              if (tb && cnt >= CAP && cnt < CAP_ALL) my_spill[(size_t)(cnt - CAP) * TILE_THREADS] = ja + 1u;
              cnt += tb ? 1u : 0u;
              k += 2u;
              src += 1;
            }
            fits = !__any(cnt > CAP_ALL);
          }
          if (fits) continue;
          // some lane holds more than the list and its spilled rows can take: drain what has
          // been collected up to this run, then walk the run with the careful loop
          cnt = cnt0;
          if (__any(cnt > CAP)) {
            if (FORCE) {
              run_force_first(cnt);
            } else {
              run_ttc(cnt, std::false_type{});
              flushed = true;
            }
            cnt = 0;
          }
        }
        uint32_t j = j0;
        while (__any(j < e)) {
          while (j < e && cnt < CAP) {
            const int2 pj = s_pos[j];
            const float ax = rel_x(pj.x), ay = (float)(pj.y - pi.y);
            bool take = sight_margin(ax, ay, nr2) < 0.0f && j != self_slot;  // strict `<`, location_hash_2d.rs:251
            if (FORCE && take) take = s_id[j] > o.id;
            if (take) {
              my_list[cnt * TILE_THREADS] = (entry_t)j;
              ++cnt;
            }
            ++j;
          }
          if (__any(cnt >= CAP)) {  // some lane is full: everyone drains
            if (FORCE) {
              run_force_first(cnt);
            } else {
              run_ttc(cnt, std::false_type{});
              flushed = true;
            }
            cnt = 0;
          }
        }
      }
    };

    PHASE_MARK(6);
    sweep(false);
    PHASE_MARK(7);
#ifdef CS_TILE_TRIPS
    if ((tid & 63u) == 0u) {
      atomicAdd(&E.ctr->dbg[0], 1u);
      if (spilling) atomicAdd(&E.ctr->dbg[1], 1u);
      if (flushed) atomicAdd(&E.ctr->dbg[2], 1u);
    }
#endif
    if (TILE_DEBUG(8u)) cnt = 0;
    run_ttc(cnt, std::true_type{});
    PHASE_MARK(8);
    if (self_listed) n_back -= 1u;
    const bool tz = (T == 0.0f);
#ifdef CS_TILE_TRIPS
    {  // agents of this wave on the LDS path, and those with a finite time to collision (whose force pass runs)
      const uint32_t n_mine = (uint32_t)__popcll(__ballot(mine)), n_finite = (uint32_t)__popcll(__ballot(mine && T != f_inf()));
      if ((tid & 63u) == 0u) {
        atomicAdd(&E.ctr->dbg[9], n_mine);
        atomicAdd(&E.ctr->dbg[10], n_finite);
      }
    }
#endif
    if (mine && T != f_inf()) fc = make_force_ctx(o.v.x, o.v.y, T, grp, g);
    else fc = ForceCtx{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // Forces that provably vanish: an agent whose collision horizon lies far away (|v| t_i beyond its sight by more than
    // the exp2 underflow distance, zanlungo_forward_vanishes) has exactly +0 in every forward term.  Such a lane checks
    // its entries for the NaN direction only (forward_terms_vanish) and then passes mask 0 to the full loop: a wave of
    // such lanes skips it, one with a lane whose check failed runs it for that lane.  Its fx, fy stay +0, the bits the full
    // loop produces: there scale = (mag * (+0)) * inv_n = +-0 (mag finite, inv_n = rsq(d2) finite and > 0 for d2 >= 1),
    // and fma(px, +-0, +0) = +0 for a finite px (px * +-0 is exact; +-0 + +0 = +0), term after term from fx = fy = +0.
    // Lanes that fail the pre-test or the check run the unchanged loop, so every NaN comes from there, with its bits.
    // (The spilled-row form, the drained lists of `flushed` and every ablation (TILE_DEBUG) keep the full loop for every
    // lane, so that ablation timings still compare with the recorded ones.)
    const bool vanish = mine && T != f_inf() && zanlungo_forward_vanishes(fc, T, grp.vanish2);
#ifdef CS_TILE_TRIPS
    {  // the pre-test: lanes that pass, waves in which every lane with a finite t_i passes, their forward entries
      const unsigned long long finite = __ballot(mine && T != f_inf()), pass = __ballot(vanish);
      const uint32_t all = (mine && T != f_inf()) ? (uint32_t)__popcll(fwd) + (uint32_t)__popcll(fwd2) : 0u;
      uint32_t ent = vanish ? all : 0u, ent_all = all;
      for (int d = 32; d; d >>= 1) {
        ent += __shfl_xor(ent, d);
        ent_all += __shfl_xor(ent_all, d);
      }
      if ((tid & 63u) == 0u) {
        atomicAdd(&E.ctr->dbg[11], (uint32_t)__popcll(pass));
        if (finite != 0ull && (finite & ~pass) == 0ull) atomicAdd(&E.ctr->dbg[12], 1u);
        atomicAdd(&E.ctr->dbg[13], ent);
        atomicAdd(&E.ctr->dbg[16], ent_all);
      }
    }
#endif
    // lanes with t_i = inf take no force (zanlungo.rs:211)
    if (TILE_DEBUG(64u)) {
    } else if (!__any(flushed)) {
      unsigned long long m = (T != f_inf()) ? fwd : 0ull;
      // Only a wave in which every lane with forward entries is a candidate takes the check.  Elsewhere the loop's trip
      // count stays some other lane's, and the check would only add to it (the creep scene, where 0.75 % of the lanes
      // pass, ran its step kernel 5 % slower with the check in every wave that had a candidate).
      const unsigned long long work = __builtin_amdgcn_ballot_w64(m != 0ull);
      if (!TILE_DEBUG(~0u) && !spilling && work != 0ull && (work & ~__builtin_amdgcn_ballot_w64(vanish)) == 0ull) {
        if (m != 0ull && forward_terms_vanish(m)) m = 0ull;
#ifdef CS_TILE_TRIPS
        {  // lanes that took the fast path, waves whose full loop it emptied
          const unsigned long long fast = __ballot(vanish && m == 0ull);
          if ((tid & 63u) == 0u) {
            atomicAdd(&E.ctr->dbg[14], (uint32_t)__popcll(fast));
            if (!wave_any(m != 0ull)) atomicAdd(&E.ctr->dbg[15], 1u);
          }
        }
#endif
      }
      run_force(m, (T != f_inf()) ? fwd2 : 0ull);
    } else {
      cnt = 0;
      if (T == f_inf()) {
        lx = 1; hx = 0;  // nothing to collect
      }
      sweep(true);
      run_force_first(cnt);
    }
    if (mine) {
      if (T != f_inf()) {
        // Neighbours with a smaller id have weight 0: their term is (d/|d|) * 0 = 0, except
        // with t_i == 0, where 0 * A * |dv| / 0 = NaN (zanlungo.rs:163; SURVEY.md KAT-Z3).
        if (tz && n_back > 0) {
          fx = f_nan();
          fy = f_nan();
        }
      } else {
        fx = 0.0f;
        fy = 0.0f;
      }
      wx = __builtin_fmaf(fx, grp.inv_mass, o.u.x);  // recommended + force * (1/m), zanlungo.rs:216
      wy = __builtin_fmaf(fy, grp.inv_mass, o.u.y);
      if (tz) atomicAdd(&E.ctr->n_tti_zero, 1u);
    }
    PHASE_MARK(9);
  }
  if (active && !TILE_DEBUG(4u)) step_epilogue(P, E, Ep, i, o.gx, o.gy, o.off, o.id, meta, grp, wx, wy, route_st, late_check);
  PHASE_MARK(10);
  }  // chunk
  BORDER_DONE();
  PHASE_END();
}
#undef BORDER_DONE

// CS_CFG_TILE_OVERLAP, "early exchange": one wave on the second stream, in front of the next step's halo exchange, waits
// until the border windows of the step kernel's launch `seq` have all finished (Counters::border_flag, published by the
// last of them with everything it packed released at agent scope).  Bounded: giving up poisons the engine.
__global__ void k_wait_border(Counters* __restrict__ ctr, uint32_t seq) {
  if (threadIdx.x != 0) return;
  for (uint32_t spins = 0; spins < (1u << 22); ++spins) {
    if (__hip_atomic_load(&ctr->border_flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == seq) return;
    __builtin_amdgcn_s_sleep(16);
  }
  atomicAdd(&ctr->n_early_stalled, 1u);
}
