// cs_kernels_aux.hip.inc — K7 halo pack/unpack, K6 spawn, radius query
// Part of the single translation unit crowdstep_hip.hip (included there, in order).

// ---------------------------------------------------------------------------
// K7: halo exchange of a tile (DESIGN.md "Tiles").  A record is what a neighbour tile needs
// to see an agent: cell-relative state + its GLOBAL cell.  Ownership is decided by cell
// alone, so migrants and ghosts travel the same way: everything within 2*halo cells of a
// shared edge (the ghost ring itself holds the agents that just walked out) is sent.
// Buffer layout: record 0 is the header (word 0 = record count), records follow.
// ---------------------------------------------------------------------------
// (HaloRecord, halo_append, HaloBuffers8 and halo_pack_agent live in cs_device_types.hip.inc: the step
// kernels pack their border agents themselves.)

// `clear_a` / `clear_b`: send buffers of the OTHER axis, whose record counts are reset here for
// their next pack (their last exchange is complete in stream order), which saves two memsets
// per phase.
__global__ void k_halo_pack(GridDev g, AgentArrays a, uint32_t n_ub, uint32_t axis, uint32_t band,
                            HaloRecord* __restrict__ send_lo, HaloRecord* __restrict__ send_hi,
                            uint32_t cap, Counters* __restrict__ ctr, HaloRecord* __restrict__ clear_a,
                            HaloRecord* __restrict__ clear_b) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    if (clear_a) reinterpret_cast<uint32_t*>(clear_a)[0] = 0u;
    if (clear_b) reinterpret_cast<uint32_t*>(clear_b)[0] = 0u;
  }
  if (i >= n_ub || i >= ctr->n_pending) return;
  const uint32_t c = a.cell[i];
  if (c == CS_INVALID_CELL) return;
  const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
  const uint32_t q = axis == 0 ? cx : cy;
  const uint32_t extent = axis == 0 ? g.ncells / g.nx : g.nx;
  const bool lo = send_lo != nullptr && q < band;
  const bool hi = send_hi != nullptr && q + band >= extent;
  if (!lo && !hi) return;
  HaloRecord r;
  const float2 o = a.off[i], v = a.vel[i];
  r.ox = o.x; r.oy = o.y; r.vx = v.x; r.vy = v.y;
  r.id = a.id[i];
  r.meta = a.meta[i];
  r.gcx = g.org_x + cx;
  r.gcy = g.org_y + cy;
  r.route = a.route ? a.route[i] : 0u;
  r.reserved = 0u;
  if (lo) halo_append(send_lo, cap, r, ctr);
  if (hi) halo_append(send_hi, cap, r, ctr);
}

// Both directions of one axis in one launch: blocks [0, blocks_per_dir) read recv_a, the rest recv_b.
__global__ void k_halo_unpack(GridDev g, AgentArrays a, uint32_t slot_cap,
                              const HaloRecord* __restrict__ recv_a, const HaloRecord* __restrict__ recv_b,
                              uint32_t cap, uint32_t blocks_per_dir, uint32_t* __restrict__ cell_count,
                              Counters* __restrict__ ctr) {
  const bool second = blockIdx.x >= blocks_per_dir;
  const HaloRecord* __restrict__ recv = second ? recv_b : recv_a;
  if (!recv) return;
  const uint32_t n = min(reinterpret_cast<const uint32_t*>(recv)[0], cap);
  uint32_t i = (blockIdx.x - (second ? blocks_per_dir : 0u)) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const HaloRecord r = recv[i + 1];
  const long long lx = (long long)r.gcx - (long long)g.org_x, ly = (long long)r.gcy - (long long)g.org_y;
  const long long n_rows = g.ncells / g.nx;
  if (lx < 0 || ly < 0 || lx >= n_rows || ly >= (long long)g.nx) return;  // not in my ring
  const uint32_t slot = atomicAdd(&ctr->n_pending, 1u);
  if (slot >= slot_cap) {
    atomicAdd(&ctr->n_halo_overflow, 1u);
    return;
  }
  const uint32_t cell = (uint32_t)lx * g.nx + (uint32_t)ly;
  a.off[slot] = make_float2(r.ox, r.oy);
  a.vel[slot] = make_float2(r.vx, r.vy);
  a.id[slot] = r.id;
  a.meta[slot] = r.meta;
  a.cell[slot] = cell;
  a.rank[slot] = atomicAdd(&cell_count[cell], 1u);
  if (a.route) a.route[slot] = r.route;
}

__global__ void k_halo_pack_all(GridDev g, AgentArrays a, uint32_t n_ub, uint32_t band, HaloBuffers8 send,
                                Counters* __restrict__ ctr) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ub || i >= ctr->n_pending) return;
  const uint32_t c = a.cell[i];
  if (c == CS_INVALID_CELL) return;
  if (!halo_in_band(g, band, c)) return;  // (the lanes left append together)
  const float2 o = a.off[i], v = a.vel[i];
  halo_pack_agent(g, band, send, c, o.x, o.y, v.x, v.y, a.id[i], a.meta[i], a.route ? a.route[i] : 0u, ctr);
}

// Blocks [d * blocks_per_dir, (d + 1) * blocks_per_dir) merge receive buffer d.  The transport
// has finished with the send buffers by now (stream order), so their record counts are reset
// here for the next step's pack.
// step_tag (a mesh's steps only, else 0): 1 + the index of the mesh step this unpack belongs to.  The first eight threads
// then also merge the mesh's failure word (Counters::mesh_fail_step): this tile's own error counters as of now, the
// words its neighbours sent, the smallest non-zero value; it goes out with the next exchange.
__global__ void k_halo_unpack_all(GridDev g, AgentArrays a, uint32_t slot_cap, HaloBuffers8 recv,
                                  HaloBuffers8 send, uint32_t blocks_per_dir,
                                  uint32_t* __restrict__ cell_count, Counters* __restrict__ ctr, uint32_t step_tag) {
  if (blockIdx.x == 0 && threadIdx.x < 64) {  // (one whole wave, so that the shuffles below have all their lanes)
    const uint32_t t = threadIdx.x;
    uint32_t word = 0u;
    if (step_tag) {
      if (t < 8 && recv.p[t]) word = reinterpret_cast<const uint32_t*>(recv.p[t])[1];
      if (t == 8) {
        word = ctr->mesh_fail_step;
        if (!word && (ctr->n_out_of_bounds | ctr->n_halo_late | ctr->n_early_stalled | ctr->n_win_dropped | ctr->n_scan_stalled | ctr->n_halo_overflow))
          word = step_tag;
      }
      uint32_t key = word ? word : 0xFFFFFFFFu;  // smallest non-zero
      for (int d = 8; d > 0; d >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, d, 64));
      word = key == 0xFFFFFFFFu ? 0u : key;
      if (t == 0) ctr->mesh_fail_step = word;
    }
    if (t < 8 && send.p[t]) {
      uint32_t* head = reinterpret_cast<uint32_t*>(send.p[t]);
      head[0] = 0u;
      if (step_tag) head[1] = word;
    }
  }
  const uint32_t d = blockIdx.x / blocks_per_dir;
  const HaloRecord* __restrict__ rb = recv.p[d];
  if (!rb) return;
  const uint32_t n = min(reinterpret_cast<const uint32_t*>(rb)[0], recv.cap[d]);
  const uint32_t i = (blockIdx.x - d * blocks_per_dir) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const HaloRecord r = rb[i + 1];
  const long long lx = (long long)r.gcx - (long long)g.org_x, ly = (long long)r.gcy - (long long)g.org_y;
  const long long n_rows = g.ncells / g.nx;
  if (lx < 0 || ly < 0 || lx >= n_rows || ly >= (long long)g.nx) return;  // not in my ring
  const uint32_t slot = atomicAdd(&ctr->n_pending, 1u);
  if (slot >= slot_cap) {
    atomicAdd(&ctr->n_halo_overflow, 1u);
    return;
  }
  const uint32_t cell = (uint32_t)lx * g.nx + (uint32_t)ly;
  a.off[slot] = make_float2(r.ox, r.oy);
  a.vel[slot] = make_float2(r.vx, r.vy);
  a.id[slot] = r.id;
  a.meta[slot] = r.meta;
  a.cell[slot] = cell;
  a.rank[slot] = atomicAdd(&cell_count[cell], 1u);
  if (a.route) a.route[slot] = r.route;
}

// ---------------------------------------------------------------------------
// K6: spawn.  Sinks in ascending handle order.  A sink spawns ONE agent at its source iff its
// generator asked for > 0 and nobody stood within 0.4 of the source at the end of the previous
// step (lib.rs:199-254); ids are sequential in ascending sink order, so the slots need an
// exclusive scan of the spawn flags.  Two launches of SPAWN_BLOCK sinks per workgroup:
// k_spawn_count (flags per block -> block totals, and a copy of the id counter), then
// k_spawn_apply (every block sums the totals before it, rescans its own flags, writes agents).
// ---------------------------------------------------------------------------
#define SPAWN_BLOCK 1024

__device__ __forceinline__ uint32_t spawn_flag(const SinkDev* __restrict__ sinks,
                                               const uint32_t* __restrict__ want,
                                               const uint32_t* __restrict__ src_occupied, uint32_t s,
                                               uint32_t n_sinks) {
  if (s >= n_sinks) return 0u;
  return (want[s] > 0 && src_occupied[s] == 0 && sinks[s].src_cell != CS_INVALID_CELL) ? 1u : 0u;
}

// scratch: [0] = id of the first agent of this step, [1 + b] = spawns of block b
__global__ void __launch_bounds__(SPAWN_BLOCK) k_spawn_count(const SinkDev* __restrict__ sinks,
                                                             const uint32_t* __restrict__ want,
                                                             uint32_t n_sinks,
                                                             const uint32_t* __restrict__ src_occupied,
                                                             const Counters* __restrict__ ctr,
                                                             uint32_t* __restrict__ scratch) {
  __shared__ uint32_t wsum[SPAWN_BLOCK / 64];
  const uint32_t flag = spawn_flag(sinks, want, src_occupied, blockIdx.x * SPAWN_BLOCK + threadIdx.x, n_sinks);
  const unsigned long long m = __ballot(flag != 0u);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < SPAWN_BLOCK / 64; ++w) t += wsum[w];
    scratch[1 + blockIdx.x] = t;
    if (blockIdx.x == 0) scratch[0] = ctr->next_id;
  }
}

__global__ void __launch_bounds__(SPAWN_BLOCK) k_spawn_apply(AgentArrays a, uint32_t n_slots, uint32_t cap,
                                                             const SinkDev* __restrict__ sinks,
                                                             const uint32_t* __restrict__ want,  // per sink slot
                                                             uint32_t n_sinks, uint32_t n_want,
                                                             uint32_t* __restrict__ src_occupied,
                                                             uint32_t* __restrict__ cell_count,
                                                             uint32_t* __restrict__ spawned_slots,
                                                             Counters* __restrict__ ctr,
                                                             const uint32_t* __restrict__ scratch) {
  __shared__ uint32_t wsum[SPAWN_BLOCK / 64];
  __shared__ uint32_t s_base, s_total;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t first_id = scratch[0];
  // spawns of the blocks before this one, and of all blocks
  uint32_t before = 0, all = 0;
  for (uint32_t b = threadIdx.x; b < gridDim.x; b += SPAWN_BLOCK) {
    const uint32_t t = scratch[1 + b];
    all += t;
    if (b < blockIdx.x) before += t;
  }
  for (int d = 32; d > 0; d >>= 1) {
    before += __shfl_down(before, d, 64);
    all += __shfl_down(all, d, 64);
  }
  if (threadIdx.x == 0) {
    s_base = 0;
    s_total = 0;
  }
  __syncthreads();
  if (lane == 0 && (before | all)) {
    atomicAdd(&s_base, before);
    atomicAdd(&s_total, all);
  }
  __syncthreads();
  const uint32_t total = s_total;

  const uint32_t s = blockIdx.x * SPAWN_BLOCK + threadIdx.x;
  const uint32_t flag = spawn_flag(sinks, want, src_occupied, s, n_sinks);
  if (s < n_sinks) src_occupied[s] = 0u;  // read for the last time this step: the step kernel marks anew
  const uint32_t incl = wave_incl_scan(flag, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t woff = 0;
  for (int w = 0; w < wave; ++w) woff += wsum[w];
  const uint32_t excl = s_base + woff + incl - flag;
  if (flag) {
    const uint32_t slot = n_slots + excl;
    if (slot < cap) {
      const SinkDev& sk = sinks[s];
      a.off[slot] = make_float2(sk.src_ox, sk.src_oy);
      a.vel[slot] = make_float2(0.0f, 0.0f);
      a.id[slot] = first_id + excl;
      a.cell[slot] = sk.src_cell;
      a.meta[slot] = sk.group;  // next_waypoint = 0
      a.rank[slot] = atomicAdd(&cell_count[sk.src_cell], 1u);
      spawned_slots[excl] = s;
      // RMFPlanner::set_target for a (source, first waypoint) pair that is already planned:
      // agent_cache.insert(id, (route, 0)), rmf/mod.rs:220-222
      if (a.route) a.route[slot] = sk.spawn_route;
    }
  }
  // the host reserved n_want slots; the ones no sink used must not look alive
  for (uint32_t k = total + blockIdx.x * SPAWN_BLOCK + threadIdx.x; k < n_want; k += gridDim.x * SPAWN_BLOCK)
    if (n_slots + k < cap) a.cell[n_slots + k] = CS_INVALID_CELL;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctr->n_spawned = total;
    ctr->next_id = first_id + total;
  }
}

// Tile engines, Phase A without the host.  Every tile knows every sink; k_spawn_probe_dev says
// which of the sinks this tile OWNS would spawn; the caller ORs the flag vectors of all tiles
// (an all-reduce); k_spawn_commit_dev hands out ids in ascending sink order over the combined
// flags (the same on every tile) and appends the agents of the owned sinks.
__global__ void k_spawn_probe_dev(const SinkDev* __restrict__ sinks, const uint32_t* __restrict__ want,
                                  uint32_t n_sinks, const uint32_t* __restrict__ src_occupied,
                                  int* __restrict__ flags) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n_sinks) flags[s] = (int)spawn_flag(sinks, want, src_occupied, s, n_sinks);
}

__global__ void __launch_bounds__(SPAWN_BLOCK) k_spawn_count_flags(const int* __restrict__ flags, uint32_t n_sinks,
                                                                   Counters* __restrict__ ctr,
                                                                   uint32_t* __restrict__ scratch) {
  __shared__ uint32_t wsum[SPAWN_BLOCK / 64];
  const uint32_t s = blockIdx.x * SPAWN_BLOCK + threadIdx.x;
  const bool flag = s < n_sinks && flags[s] != 0;
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < SPAWN_BLOCK / 64; ++w) t += wsum[w];
    scratch[1 + blockIdx.x] = t;
    if (blockIdx.x == 0) {
      scratch[0] = ctr->next_id;
      ctr->n_spawned = 0;  // the commit kernel counts this tile's own spawns into it
    }
  }
}

__global__ void __launch_bounds__(SPAWN_BLOCK) k_spawn_commit_dev(AgentArrays a, uint32_t slot_cap,
                                                                  const SinkDev* __restrict__ sinks,
                                                                  const int* __restrict__ flags, uint32_t n_sinks,
                                                                  uint32_t* __restrict__ cell_count,
                                                                  Counters* __restrict__ ctr,
                                                                  const uint32_t* __restrict__ scratch) {
  __shared__ uint32_t wsum[SPAWN_BLOCK / 64];
  __shared__ uint32_t s_base, s_total;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t first_id = scratch[0];
  uint32_t before = 0, all = 0;
  for (uint32_t b = threadIdx.x; b < gridDim.x; b += SPAWN_BLOCK) {
    const uint32_t t = scratch[1 + b];
    all += t;
    if (b < blockIdx.x) before += t;
  }
  for (int d = 32; d > 0; d >>= 1) {
    before += __shfl_down(before, d, 64);
    all += __shfl_down(all, d, 64);
  }
  if (threadIdx.x == 0) {
    s_base = 0;
    s_total = 0;
  }
  __syncthreads();
  if (lane == 0 && (before | all)) {
    atomicAdd(&s_base, before);
    atomicAdd(&s_total, all);
  }
  __syncthreads();
  const uint32_t s = blockIdx.x * SPAWN_BLOCK + threadIdx.x;
  const uint32_t flag = (s < n_sinks && flags[s] != 0) ? 1u : 0u;
  const uint32_t incl = wave_incl_scan(flag, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t woff = 0;
  for (int w = 0; w < wave; ++w) woff += wsum[w];
  const uint32_t excl = s_base + woff + incl - flag;
  if (flag) {
    const SinkDev& sk = sinks[s];
    if (sk.src_cell == CS_INVALID_CELL && sk.ghost_cell != CS_INVALID_CELL) {
      // another tile's spawn inside my ring: a ghost for this step (see SinkDev.ghost_cell)
      const uint32_t slot = atomicAdd(&ctr->n_pending, 1u);
      if (slot >= slot_cap) {
        atomicAdd(&ctr->n_halo_overflow, 1u);
      } else {
        a.off[slot] = make_float2(sk.src_ox, sk.src_oy);
        a.vel[slot] = make_float2(0.0f, 0.0f);
        a.id[slot] = first_id + excl;
        a.cell[slot] = sk.ghost_cell;
        a.meta[slot] = sk.group;
        if (a.route) a.route[slot] = sk.spawn_route;
        a.rank[slot] = atomicAdd(&cell_count[sk.ghost_cell], 1u);
      }
    }
    if (sk.src_cell != CS_INVALID_CELL) {  // this tile owns the source
      const uint32_t slot = atomicAdd(&ctr->n_pending, 1u);
      if (slot >= slot_cap) {
        atomicAdd(&ctr->n_halo_overflow, 1u);
      } else {
        a.off[slot] = make_float2(sk.src_ox, sk.src_oy);
        a.vel[slot] = make_float2(0.0f, 0.0f);
        a.id[slot] = first_id + excl;
        a.cell[slot] = sk.src_cell;
        a.meta[slot] = sk.group;  // next_waypoint = 0
        a.rank[slot] = atomicAdd(&cell_count[sk.src_cell], 1u);
        if (a.route) a.route[slot] = sk.spawn_route;
        atomicAdd(&ctr->n_spawned, 1u);
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) ctr->next_id = first_id + s_total;
}

// ---------------------------------------------------------------------------
// radius query against the sorted state (SpatialIndex::get_neighbours_in_radius,
// location_hash_2d.rs:240-258).  One block, cells in x-major / y-minor order;
// used by cs_query_radius (host API), not by the step.
// ---------------------------------------------------------------------------
__global__ void k_query_radius(GridDev g, AgentArrays a, const uint32_t* __restrict__ cell_start,
                               long long lx, long long hx, long long ly, long long hy,
                               uint32_t qcx, uint32_t qcy, float qox, float qoy, float r,
                               uint32_t* __restrict__ out_ids, float* __restrict__ out_d2,
                               uint32_t out_cap, uint32_t* __restrict__ out_count) {
  // serial over cells (order matters), parallel inside a cell is not needed: tiny
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t n = 0;
  for (long long x = lx; x <= hx; ++x) {
    for (long long y = ly; y <= hy; ++y) {
      if (x < 0 || y < 0) continue;
      unsigned long long flat = (unsigned long long)x * g.nx + (unsigned long long)y;
      if (flat >= g.ncells) continue;
      uint32_t b = cell_start[flat], e = cell_start[flat + 1];
      // ascending id inside the cell: selection order over the (small) cell
      uint32_t last = 0;
      bool first = true;
      for (uint32_t k = b; k < e; ++k) {
        uint32_t best = 0xFFFFFFFFu, bj = 0;
        bool found = false;
        for (uint32_t j = b; j < e; ++j) {
          uint32_t idj = a.id[j];
          if ((first || idj > last) && (!found || idj < best)) {
            best = idj;
            bj = j;
            found = true;
          }
        }
        if (!found) break;
        last = best;
        first = false;
        uint32_t cj = a.cell[bj];
        uint32_t ax = cj / g.nx, ay = cj - ax * g.nx;
        float2 oj = a.off[bj];
        float rx = (float)((long long)ax - (long long)qcx) * g.cs + (oj.x - qox);
        float ry = (float)((long long)ay - (long long)qcy) * g.cs + (oj.y - qoy);
        if (sqrtf(rx * rx + ry * ry) < r) {
          if (n < out_cap) {
            out_ids[n] = best;
            out_d2[n] = rx * rx + ry * ry;
          }
          ++n;
        }
      }
    }
  }
  *out_count = n;
}

// ---------------------------------------------------------------------------
// Re-cutting a running mesh (DESIGN.md section 7): every tile exports the agents it owns as halo
// records (the record holds everything: offset, velocity, id, group | waypoint, GLOBAL cell,
// route), takes a new rectangle, and imports from all exports the records it now owns.
// ---------------------------------------------------------------------------
// `owned_only`: the arrays hold ghosts (a halo exchange ran since the last step), told from the held
// agents by their cell; right after a step every live record is an agent this tile holds, also
// the ones that have just walked into the ring (the next exchange hands them over).
__global__ void k_tile_histogram(GridDev g, AgentArrays a, uint32_t n_ub, const Counters* __restrict__ ctr,
                                 uint32_t owned_only, uint32_t* __restrict__ rows, uint32_t* __restrict__ cols) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ub || i >= ctr->n_pending) return;
  const uint32_t c = a.cell[i];
  if (c == CS_INVALID_CELL) return;
  const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
  if (owned_only && (cx < g.own_x0 || cx >= g.own_x1 || cy < g.own_y0 || cy >= g.own_y1)) return;  // a ghost
  atomicAdd(&rows[g.org_x + cx], 1u);
  atomicAdd(&cols[g.org_y + cy], 1u);
}
// The live records in the owned cells of a tile whose arrays hold ghosts: what cs_agent_count reports in that state (the
// host's count is the number of agents the last step moved; the exchange has handed some over since).  One atomic per wave.
__global__ void k_tile_count_owned(GridDev g, AgentArrays a, uint32_t n_ub, const Counters* __restrict__ ctr,
                                   uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool mine = false;
  if (i < n_ub && i < ctr->n_pending) {
    const uint32_t c = a.cell[i];
    if (c != CS_INVALID_CELL) {
      const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
      mine = cx >= g.own_x0 && cx < g.own_x1 && cy >= g.own_y0 && cy < g.own_y1;
    }
  }
  const unsigned long long m = __ballot(mine);
  if (m && __lane_id() == __ffsll((long long)m) - 1) atomicAdd(count, (uint32_t)__popcll(m));
}
__global__ void k_tile_export(GridDev g, AgentArrays a, uint32_t n_ub, const Counters* __restrict__ ctr,
                              uint32_t owned_only, HaloRecord* __restrict__ out, uint32_t cap,
                              uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ub || i >= ctr->n_pending) return;
  const uint32_t c = a.cell[i];
  if (c == CS_INVALID_CELL) return;
  const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
  if (owned_only && (cx < g.own_x0 || cx >= g.own_x1 || cy < g.own_y0 || cy >= g.own_y1)) return;  // ghosts stay behind
  const uint32_t k = atomicAdd(count, 1u);
  if (k >= cap) return;
  HaloRecord r;
  const float2 o = a.off[i], v = a.vel[i];
  r.ox = o.x; r.oy = o.y; r.vx = v.x; r.vy = v.y;
  r.id = a.id[i];
  r.meta = a.meta[i];
  r.gcx = g.org_x + cx;
  r.gcy = g.org_y + cy;
  r.route = a.route ? a.route[i] : 0u;
  r.reserved = 0u;
  out[k] = r;
}
__global__ void k_tile_import(GridDev g, AgentArrays a, uint32_t slot_cap, const HaloRecord* __restrict__ rec,
                              uint32_t n, uint32_t* __restrict__ cell_count, Counters* __restrict__ ctr,
                              uint32_t* __restrict__ kept) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const HaloRecord r = rec[i];
  const long long lx = (long long)r.gcx - (long long)g.org_x, ly = (long long)r.gcy - (long long)g.org_y;
  if (lx < (long long)g.own_x0 || lx >= (long long)g.own_x1 || ly < (long long)g.own_y0 || ly >= (long long)g.own_y1)
    return;  // another tile owns it now
  const uint32_t slot = atomicAdd(&ctr->n_pending, 1u);
  if (slot >= slot_cap) {
    atomicAdd(&ctr->n_halo_overflow, 1u);
    return;
  }
  const uint32_t cell = (uint32_t)lx * g.nx + (uint32_t)ly;
  a.off[slot] = make_float2(r.ox, r.oy);
  a.vel[slot] = make_float2(r.vx, r.vy);
  a.id[slot] = r.id;
  a.meta[slot] = r.meta;
  a.cell[slot] = cell;
  if (a.route) a.route[slot] = r.route;
  a.rank[slot] = atomicAdd(&cell_count[cell], 1u);
  atomicAdd(kept, 1u);
}

// Batch form: one wave per query, queries side by side.  Cells in the reference's order (x-major,
// y-minor); inside a cell the members in sight are emitted in ascending id by repeated wave-wide
// minimum (cells hold a handful of agents).  Same arithmetic as k_query_radius.  On a tile engine
// only the agents the tile HOLDS are reported (every agent is held by exactly one tile, so the
// union over the tiles of a mesh is the exact answer); out_cell = GLOBAL cell (x * global stride + y).
struct QueryDev {
  long long lx, hx, ly, hy;
  uint32_t qcx, qcy;
  float qox, qoy, r;
  uint32_t pad;
};
__global__ void __launch_bounds__(64) k_query_radius_batch(GridDev g, AgentArrays a,
                                                           const uint32_t* __restrict__ cell_start,
                                                           const QueryDev* __restrict__ queries, uint32_t n_queries,
                                                           uint32_t global_stride, uint32_t owned_only,
                                                           uint32_t* __restrict__ out_ids,
                                                           float* __restrict__ out_d2, uint32_t* __restrict__ out_cell,
                                                           uint32_t cap, uint32_t* __restrict__ out_count) {
  const uint32_t q = blockIdx.x;
  if (q >= n_queries) return;
  const QueryDev Q = queries[q];
  const int lane = threadIdx.x;
  uint32_t n = 0;
  for (long long x = Q.lx; x <= Q.hx; ++x) {
    for (long long y = Q.ly; y <= Q.hy; ++y) {
      if (x < 0 || y < 0) continue;
      const unsigned long long flat = (unsigned long long)x * g.nx + (unsigned long long)y;
      if (flat >= g.ncells) continue;
      const uint32_t b = cell_start[flat], e = cell_start[flat + 1];
      uint32_t last = 0;
      bool first = true;
      for (;;) {
        // this lane's best candidate: the smallest id beyond `last` among the members in sight
        uint32_t best = 0xFFFFFFFFu, bcell = 0;
        float bd2 = 0.0f;
        for (uint32_t j = b + (uint32_t)lane; j < e; j += 64u) {
          const uint32_t idj = a.id[j];
          if (!(first || idj > last) || idj >= best) continue;
          const uint32_t cj = a.cell[j];
          const uint32_t ax = cj / g.nx, ay = cj - ax * g.nx;
          if (owned_only && (ax < g.own_x0 || ax >= g.own_x1 || ay < g.own_y0 || ay >= g.own_y1)) continue;  // a ghost
          const float2 oj = a.off[j];
          const float rx = (float)((long long)ax - (long long)Q.qcx) * g.cs + (oj.x - Q.qox);
          const float ry = (float)((long long)ay - (long long)Q.qcy) * g.cs + (oj.y - Q.qoy);
          if (sqrtf(rx * rx + ry * ry) < Q.r) {
            best = idj;
            bd2 = rx * rx + ry * ry;
            bcell = (g.org_x + ax) * global_stride + (g.org_y + ay);
          }
        }
        for (int d = 32; d > 0; d >>= 1) {  // wave-wide minimum id, carrying its distance and cell
          const uint32_t ob = __shfl_xor(best, d, 64), oc = __shfl_xor(bcell, d, 64);
          const float od = __shfl_xor(bd2, d, 64);
          if (ob < best) {
            best = ob;
            bd2 = od;
            bcell = oc;
          }
        }
        if (best == 0xFFFFFFFFu) break;
        if (lane == 0 && n < cap) {
          out_ids[(size_t)q * cap + n] = best;
          if (out_d2) out_d2[(size_t)q * cap + n] = bd2;
          if (out_cell) out_cell[(size_t)q * cap + n] = bcell;
        }
        ++n;
        last = best;
        first = false;
      }
    }
  }
  if (lane == 0) out_count[q] = n;
}

// CS_HLP_ROUTE: write the agent_cache entries the host decided on (rmf/mod.rs:221,229)
// pairs: (slot in the current agent arrays, entry)
__global__ void k_route_assign(uint32_t* __restrict__ route, uint32_t n_slots, const uint2* __restrict__ pairs,
                               uint32_t n) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n && pairs[k].x < n_slots) route[pairs[k].x] = pairs[k].y;
}

// Streaming agents view: live agents of the current state, global f64 positions, compacted in
// no particular order (one atomic per wave).
__global__ void k_snapshot(GridDev g, AgentArrays a, uint32_t n, double off_x, double off_y, double cell_size,
                           cs_snapshot_record* __restrict__ out, uint32_t cap, uint32_t* __restrict__ count,
                           const uint64_t* __restrict__ ext_tab, uint32_t n_tab, uint32_t dev_base, uint64_t ext_base) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t cell = i < n ? a.cell[i] : CS_INVALID_CELL;
  const bool live = cell != CS_INVALID_CELL;
  const unsigned long long m = __ballot(live);
  if (!m) return;
  const int lane = __lane_id();
  uint32_t base = 0;
  if (lane == __ffsll((long long)m) - 1) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = __shfl(base, __ffsll((long long)m) - 1, 64);
  if (!live) return;
  const uint32_t k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (k >= cap) return;
  const uint32_t cx = cell / g.nx, cy = cell - cx * g.nx;
  const float2 o = a.off[i], v = a.vel[i];
  cs_snapshot_record r;
  r.x = off_x + ((double)(g.org_x + cx) * cell_size + (double)o.x);
  r.y = off_y + ((double)(g.org_y + cy) * cell_size + (double)o.y);
  r.vx = v.x;
  r.vy = v.y;
  r.id = (uint32_t)ext_id_dev(a.id[i], ext_tab, n_tab, dev_base, ext_base);  // CS_CFG_WIDE_IDS: the low 32 bits
  r.next_waypoint = meta_waypoint(g, a.meta[i]);
  out[k] = r;
}

// ---------------------------------------------------------------------------
// Simulation::remove_agents (lib.rs:176-192): find the slot that holds agent `id` and mark it
// dead, on the device (the host used to download the whole state to find one id).
// meta from (group | waypoint << from_bits) to (group | waypoint << to_bits): cs_engine::widen_groups
__global__ void k_repack_meta(uint32_t* __restrict__ meta, uint32_t n, uint32_t from_bits, uint32_t to_bits) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = meta[i];
  meta[i] = (m & ((1u << from_bits) - 1u)) | ((m >> from_bits) << to_bits);
}

// found[0] = slot (or 0xFFFFFFFF), found[1] = its meta word.  `owned_only`: a tile whose arrays hold ghosts removes only
// an agent in its owned cells (the rule of k_write_match): the ghost copy of a neighbour's agent is nobody here.
// ---------------------------------------------------------------------------
__global__ void k_remove_by_id(GridDev g, AgentArrays a, uint32_t n_ub, const Counters* __restrict__ ctr, uint32_t tile,
                               uint32_t owned_only, uint32_t id, uint32_t* __restrict__ found) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ub || (tile && i >= ctr->n_pending)) return;
  const uint32_t c = a.cell[i];
  if (c == CS_INVALID_CELL || a.id[i] != id) return;
  if (owned_only) {
    const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
    if (cx < g.own_x0 || cx >= g.own_x1 || cy < g.own_y0 || cy >= g.own_y1) return;  // a ghost
  }
  found[0] = i;
  found[1] = a.meta[i];
  a.cell[i] = CS_INVALID_CELL;
}
