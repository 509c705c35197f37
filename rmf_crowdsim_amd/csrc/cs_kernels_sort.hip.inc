// cs_kernels_sort.hip.inc — K1 histogram, K2 scan, K3 scatter: the per-step cell re-sort
// Part of the single translation unit crowdstep_hip.hip (included there, in order).

// ---------------------------------------------------------------------------
// K1: histogram + arrival rank (used when the histogram kept by k_step is stale)
// ---------------------------------------------------------------------------
__global__ void k_count(AgentArrays a, uint32_t first, uint32_t n, uint32_t* __restrict__ cell_count,
                        const Counters* __restrict__ ctr, uint32_t tile) {
  uint32_t i = first + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (tile && i >= ctr->n_pending)) return;
  uint32_t c = a.cell[i];
  if (c == CS_INVALID_CELL) return;
  a.rank[i] = atomicAdd(&cell_count[c], 1u);
}

__global__ void k_mark_sources(GridDev g, AgentArrays a, uint32_t n, const SinkDev* __restrict__ sinks,
                               const uint32_t* __restrict__ src_cell_start,
                               const uint32_t* __restrict__ src_sorted,
                               uint32_t* __restrict__ src_occupied, const Counters* __restrict__ ctr) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (g.tile && i >= ctr->n_pending)) return;
  uint32_t c = a.cell[i];
  if (c == CS_INVALID_CELL) return;
  float2 o = a.off[i];
  mark_sources(g, sinks, src_cell_start, src_sorted, src_occupied, c, o.x, o.y);
}

// Tile engines: append agents whose ids were assigned across tiles (cs_spawn_commit).
struct SpawnRecord {
  float ox, oy;
  uint32_t id, cell, meta, route;  // route: the agent_cache entry of a route follower (0 = none)
};
__global__ void k_append_spawns(AgentArrays a, uint32_t slot_cap, const SpawnRecord* __restrict__ rec,
                                uint32_t n, uint32_t* __restrict__ cell_count, Counters* __restrict__ ctr) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SpawnRecord r = rec[i];
  const uint32_t slot = atomicAdd(&ctr->n_pending, 1u);
  if (slot >= slot_cap) {
    atomicAdd(&ctr->n_halo_overflow, 1u);
    return;
  }
  a.off[slot] = make_float2(r.ox, r.oy);
  a.vel[slot] = make_float2(0.0f, 0.0f);
  a.id[slot] = r.id;
  a.cell[slot] = r.cell;
  a.meta[slot] = r.meta;
  if (a.route) a.route[slot] = r.route;
  a.rank[slot] = atomicAdd(&cell_count[r.cell], 1u);
}

// ---------------------------------------------------------------------------
// K2: exclusive scan of cell_count -> cell_start (and zero cell_count)
//   pass A: per-block totals; pass B: one workgroup turns the totals into block offsets
//   (an exclusive scan, in place); pass C: an in-block scan from the block's offset.  1024 cells per block.
// ---------------------------------------------------------------------------
#define SCAN_BLOCK 256
#define SCAN_ITEMS 4
#define SCAN_TILE (SCAN_BLOCK * SCAN_ITEMS)

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_totals(const uint32_t* __restrict__ cell_count,
                                                            uint32_t ncells,
                                                            uint32_t* __restrict__ block_totals) {
  __shared__ uint32_t wsum[SCAN_BLOCK / 64];
  uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  uint32_t s = 0;
  if (base + SCAN_ITEMS <= ncells) {
    uint4 v = *reinterpret_cast<const uint4*>(cell_count + base);
    s = v.x + v.y + v.z + v.w;
  } else {
    for (uint32_t k = 0; k < SCAN_ITEMS; ++k)
      if (base + k < ncells) s += cell_count[base + k];
  }
  for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < SCAN_BLOCK / 64; ++w) t += wsum[w];
    block_totals[blockIdx.x] = t;
  }
}

// Pass B: block_totals -> the offset of every block (exclusive scan, in place), ONE workgroup.  Thread t adds up a run of
// ceil(nblocks / 1024) totals rounded up to whole uint4s, the runs' sums are scanned across the workgroup, and every
// thread writes its run's prefixes.  Linear in the blocks: k_scan_apply used to add up all earlier totals in every
// block, O(blocks^2) loads (~0.5 s a step at the 2.1M blocks of a grid near the 31-bit cell limit).
#define SCAN_BASES_BLOCK 1024
__global__ void __launch_bounds__(SCAN_BASES_BLOCK) k_scan_bases(uint32_t* __restrict__ block_totals, uint32_t nblocks) {
  __shared__ uint32_t wsum[SCAN_BASES_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t run = ((nblocks + SCAN_BASES_BLOCK - 1) / SCAN_BASES_BLOCK + 3u) & ~3u;
  const uint32_t lo = min(threadIdx.x * run, nblocks), hi = min(lo + run, nblocks);  // (lo: a multiple of 4)
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; i += SCAN_ITEMS) {
    if (i + SCAN_ITEMS <= hi) {
      const uint4 q = *reinterpret_cast<const uint4*>(block_totals + i);
      s += q.x + q.y + q.z + q.w;
    } else {
      for (uint32_t k = i; k < hi; ++k) s += block_totals[k];
    }
  }
  const uint32_t incl = wave_incl_scan(s, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t base = incl - s;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  for (uint32_t i = lo; i < hi; i += SCAN_ITEMS) {
    if (i + SCAN_ITEMS <= hi) {
      const uint4 q = *reinterpret_cast<const uint4*>(block_totals + i);
      const uint32_t o1 = base + q.x, o2 = o1 + q.y, o3 = o2 + q.z;
      *reinterpret_cast<uint4*>(block_totals + i) = make_uint4(base, o1, o2, o3);
      base = o3 + q.w;
    } else {
      for (uint32_t k = i; k < hi; ++k) {
        const uint32_t t = block_totals[k];
        block_totals[k] = base;
        base += t;
      }
    }
  }
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_apply(uint32_t* __restrict__ cell_count,
                                                           uint32_t ncells,
                                                           const uint32_t* __restrict__ block_bases,
                                                           uint32_t* __restrict__ cell_start,
                                                           Counters* __restrict__ ctr,
                                                           uint32_t* __restrict__ n_blocks) {
  __shared__ uint32_t wsum[SCAN_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t block_base = block_bases[blockIdx.x];  // (k_scan_bases)

  uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  bool full = base + SCAN_ITEMS <= ncells;
  if (full) {
    uint4 q = *reinterpret_cast<const uint4*>(cell_count + base);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    *reinterpret_cast<uint4*>(cell_count + base) = make_uint4(0, 0, 0, 0);
  } else {
    for (uint32_t k = 0; k < SCAN_ITEMS; ++k) {
      v[k] = (base + k < ncells) ? cell_count[base + k] : 0u;
      if (base + k < ncells) cell_count[base + k] = 0u;
    }
  }
  uint32_t tsum = v[0] + v[1] + v[2] + v[3];
  uint32_t incl = wave_incl_scan(tsum, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t woff = 0;
  for (int w = 0; w < wave; ++w) woff += wsum[w];
  uint32_t excl = block_base + woff + incl - tsum;
  uint32_t o0 = excl, o1 = o0 + v[0], o2 = o1 + v[1], o3 = o2 + v[2];
  if (full) {
    *reinterpret_cast<uint4*>(cell_start + base) = make_uint4(o0, o1, o2, o3);
  } else {
    uint32_t o[4] = {o0, o1, o2, o3};
    for (uint32_t k = 0; k < SCAN_ITEMS; ++k)
      if (base + k < ncells) cell_start[base + k] = o[k];
  }
  // the thread holding the last cell publishes the grand total
  if (base <= ncells - 1 && ncells - 1 < base + SCAN_ITEMS) {
    uint32_t total = o3 + v[3];
    if (!full) {
      total = excl;
      for (uint32_t k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < ncells) total += v[k];
    }
    cell_start[ncells] = total;
    ctr->n_alive = total;
    ctr->n_owned = 0;  // the block builder that follows counts the owned agents
    n_blocks[0] = 0;   // ... and the workgroups of the step kernel (small crowds: of the NEXT step's, cs_engine)
    n_blocks[1] = 0;   //     (its border windows: build_band)
    ctr->n_destroyed = 0;  // the step kernel that follows counts into these
    ctr->n_waypoint_hits = 0;
    ctr->n_tti_zero = 0;
    ctr->n_nonfinite = 0;
    ctr->n_clamped = 0;
    ctr->n_wp_events = 0;
  }
}

// K2 in ONE launch: every workgroup scans its tile of 1,024 cells, publishes the tile's total, and adds up the totals of
// the tiles before it as they appear (a "decoupled look-back" without the chain: every tile publishes its total as soon
// as it has it, a tile waits for ALL its predecessors side by side, one per thread).  A total travels as ONE 64-bit
// word (the launch's sequence number | the sum): no fence, no reset between launches, a stale word is recognised by its
// number.  Written and read with agent-scope atomics: the eight XCDs' L2s are not coherent with each other.
// Which tile a workgroup scans is NOT its blockIdx: it takes a ticket when it starts (one atomic on a counter that only
// grows: the host passes the count of all earlier launches), so a tile waits only for tiles whose workgroups have
// already started, whatever order the dispatcher starts workgroups in and however few are resident at once (another
// process on the GPU, a launch on the second stream): the forward-progress guarantee of a decoupled look-back (the
// round-4 form waited on smaller blockIdx values, which HIP does not promise to start first).  The spin stays bounded
// as a backstop (a tile that gives up poisons the engine: Counters::n_scan_stalled).  Saves the second launch of the
// two-kernel form (~4.5 us of latency per step, at every crowd size).
#define SCAN_ONEPASS_MAX_BLOCKS 1024u
__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_onepass(uint32_t* __restrict__ cell_count, uint32_t ncells,
                                                             uint32_t* __restrict__ cell_start, Counters* __restrict__ ctr,
                                                             uint32_t* __restrict__ n_blocks,
                                                             unsigned long long* __restrict__ tile_sums, uint32_t seq,
                                                             uint32_t* __restrict__ ticket, uint32_t ticket_base) {
  __shared__ uint32_t wsum[SCAN_BLOCK / 64];
  __shared__ uint32_t psum[SCAN_BLOCK / 64];
  __shared__ uint32_t s_tile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1u) - ticket_base;  // (mod 2^32: the counter may wrap, the difference does not)
  __syncthreads();
  const uint32_t tile = s_tile;
  if (tile >= gridDim.x) {  // (the host's ticket count and the device's have parted: an earlier launch never ran.  The
    if (threadIdx.x == 0) atomicAdd(&ctr->n_scan_stalled, 1u);  //  step's sort is void: say so, touch nothing)
    return;
  }
  const uint32_t base = tile * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  const bool full = base + SCAN_ITEMS <= ncells;
  if (full) {
    const uint4 q = *reinterpret_cast<const uint4*>(cell_count + base);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    *reinterpret_cast<uint4*>(cell_count + base) = make_uint4(0, 0, 0, 0);  // (only this thread ever reads these four)
  } else {
    for (uint32_t k = 0; k < SCAN_ITEMS; ++k) {
      v[k] = (base + k < ncells) ? cell_count[base + k] : 0u;
      if (base + k < ncells) cell_count[base + k] = 0u;
    }
  }
  const uint32_t tsum = v[0] + v[1] + v[2] + v[3];
  const uint32_t incl = wave_incl_scan(tsum, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < SCAN_BLOCK / 64; ++w) t += wsum[w];
    __hip_atomic_store(&tile_sums[tile], ((unsigned long long)seq << 32) | t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the tiles before this one (all of them have started: their tickets are smaller): thread p waits for tile p (p, p + 256, ...)
  uint32_t part = 0;
  bool gave_up = false;
  for (uint32_t p = threadIdx.x; p < tile; p += SCAN_BLOCK) {
    unsigned long long w = 0;
    uint32_t spins = 0;
    do {
      w = __hip_atomic_load(&tile_sums[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((uint32_t)(w >> 32) == seq) break;
      __builtin_amdgcn_s_sleep(1);
    } while (++spins < (1u << 20));  // (~a second)
    if ((uint32_t)(w >> 32) != seq) gave_up = true;
    part += (uint32_t)w;
  }
  if (gave_up) atomicAdd(&ctr->n_scan_stalled, 1u);
  for (int d = 32; d > 0; d >>= 1) part += __shfl_down(part, d, 64);
  if (lane == 0) psum[wave] = part;
  __syncthreads();
  uint32_t block_base = 0;
  for (int w = 0; w < SCAN_BLOCK / 64; ++w) block_base += psum[w];
  uint32_t woff = 0;
  for (int w = 0; w < wave; ++w) woff += wsum[w];
  const uint32_t excl = block_base + woff + incl - tsum;
  const uint32_t o0 = excl, o1 = o0 + v[0], o2 = o1 + v[1], o3 = o2 + v[2];
  if (full) {
    *reinterpret_cast<uint4*>(cell_start + base) = make_uint4(o0, o1, o2, o3);
  } else {
    const uint32_t o[4] = {o0, o1, o2, o3};
    for (uint32_t k = 0; k < SCAN_ITEMS; ++k)
      if (base + k < ncells) cell_start[base + k] = o[k];
  }
  // the thread holding the last cell publishes the grand total (what k_scan_apply's does)
  if (base <= ncells - 1 && ncells - 1 < base + SCAN_ITEMS) {
    uint32_t total = o3 + v[3];
    if (!full) {
      total = excl;
      for (uint32_t k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < ncells) total += v[k];
    }
    cell_start[ncells] = total;
    ctr->n_alive = total;
    ctr->n_owned = 0;
    n_blocks[0] = 0;
    n_blocks[1] = 0;
    ctr->n_destroyed = 0;
    ctr->n_waypoint_hits = 0;
    ctr->n_tti_zero = 0;
    ctr->n_nonfinite = 0;
    ctr->n_clamped = 0;
    ctr->n_wp_events = 0;
  }
}

// ---------------------------------------------------------------------------
// K3: scatter records into cell order
// ---------------------------------------------------------------------------
__global__ void k_scatter(AgentArrays src, AgentArrays dst, uint32_t n,
                          const uint32_t* __restrict__ cell_start, const Counters* __restrict__ ctr,
                          uint32_t tile, uint32_t g_ncells) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // the live records land in [0, n_live); the rest of the destination's slots (up to the host's
  // slot count, an upper bound) hold records of an earlier step and must not read "alive"
  if (i >= cell_start[g_ncells]) dst.cell[i] = CS_INVALID_CELL;
  if (tile && i >= ctr->n_pending) return;
  uint32_t c = src.cell[i];
  if (c == CS_INVALID_CELL) return;
  uint32_t d = cell_start[c] + src.rank[i];
  dst.off[d] = src.off[i];
  dst.vel[d] = src.vel[i];
  dst.id[d] = src.id[i];
  dst.cell[d] = c;
  dst.meta[d] = src.meta[i];
  if (src.route) dst.route[d] = src.route[i];
}

// One returning atomic per RUN of lanes with the same cell instead of one per agent.  The step
// kernels' agents come in cell order and few change cell per step, so the lanes of a wave that
// share a cell are nearly always neighbours: a run's first lane reserves as many slots as the run
// is long, rank = base + position in the run.  (Lanes with the same cell that are not neighbours, a
// walker arriving in a cell whose residents sit elsewhere in the wave, are runs of their own: one
// more atomic on that counter.)  Runs are found with one ballot and bit arithmetic; the loop over
// the wave's distinct cells this replaces cost ~80 instructions per wave.
__device__ __forceinline__ uint32_t wave_histogram_rank(uint32_t* __restrict__ cell_count,
                                                        uint32_t cell, bool valid) {
  const int lane = __lane_id();
  const unsigned long long active = __ballot(true);  // lanes that returned earlier take no part
  const uint32_t prev = __shfl_up(cell, 1, 64);
  const bool prev_ok = lane > 0 && ((active >> (lane - 1)) & 1ull) && __shfl_up(valid ? 1 : 0, 1, 64) != 0;
  // a lane starts a run unless it continues its (active, valid) predecessor's; lanes without a
  // cell of their own (valid == false) end the run before them and start none
  const bool head = !(valid && prev_ok && prev == cell);
  const unsigned long long heads = __ballot(head);
  const unsigned long long below = heads & ((2ull << lane) - 1ull);  // (this lane's own run start is among them)
  const int first = 63 - __clzll((long long)below);
  // a run ends before the next head, and before the next lane that is not active
  const unsigned long long stops = lane == 63 ? 0ull : ((heads | ~active) >> (lane + 1));
  const int end = stops ? lane + 1 + (__ffsll((long long)stops) - 1) : 64;
  uint32_t base = 0;
  if (valid && first == lane) base = atomicAdd(&cell_count[cell], (uint32_t)(end - lane));
  base = __shfl(base, first, 64);
  return base + (uint32_t)(lane - first);
}
