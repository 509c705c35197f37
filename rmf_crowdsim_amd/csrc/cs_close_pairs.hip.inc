// cs_close_pairs.hip.inc — the pairs of agents within a distance of one another, between steps: contacts, near misses,
// overlaps (include/crowdstep_state.h, "Pairs of agents between steps").  Part of the single translation unit
// crowdstep_hip.hip (included there, after cs_field.hip.inc; it uses sel_load / sel_pred / sel_begin of
// cs_select.hip.inc and k_ids_scan of cs_kernels_ids.hip.inc, none of which it changes).
//
//   K_pairs_count  k_pairs_count, one lane per slot of the CELL-SORTED arrays (the call sorts first, as the spatial
//                  queries do), so the lanes of a wave stand in the same or in adjacent cells and walk nearly the same
//                  slots at the same time.  A lane rebuilds its own f64 position (the expression of
//                  cs_engine::to_global, through sel_load) and its two role bits (sel_pred) once, then walks the cell
//                  rectangle of `reach` cells each way, row by row: the cells (row, y_lo .. y_hi) of one row are ONE
//                  run of slots, cell_start[row * nx + y_lo] .. cell_start[row * nx + y_hi + 1], so the walk is a loop
//                  over slots, however many of them one cell holds.  For every candidate with a LARGER device id (each
//                  unordered pair is judged once, by its smaller id) it evaluates dx * dx + dy * dy < distance^2 in f64.
//   candidates     are RECOMPUTED FROM THEIR COLUMNS (cell, off, id: 16 bytes), not staged in LDS: the lanes of a
//                  workgroup are slots in cell order, their rectangles overlap but differ (a workgroup would have to
//                  stage the union of them, several times what one lane reads, and index into it per lane), the reach
//                  and the occupancy of a cell are the caller's, so no fixed LDS budget fits, and the reads of
//                  neighbouring lanes hit the same cache lines anyway.  What costs more than the test, the
//                  candidate's own rectangle test and its role bits (meta, group table, velocity, two selections), is
//                  evaluated only for candidates that passed the distance test.
//   no pre-reject  there is no f32 pre-reject: every decision is the f64 expression itself.
//   tally          a lane counts its own hits (its walk is its own, so there is no ballot to take per candidate); the
//                  counts are summed over the wave by shuffles, over the workgroup in LDS, and leave with ONE 64-bit
//                  atomic per workgroup.
//   K_pairs_emit   k_pairs_emit, only when listing: the same walk twice, first to count, then, at the place the
//                  workgroup took with one atomic (a prefix sum over its lanes), to write (a << 32 | b, d2).
//   sort           LSD radix over 4-bit digits of the 64-bit key with the f64 payload, k_pairs_hist / k_ids_scan /
//                  k_pairs_scatter; the digits above the bits of the largest listed id are zero in both halves of the key
//                  and their passes are skipped.  Ascending device id is ascending external id, so the host maps
//                  min(count, cap) pairs and does nothing else per pair.
//   mesh           k_pairs_band exports (id, x, y, role bits, tile) of the participants within reach of an edge that has
//                  a neighbour tile; k_pairs_cross_count / _emit test a tile's band against the gathered records of the
//                  tiles with a higher index, LDS-tiled over the foreign records, the same f64 expression.
//
// WHY THE WALK IS CONSERVATIVE.  Only participants can be in a pair: agents whose reported position is finite and inside
// the grid's own rectangle.  The agents whose stored offset does not lie in the cell they are indexed under are the ones
// clamped into row or column 0 from below the low edge (reported below gx0 / gy0), the ones aliased beyond the row
// stride (reported at or above gy1) and the ones with a NaN position: none of them takes part.  For a participant the
// offset lies in [0, cell_size] of its cell (up to one rounding), so two participants closer than `distance` along an axis
// stand in cells at most distance / cell_size + 1 apart along it; the walk reaches ceil(distance / cell_size) + 1.
//
// Scratch: the count needs 256 bytes of the by-id scratch.  The pair arrays (two key arrays, two payload arrays, the
// digit histogram) live in cs_engine::pairs_scratch while they need at most PAIRS_SCRATCH_KEEP bytes (16 MiB: kept and
// counted by cs_device_bytes); a larger need is allocated for the call and freed before it returns.

#define PAIRS_BLOCK 256u
#define PAIRS_WAVES (PAIRS_BLOCK / 64u)
#define PAIRS_SCRATCH_KEEP ((size_t)16u << 20)

struct PairsArgs {
  double gx0, gx1, gy0, gy1;      // the grid's own rectangle: gx0 <= x < gx1 && gy0 <= y < gy1 takes part
  double dist2;                   // distance * distance
  double off_x, off_y, cell_size;
  uint32_t reach;                 // cells walked each way
  uint32_t owned_only;            // a tile whose arrays hold ghosts: owned agents only
  uint32_t n_groups;
  uint32_t roles;                 // bit 0: sel_a given, bit 1: sel_b given (not given: everyone)
  uint32_t want_vel;              // a given selection has a speed term
  uint32_t pad;
  cs_selection a, b;
};

// a band record of the mesh: a participant near a cut
struct PairsBandRec {
  double x, y;
  uint32_t id;
  uint32_t bits;  // 1: role A, 2: role B, tile index << 2
};
static_assert(sizeof(PairsBandRec) == 24, "band records travel as three 8-byte words");

__device__ __forceinline__ bool pairs_in_grid(const PairsArgs& P, double x, double y) {
  return P.gx0 <= x && x < P.gx1 && P.gy0 <= y && y < P.gy1;  // (a NaN or an infinity is outside)
}

// what a lane knows of its own agent
struct PairsSelf {
  double x, y;
  uint32_t id, cx, cy;
  bool ra, rb;
};

// Slot i as a party to pairs; false: no live (owned) agent, not a participant, or of neither role.
__device__ __forceinline__ bool pairs_self(const GridDev& g, const AgentArrays& a, uint32_t i, uint32_t limit,
                                           const SelGroupDev* __restrict__ groups, const PairsArgs& P, PairsSelf* s) {
  SelAgent ag;
  if (!sel_load(g, a, i, limit, P.owned_only, groups, P.n_groups, P.off_x, P.off_y, P.cell_size, P.want_vel != 0u, &ag))
    return false;
  if (!pairs_in_grid(P, ag.x, ag.y)) return false;
  s->ra = !(P.roles & 1u) || sel_pred(P.a, ag.x, ag.y, ag.vx, ag.vy, ag.wp, ag.g.sink, ag.g.hlp, ag.g.lp);
  s->rb = !(P.roles & 2u) || sel_pred(P.b, ag.x, ag.y, ag.vx, ag.vy, ag.wp, ag.g.sink, ag.g.hlp, ag.g.lp);
  if (!(s->ra || s->rb)) return false;
  const uint32_t c = a.cell[i];
  s->cx = c / g.nx;
  s->cy = c - s->cx * g.nx;
  s->x = ag.x;
  s->y = ag.y;
  s->id = a.id[i];
  return true;
}

// The walk of one lane: the pairs (s, q) with id_q > id_s.  EMIT: written from keys[at] on (below cap), and *top raised
// to the largest id written.  Returns their number.
template <bool EMIT>
__device__ __forceinline__ uint32_t pairs_walk(const GridDev& g, const AgentArrays& a, uint32_t limit,
                                               const uint32_t* __restrict__ cell_start,
                                               const SelGroupDev* __restrict__ groups, const PairsArgs& P,
                                               const PairsSelf& s, unsigned long long at, unsigned long long cap,
                                               unsigned long long* __restrict__ keys, double* __restrict__ d2s,
                                               uint32_t* top) {
  // the rectangle of cells, clipped to the (owned) grid: rows are x, g.ny of them; columns are y, g.nx of them
  const long long lo_x = P.owned_only ? g.own_x0 : 0u, hi_x = P.owned_only ? g.own_x1 : g.ny;
  const long long lo_y = P.owned_only ? g.own_y0 : 0u, hi_y = P.owned_only ? g.own_y1 : g.nx;
  const long long R = P.reach;
  const long long xl = max((long long)s.cx - R, lo_x), xh = min((long long)s.cx + R, hi_x - 1);
  const long long yl = max((long long)s.cy - R, lo_y), yh = min((long long)s.cy + R, hi_y - 1);
  uint32_t n = 0;
  if (yl > yh) return 0u;
  for (long long xr = xl; xr <= xh; ++xr) {
    const uint32_t rowbase = (uint32_t)xr * g.nx;  // (below ncells, which fits 32 bits)
    const uint32_t b = cell_start[rowbase + (uint32_t)yl];
    const uint32_t e = min(cell_start[rowbase + (uint32_t)yh + 1u], limit);  // (index <= ncells: the table has ncells + 1)
    const double bx = (double)((uint64_t)g.org_x + (uint64_t)xr) * P.cell_size;
    for (uint32_t j = b; j < e; ++j) {
      const uint32_t idj = a.id[j];
      if (idj <= s.id) continue;
      const uint32_t cyj = a.cell[j] - rowbase;
      if (cyj > (uint32_t)yh) continue;  // (a slot that is not of this row's run: cannot happen in sorted arrays)
      const float2 off = a.off[j];
      const double xq = P.off_x + (bx + (double)off.x);
      const double yq = P.off_y + ((double)((uint64_t)g.org_y + cyj) * P.cell_size + (double)off.y);
      const double dx = s.x - xq, dy = s.y - yq;
      const double d2 = dx * dx + dy * dy;
      if (!(d2 < P.dist2)) continue;
      if (!pairs_in_grid(P, xq, yq)) continue;
      if (P.roles) {
        const uint32_t meta = a.meta[j];
        const uint32_t grp = meta_group(g, meta);
        if (grp >= P.n_groups) continue;
        const SelGroupDev gq = groups[grp];
        const uint32_t wp = meta_waypoint(g, meta);
        double vx = 0.0, vy = 0.0;
        if (P.want_vel) {
          const float2 v = a.vel[j];
          vx = (double)v.x;
          vy = (double)v.y;
        }
        const bool qa = !(P.roles & 1u) || sel_pred(P.a, xq, yq, vx, vy, wp, gq.sink, gq.hlp, gq.lp);
        const bool qb = !(P.roles & 2u) || sel_pred(P.b, xq, yq, vx, vy, wp, gq.sink, gq.hlp, gq.lp);
        if (!((s.ra && qb) || (qa && s.rb))) continue;
      }
      if (EMIT) {
        if (at + n < cap) {
          keys[at + n] = ((unsigned long long)s.id << 32) | idj;
          if (d2s) d2s[at + n] = d2;
        }
        *top = max(*top, idj);
      }
      ++n;
    }
  }
  return n;
}

__device__ __forceinline__ unsigned long long pairs_wave_sum(unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// the workgroup's hits into *total with one 64-bit atomic (every lane of the workgroup calls this)
__device__ __forceinline__ void pairs_block_tally(uint32_t n, unsigned long long* __restrict__ total) {
  __shared__ unsigned long long s_sum[PAIRS_WAVES];
  const unsigned long long w = pairs_wave_sum(n);
  if (__lane_id() == 0u) s_sum[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0u) {
    unsigned long long t = 0;
    for (uint32_t k = 0; k < PAIRS_WAVES; ++k) t += s_sum[k];
    if (t) atomicAdd(total, t);
  }
}

// where this lane's n entries go: the workgroup takes its place at *cursor with one atomic (every lane calls this).
// The workgroup's total is below 2^32: a listing holds at most CS_PAIRS_MAX pairs.
__device__ __forceinline__ unsigned long long pairs_block_place(uint32_t n, unsigned long long* __restrict__ cursor) {
  __shared__ unsigned long long s_base[PAIRS_WAVES];
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
  uint32_t incl = n;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane >= (uint32_t)d) incl += o;
  }
  if (lane == 63u) s_base[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0u) {
    unsigned long long t = 0;
    for (uint32_t k = 0; k < PAIRS_WAVES; ++k) {
      const unsigned long long c = s_base[k];
      s_base[k] = t;
      t += c;
    }
    const unsigned long long base = t ? atomicAdd(cursor, t) : 0ull;
    for (uint32_t k = 0; k < PAIRS_WAVES; ++k) s_base[k] += base;
  }
  __syncthreads();
  return s_base[wave] + (incl - n);
}

// the largest id the workgroup wrote into *top_out with one atomic (every lane calls this)
__device__ __forceinline__ void pairs_block_top(uint32_t top, uint32_t* __restrict__ top_out) {
  __shared__ uint32_t s_top[PAIRS_WAVES];
  for (int d = 32; d >= 1; d >>= 1) top = max(top, (uint32_t)__shfl_xor(top, d, 64));
  if (__lane_id() == 0u) s_top[threadIdx.x >> 6] = top;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t t = 0;
    for (uint32_t k = 0; k < PAIRS_WAVES; ++k) t = max(t, s_top[k]);
    if (t) atomicMax(top_out, t);
  }
}

// K_pairs_count.  hdr[0] += the pairs (starts at 0).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_pairs_count(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                  const SelGroupDev* __restrict__ groups, PairsArgs P, unsigned long long* __restrict__ hdr) {
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);  // the sorted arrays hold the live agents in front
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  PairsSelf s;
  uint32_t n = 0;
  if (pairs_self(g, a, i, limit, groups, P, &s))
    n = pairs_walk<false>(g, a, limit, cell_start, groups, P, s, 0ull, 0ull, nullptr, nullptr, nullptr);
  pairs_block_tally(n, &hdr[0]);
}

// K_pairs_emit.  hdr[1]: the cursor of the list (starts at 0), the low word of hdr[2]: the largest id listed.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_pairs_emit(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                 const SelGroupDev* __restrict__ groups, PairsArgs P, unsigned long long* __restrict__ hdr,
                 unsigned long long* __restrict__ keys, double* __restrict__ d2s, unsigned long long cap) {
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  PairsSelf s;
  const bool live = pairs_self(g, a, i, limit, groups, P, &s);
  uint32_t n = 0;
  if (live) n = pairs_walk<false>(g, a, limit, cell_start, groups, P, s, 0ull, 0ull, nullptr, nullptr, nullptr);
  const unsigned long long at = pairs_block_place(n, &hdr[1]);
  uint32_t top = 0;
  if (live && n) pairs_walk<true>(g, a, limit, cell_start, groups, P, s, at, cap, keys, d2s, &top);
  pairs_block_top(top, reinterpret_cast<uint32_t*>(&hdr[2]));
}

// The band of a tile: the participants (of a role) whose cell lies within `reach` cells of an owned edge behind which
// another tile lies (edges: bit 0 x low, 1 x high, 2 y low, 3 y high).  Compacted in no particular order, one atomic per
// wave; *count is the full number, records beyond cap are dropped (the host gives room for every slot).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_pairs_band(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                 const SelGroupDev* __restrict__ groups, PairsArgs P, uint32_t edges, uint32_t tile_index,
                 PairsBandRec* __restrict__ out, uint32_t cap, uint32_t* __restrict__ count) {
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  PairsSelf s;
  bool hit = pairs_self(g, a, i, limit, groups, P, &s);
  if (hit) {
    const unsigned long long R = P.reach;
    hit = ((edges & 1u) && (unsigned long long)s.cx < g.own_x0 + R) || ((edges & 2u) && s.cx + R >= g.own_x1) ||
          ((edges & 4u) && (unsigned long long)s.cy < g.own_y0 + R) || ((edges & 8u) && s.cy + R >= g.own_y1);
  }
  const unsigned long long m = __ballot(hit);
  if (!m) return;
  const uint32_t lane = __lane_id();
  const int first = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if ((int)lane == first) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = __shfl(base, first, 64);
  if (!hit) return;
  const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (at >= cap) return;
  PairsBandRec r;
  r.x = s.x;
  r.y = s.y;
  r.id = s.id;
  r.bits = (s.ra ? 1u : 0u) | (s.rb ? 2u : 0u) | (tile_index << 2);
  out[at] = r;
}

// One lane per band record of the local tile against the n_f foreign records, staged PAIRS_BLOCK at a time in LDS (6 KiB;
// every lane of a wave reads the same staged record: a broadcast).  Every lane of the workgroup runs the loop.
template <bool EMIT>
__device__ __forceinline__ uint32_t pairs_cross_walk(const PairsBandRec& me, bool live,
                                                     const PairsBandRec* __restrict__ foreign, uint32_t n_f, double dist2,
                                                     PairsBandRec* s_f, unsigned long long at, unsigned long long cap,
                                                     unsigned long long* __restrict__ keys, double* __restrict__ d2s,
                                                     uint32_t* top) {
  uint32_t n = 0;
  for (uint32_t base = 0; base < n_f; base += PAIRS_BLOCK) {
    __syncthreads();  // (the chunk before is read)
    if (base + threadIdx.x < n_f) s_f[threadIdx.x] = foreign[base + threadIdx.x];
    __syncthreads();
    const uint32_t m = min(PAIRS_BLOCK, n_f - base);
    if (!live) continue;
    for (uint32_t k = 0; k < m; ++k) {
      const PairsBandRec q = s_f[k];
      const double dx = me.x - q.x, dy = me.y - q.y;
      const double d2 = dx * dx + dy * dy;
      if (!(d2 < dist2)) continue;
      if (!(((me.bits & 1u) && (q.bits & 2u)) || ((q.bits & 1u) && (me.bits & 2u)))) continue;
      if (EMIT) {
        if (at + n < cap) {
          const uint32_t lo = min(me.id, q.id), hi = max(me.id, q.id);
          keys[at + n] = ((unsigned long long)lo << 32) | hi;
          if (d2s) d2s[at + n] = d2;
        }
        *top = max(*top, max(me.id, q.id));
      }
      ++n;
    }
  }
  return n;
}

__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_pairs_cross_count(const PairsBandRec* __restrict__ local, uint32_t n_l, const PairsBandRec* __restrict__ foreign,
                        uint32_t n_f, double dist2, unsigned long long* __restrict__ hdr) {
  __shared__ PairsBandRec s_f[PAIRS_BLOCK];
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const bool live = i < n_l;
  PairsBandRec me = {};
  if (live) me = local[i];
  const uint32_t n = pairs_cross_walk<false>(me, live, foreign, n_f, dist2, s_f, 0ull, 0ull, nullptr, nullptr, nullptr);
  pairs_block_tally(n, &hdr[0]);
}

__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_pairs_cross_emit(const PairsBandRec* __restrict__ local, uint32_t n_l, const PairsBandRec* __restrict__ foreign,
                       uint32_t n_f, double dist2, unsigned long long* __restrict__ hdr,
                       unsigned long long* __restrict__ keys, double* __restrict__ d2s, unsigned long long cap) {
  __shared__ PairsBandRec s_f[PAIRS_BLOCK];
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const bool live = i < n_l;
  PairsBandRec me = {};
  if (live) me = local[i];
  const uint32_t n = pairs_cross_walk<false>(me, live, foreign, n_f, dist2, s_f, 0ull, 0ull, nullptr, nullptr, nullptr);
  const unsigned long long at = pairs_block_place(n, &hdr[1]);
  uint32_t top = 0;
  pairs_cross_walk<true>(me, live && n, foreign, n_f, dist2, s_f, at, cap, keys, d2s, &top);
  pairs_block_top(top, reinterpret_cast<uint32_t*>(&hdr[2]));
}

// The sort of the list: k_ids_hist and k_ids_scatter over 64-bit keys with an optional f64 payload (the scan of the
// histogram does not see the keys: k_ids_scan serves as it is).  Tiles, items and radix are those of the ids' sort.
__global__ void __launch_bounds__(IDS_BLOCK)
    k_pairs_hist(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t shift, uint32_t* __restrict__ hist,
                 uint32_t n_tiles) {
  __shared__ uint32_t cnt[IDS_RADIX];
  if (threadIdx.x < IDS_RADIX) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * IDS_TILE;
  for (uint32_t k = threadIdx.x; k < IDS_TILE; k += IDS_BLOCK)
    if (base + k < n) atomicAdd(&cnt[(uint32_t)(keys[base + k] >> shift) & (IDS_RADIX - 1u)], 1u);
  __syncthreads();
  if (threadIdx.x < IDS_RADIX) hist[threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

// stable scatter of one digit: thread t of tile b owns keys [b * IDS_TILE + t * IDS_ITEMS, + IDS_ITEMS)
__global__ void __launch_bounds__(IDS_BLOCK)
    k_pairs_scatter(const unsigned long long* __restrict__ keys, unsigned long long* __restrict__ out,
                    const double* __restrict__ pay, double* __restrict__ pay_out, uint32_t n, uint32_t shift,
                    const uint32_t* __restrict__ hist, uint32_t n_tiles) {
  __shared__ uint32_t cnt[IDS_RADIX][IDS_BLOCK];
  __shared__ uint32_t seg[IDS_RADIX][IDS_RADIX];
  const uint32_t t = threadIdx.x;
  const uint32_t base = blockIdx.x * IDS_TILE + t * IDS_ITEMS;
  for (uint32_t d = 0; d < IDS_RADIX; ++d) cnt[d][t] = 0;
  for (uint32_t j = 0; j < IDS_ITEMS; ++j)
    if (base + j < n) ++cnt[(uint32_t)(keys[base + j] >> shift) & (IDS_RADIX - 1u)][t];
  __syncthreads();
  {  // exclusive scan along the threads for every digit: thread (d, s) takes 16 threads' counts of digit d
    const uint32_t d = t / IDS_RADIX, s = t % IDS_RADIX;
    uint32_t* row = &cnt[d][s * (IDS_BLOCK / IDS_RADIX)];
    uint32_t sum = 0;
    for (uint32_t u = 0; u < IDS_BLOCK / IDS_RADIX; ++u) sum += row[u];
    seg[d][s] = sum;
    __syncthreads();
    uint32_t run = hist[d * n_tiles + blockIdx.x];
    for (uint32_t u = 0; u < s; ++u) run += seg[d][u];
    for (uint32_t u = 0; u < IDS_BLOCK / IDS_RADIX; ++u) {
      const uint32_t v = row[u];
      row[u] = run;
      run += v;
    }
  }
  __syncthreads();
  for (uint32_t j = 0; j < IDS_ITEMS; ++j) {
    if (base + j >= n) break;
    const unsigned long long k = keys[base + j];
    const uint32_t at = cnt[(uint32_t)(k >> shift) & (IDS_RADIX - 1u)][t]++;
    if (at < n) {
      out[at] = k;
      if (pay) pay_out[at] = pay[base + j];
    }
  }
}

namespace {

// one listed pair on the host: the key (device ids, a << 32 | b) and the left-hand side
struct PairRec {
  uint64_t key;
  double d2;
};
bool operator<(const PairRec& l, const PairRec& r) { return l.key < r.key; }

// merge the ascending runs of v ending at `ends` (pairwise, in place): mesh_merge_runs for pairs
void pairs_merge_runs(std::vector<PairRec>& v, std::vector<size_t> ends) {
  while (ends.size() > 1) {
    std::vector<size_t> next;
    for (size_t i = 0; i < ends.size(); i += 2) {
      if (i + 1 < ends.size()) {
        const size_t b = i ? ends[i - 1] : 0;
        std::inplace_merge(v.begin() + (long)b, v.begin() + (long)ends[i], v.begin() + (long)ends[i + 1]);
      }
      next.push_back(ends[std::min(i + 1, ends.size() - 1)]);
    }
    ends.swap(next);
  }
}

// a NaN or negative distance, a selection cs_select_agents refuses, distances without pairs (3)
int pairs_check(std::string* error, double distance, const cs_selection* sa, const cs_selection* sb,
                const cs_id_pair* out_pairs, const double* out_d2) {
  if (!(distance >= 0.0)) {
    *error = "close_pairs: the distance is NaN or negative";
    return 3;
  }
  if (sa)
    if (int rc = sel_check(error, sa, "close_pairs")) return rc;
  if (sb)
    if (int rc = sel_check(error, sb, "close_pairs")) return rc;
  if (out_d2 && !out_pairs) {
    *error = "close_pairs: out_d2 without out_pairs";
    return 3;
  }
  return 0;
}

PairsArgs pairs_args(const cs_engine* e, double distance, const cs_selection* sa, const cs_selection* sb) {
  PairsArgs P{};
  const double cs = e->grid.cell_size;
  // the low corners of cell (0, 0) and of the cell one beyond the last row and column, as cs_engine::to_global gives them
  P.gx0 = e->grid.offset_x + ((double)(uint64_t)0 * cs + (double)0.0f);
  P.gy0 = e->grid.offset_y + ((double)(uint64_t)0 * cs + (double)0.0f);
  P.gx1 = e->grid.offset_x + ((double)e->gny * cs + (double)0.0f);  // (x runs over the gny rows, y over the gnx columns)
  P.gy1 = e->grid.offset_y + ((double)e->gnx * cs + (double)0.0f);
  P.dist2 = distance * distance;
  P.off_x = e->grid.offset_x;
  P.off_y = e->grid.offset_y;
  P.cell_size = cs;
  const uint64_t most = std::max<uint64_t>(std::max(e->nx, e->ny), 1u);  // (a reach of the whole local grid reaches everyone)
  const double cells = std::ceil(distance / cs);
  P.reach = (uint32_t)((cells < (double)most) ? std::min<uint64_t>((uint64_t)cells + 1u, most) : most);
  P.owned_only = (e->tile && e->ghosts_present) ? 1u : 0u;
  P.n_groups = (uint32_t)e->groups.size();
  P.roles = (sa ? 1u : 0u) | (sb ? 2u : 0u);
  if (sa) P.a = *sa;
  if (sb) P.b = *sb;
  P.want_vel = ((sa && (sa->terms & CS_SEL_SPEED)) || (sb && (sb->terms & CS_SEL_SPEED))) ? 1u : 0u;
  return P;
}

// The pair arrays of one listing: in cs_engine::pairs_scratch while they fit PAIRS_SCRATCH_KEEP, else allocated for the
// call and freed when this goes out of scope.
struct PairsScratch {
  cs_engine* e;
  void* temp = nullptr;
  explicit PairsScratch(cs_engine* e_) : e(e_) {}
  PairsScratch(const PairsScratch&) = delete;
  PairsScratch& operator=(const PairsScratch&) = delete;
  ~PairsScratch() {
    if (!temp) return;
    hipStreamSynchronize(e->stream);
    hipFree(temp);
  }
  void* get(size_t need) {
    if (need > PAIRS_SCRATCH_KEEP) {
      if (hipMalloc(&temp, need) != hipSuccess) {
        temp = nullptr;
        e->error = "close_pairs: out of device memory for the list of pairs";
        return nullptr;
      }
      return temp;
    }
    if (need > e->pairs_scratch_bytes) {
      if (e->pairs_scratch) {
        hipStreamSynchronize(e->stream);
        hipFree(e->pairs_scratch);
      }
      e->pairs_scratch = nullptr;
      e->pairs_scratch_bytes = 0;
      if (hipMalloc(&e->pairs_scratch, need) != hipSuccess) {
        e->pairs_scratch = nullptr;
        e->error = "close_pairs: out of device memory for the list of pairs";
        return nullptr;
      }
      e->pairs_scratch_bytes = need;
    }
    return e->pairs_scratch;
  }
};

// the pair arrays in one allocation
struct PairsArrays {
  unsigned long long *keys = nullptr, *keys_other = nullptr;
  double *d2 = nullptr, *d2_other = nullptr;
  uint32_t* hist = nullptr;
  unsigned char* rest = nullptr;  // `extra` bytes behind them
};
int pairs_arrays(PairsScratch* sc, uint64_t count, bool want_d2, size_t extra, PairsArrays* out) {
  const size_t b_keys = sel_up((size_t)count * sizeof(uint64_t)), b_d2 = want_d2 ? b_keys : 0u;
  const size_t tiles = ((size_t)count + IDS_TILE - 1u) / IDS_TILE;
  const size_t b_hist = sel_up(IDS_RADIX * std::max<size_t>(tiles, 1u) * sizeof(uint32_t));
  unsigned char* p = static_cast<unsigned char*>(sc->get(2u * b_keys + 2u * b_d2 + b_hist + sel_up(extra) + 256u));
  if (!p) return 90;
  out->keys = reinterpret_cast<unsigned long long*>(p);
  out->keys_other = reinterpret_cast<unsigned long long*>(p + b_keys);
  out->d2 = want_d2 ? reinterpret_cast<double*>(p + 2u * b_keys) : nullptr;
  out->d2_other = want_d2 ? reinterpret_cast<double*>(p + 2u * b_keys + b_d2) : nullptr;
  out->hist = reinterpret_cast<uint32_t*>(p + 2u * b_keys + 2u * b_d2);
  out->rest = p + 2u * b_keys + 2u * b_d2 + b_hist;
  return 0;
}

// The radix passes over `count` listed pairs whose largest id is `top`, then the first `take` of them to the host.
int pairs_sort_download(cs_engine* e, PairsArrays A, uint64_t count, uint32_t top, size_t take, std::vector<PairRec>* out) {
  const uint32_t n = (uint32_t)count;  // (at most CS_PAIRS_MAX)
  if (n > 1u) {
    const uint32_t tiles = (n + IDS_TILE - 1u) / IDS_TILE;
    const uint32_t bits = top ? 32u - (uint32_t)__builtin_clz(top) : 1u;
    for (uint32_t word = 0; word < 64u; word += 32u)  // b in the low half, a in the high half, both at most `top`
      for (uint32_t shift = word; shift < word + bits; shift += 4u) {
        hipLaunchKernelGGL(k_pairs_hist, dim3(tiles), dim3(IDS_BLOCK), 0, e->stream, A.keys, n, shift, A.hist, tiles);
        hipLaunchKernelGGL(k_ids_scan, dim3(1), dim3(IDS_BLOCK), 0, e->stream, A.hist, IDS_RADIX * tiles);
        hipLaunchKernelGGL(k_pairs_scatter, dim3(tiles), dim3(IDS_BLOCK), 0, e->stream, A.keys, A.keys_other, A.d2, A.d2_other,
                           n, shift, A.hist, tiles);
        std::swap(A.keys, A.keys_other);
        std::swap(A.d2, A.d2_other);
      }
    HIP_OK_E(e, hipGetLastError());
  }
  take = std::min<size_t>(take, n);
  std::vector<uint64_t> keys(take);
  std::vector<double> d2(A.d2 ? take : 0u);
  if (take) {
    HIP_OK_E(e, hipMemcpyAsync(keys.data(), A.keys, take * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    if (A.d2) HIP_OK_E(e, hipMemcpyAsync(d2.data(), A.d2, take * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  }
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  out->resize(take);
  for (size_t k = 0; k < take; ++k) (*out)[k] = PairRec{keys[k], A.d2 ? d2[k] : 0.0};
  return 0;
}

// the 256-byte header of a count or a listing, in the by-id scratch, zeroed on the stream
int pairs_header(cs_engine* e, unsigned long long** hdr) {
  if (int rc = write_scratch_reserve(e, 256u)) return rc;
  *hdr = static_cast<unsigned long long*>(e->write_scratch);
  HIP_OK_E(e, hipMemsetAsync(*hdr, 0, 256u, e->stream));
  return 0;
}

// The pairs among the agents one engine holds (after sel_begin): *count = all of them; with want > 0 the first
// min(*count, want) of them in `out`, ascending, as device ids, unless *count is above CS_PAIRS_MAX (*too_many).
// One memset, one kernel and one read back for the count; for the list one more kernel, one read back, three launches
// per 4 bits of the largest id and half of the key, one download.
int pairs_run(cs_engine* e, const PairsArgs& P, size_t want, bool want_d2, std::vector<PairRec>* out, uint64_t* count,
              bool* too_many) {
  out->clear();
  *count = 0;
  *too_many = false;
  if (int rc = e->refresh_counts()) return rc;
  if (int rc = e->ensure_index()) return rc;
  const uint32_t n = e->n_slots;
  if (!n || !(P.dist2 > 0.0)) return 0;  // (distance 0: the comparison is strict)
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  const uint32_t blocks = (n + PAIRS_BLOCK - 1u) / PAIRS_BLOCK;
  hipLaunchKernelGGL(k_pairs_count, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], n, e->cell_start,
                     e->sel_groups_dev, P, hdr);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long found = 0;
  HIP_OK_E(e, hipMemcpyAsync(&found, hdr, sizeof found, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  *count = found;
  if (!want || !found) return 0;
  if (found > CS_PAIRS_MAX) {
    *too_many = true;
    return 0;
  }
  PairsScratch sc(e);
  PairsArrays A;
  if (int rc = pairs_arrays(&sc, found, want_d2, 0u, &A)) return rc;
  hipLaunchKernelGGL(k_pairs_emit, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], n, e->cell_start,
                     e->sel_groups_dev, P, hdr, A.keys, A.d2, (unsigned long long)found);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long back[3] = {0, 0, 0};
  HIP_OK_E(e, hipMemcpyAsync(back, hdr, sizeof back, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  if (back[1] != found) {
    e->error = "close_pairs: the listing found another number of pairs than the count";
    return 90;
  }
  return pairs_sort_download(e, A, found, (uint32_t)back[2], want, out);
}

int pairs_too_many(std::string* error) {
  *error = "close_pairs: too many pairs to list (more than CS_PAIRS_MAX = 67108864); the count-only form has no limit";
  return 3;
}

// device ids -> external ids, into the caller's arrays
void pairs_copy_out(const cs_engine* ids_of, const std::vector<PairRec>& list, cs_id_pair* out_pairs, double* out_d2,
                    size_t cap) {
  const size_t k = std::min(list.size(), cap);
  for (size_t i = 0; i < k; ++i) {
    out_pairs[i].a = ids_of->ext_id(list[i].key >> 32);
    out_pairs[i].b = ids_of->ext_id(list[i].key & 0xFFFFFFFFull);
    if (out_d2) out_d2[i] = list[i].d2;
  }
}

// The band of one tile of a mesh (after pairs_run on it: sorted) to the host.
int pairs_band_export(cs_mesh* m, size_t local, const PairsArgs& P, std::vector<PairsBandRec>* out) {
  cs_engine* e = m->tiles[local];
  out->clear();
  const uint32_t n = e->n_slots;
  uint32_t edges = 0;
  for (int d = 0; d < 4; ++d)
    if (m->neighbour(m->index_of[local], d) >= 0) edges |= 1u << d;  // (CS_DIR_XLO, XHI, YLO, YHI)
  if (!n || !edges || !(P.dist2 > 0.0)) return 0;
  PairsScratch sc(e);
  unsigned char* p = static_cast<unsigned char*>(sc.get(256u + (size_t)n * sizeof(PairsBandRec)));
  if (!p) return 90;
  uint32_t* d_count = reinterpret_cast<uint32_t*>(p);
  PairsBandRec* d_rec = reinterpret_cast<PairsBandRec*>(p + 256u);
  HIP_OK_E(e, hipMemsetAsync(d_count, 0, sizeof(uint32_t), e->stream));
  hipLaunchKernelGGL(k_pairs_band, dim3((n + PAIRS_BLOCK - 1u) / PAIRS_BLOCK), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev,
                     e->buf[e->cur], n, e->cell_start, e->sel_groups_dev, P, edges, m->index_of[local], d_rec, n, d_count);
  HIP_OK_E(e, hipGetLastError());
  uint32_t found = 0;
  HIP_OK_E(e, hipMemcpyAsync(&found, d_count, sizeof found, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  if (found > n) {
    e->error = "close_pairs: more band records than slots";
    return 90;
  }
  out->resize(found);
  if (found) {
    HIP_OK_E(e, hipMemcpyAsync(out->data(), d_rec, (size_t)found * sizeof(PairsBandRec), hipMemcpyDeviceToHost, e->stream));
    HIP_OK_E(e, hipStreamSynchronize(e->stream));
  }
  return 0;
}

// The pairs between the band of one local tile and the records of the tiles with a higher index, on that tile's device.
int pairs_cross(cs_engine* e, const std::vector<PairsBandRec>& local, const std::vector<PairsBandRec>& foreign, double dist2,
                size_t want, bool want_d2, std::vector<PairRec>* out, uint64_t* count, bool* too_many) {
  out->clear();
  *count = 0;
  *too_many = false;
  if (local.empty() || foreign.empty()) return 0;
  const uint32_t n_l = (uint32_t)local.size(), n_f = (uint32_t)foreign.size();
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  PairsScratch recs(e);
  const size_t b_l = sel_up((size_t)n_l * sizeof(PairsBandRec)), b_f = sel_up((size_t)n_f * sizeof(PairsBandRec));
  unsigned char* p = static_cast<unsigned char*>(recs.get(b_l + b_f));
  if (!p) return 90;
  PairsBandRec* d_l = reinterpret_cast<PairsBandRec*>(p);
  PairsBandRec* d_f = reinterpret_cast<PairsBandRec*>(p + b_l);
  HIP_OK_E(e, hipMemcpyAsync(d_l, local.data(), (size_t)n_l * sizeof(PairsBandRec), hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(d_f, foreign.data(), (size_t)n_f * sizeof(PairsBandRec), hipMemcpyHostToDevice, e->stream));
  const uint32_t blocks = (n_l + PAIRS_BLOCK - 1u) / PAIRS_BLOCK;
  hipLaunchKernelGGL(k_pairs_cross_count, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, d_l, n_l, d_f, n_f, dist2, hdr);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long found = 0;
  HIP_OK_E(e, hipMemcpyAsync(&found, hdr, sizeof found, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (the host records are uploaded)
  *count = found;
  if (!want || !found) return 0;
  if (found > CS_PAIRS_MAX) {
    *too_many = true;
    return 0;
  }
  // (the records stay where they are: the list takes an allocation of its own when both do not fit the kept scratch)
  PairsScratch sc(e);
  PairsArrays A;
  const bool share = recs.temp == nullptr;  // the records lie in the kept scratch: the list must not move them
  if (share) {
    const size_t b_keys = sel_up((size_t)found * sizeof(uint64_t));
    const size_t tiles = ((size_t)found + IDS_TILE - 1u) / IDS_TILE;
    const size_t need = 2u * b_keys + (want_d2 ? 2u * b_keys : 0u) + sel_up(IDS_RADIX * tiles * sizeof(uint32_t)) + 256u;
    void* q = nullptr;
    if (hipMalloc(&q, need) != hipSuccess) {
      e->error = "close_pairs: out of device memory for the list of pairs";
      return 90;
    }
    sc.temp = q;  // (freed with sc)
    unsigned char* b = static_cast<unsigned char*>(q);
    A.keys = reinterpret_cast<unsigned long long*>(b);
    A.keys_other = reinterpret_cast<unsigned long long*>(b + b_keys);
    A.d2 = want_d2 ? reinterpret_cast<double*>(b + 2u * b_keys) : nullptr;
    A.d2_other = want_d2 ? reinterpret_cast<double*>(b + 3u * b_keys) : nullptr;
    A.hist = reinterpret_cast<uint32_t*>(b + (want_d2 ? 4u : 2u) * b_keys);
  } else if (int rc = pairs_arrays(&sc, found, want_d2, 0u, &A)) {
    return rc;
  }
  hipLaunchKernelGGL(k_pairs_cross_emit, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, d_l, n_l, d_f, n_f, dist2, hdr, A.keys,
                     A.d2, (unsigned long long)found);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long back[3] = {0, 0, 0};
  HIP_OK_E(e, hipMemcpyAsync(back, hdr, sizeof back, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  if (back[1] != found) {
    e->error = "close_pairs: the listing found another number of pairs than the count";
    return 90;
  }
  return pairs_sort_download(e, A, found, (uint32_t)back[2], want, out);
}

}  // namespace

extern "C" {

size_t cs_close_pairs(cs_engine* e, double distance, const cs_selection* sel_a, const cs_selection* sel_b,
                      cs_id_pair* out_pairs, double* out_d2, size_t cap) {
  if (!e) return SIZE_MAX;
  hipSetDevice(e->device);
  if (pairs_check(&e->error, distance, sel_a, sel_b, out_pairs, out_d2)) return SIZE_MAX;
  if (sel_begin(e)) return SIZE_MAX;
  const size_t want = out_pairs ? cap : 0u;
  const PairsArgs P = pairs_args(e, distance, sel_a, sel_b);
  std::vector<PairRec> list;
  uint64_t count = 0;
  bool too_many = false;
  if (pairs_run(e, P, want, out_d2 != nullptr, &list, &count, &too_many)) return SIZE_MAX;
  if (too_many) {
    pairs_too_many(&e->error);
    return SIZE_MAX;
  }
  if (want) pairs_copy_out(e, list, out_pairs, out_d2, cap);
  return (size_t)count;
}

// Collective: two gathers of variable size (two collectives each), whatever the crowd and the answer.  The first carries
// every rank's band records, the second its pairs (the count-only form: its counts).
size_t cs_mesh_close_pairs(cs_mesh* m, double distance, const cs_selection* sel_a, const cs_selection* sel_b,
                           cs_id_pair* out_pairs, double* out_d2, size_t cap) {
  if (!m) return SIZE_MAX;
  if (m->dead()) return SIZE_MAX;
  if (pairs_check(&m->error, distance, sel_a, sel_b, out_pairs, out_d2)) return SIZE_MAX;
  if (m->n_tiles() > 1u && distance > (double)m->halo * m->grid.cell_size) {
    m->error = "close_pairs: on a mesh of more than one tile the distance is at most halo_cells * cell_size";
    return SIZE_MAX;
  }
  if (cs_mesh_synchronize(m)) return SIZE_MAX;
  hipSetDevice(m->device);
  const size_t want = out_pairs ? cap : 0u;
  const bool want_d2 = out_d2 != nullptr;
  int err = 0;
  bool too_many = false;
  std::string why;
  uint64_t total = 0;
  std::vector<PairRec> all;  // the sorted runs, one behind the other
  std::vector<size_t> ends;
  std::vector<std::vector<PairsBandRec>> bands(m->tiles.size());
  double dist2 = distance * distance;
  // 1. every tile: the pairs among the agents it holds, and its band
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    cs_engine* e = m->tiles[k];
    std::vector<PairRec> part;
    uint64_t c = 0;
    bool many = false;
    if (!err) err = sel_begin(e);
    const PairsArgs P = pairs_args(e, distance, sel_a, sel_b);
    if (!err) err = pairs_run(e, P, want, want_d2, &part, &c, &many);
    if (!err && m->n_tiles() > 1u) err = pairs_band_export(m, k, P, &bands[k]);
    if (err && why.empty()) why = cs_last_error(e);
    too_many = too_many || many;
    total += c;
    all.insert(all.end(), part.begin(), part.end());
    ends.push_back(all.size());
  }
  // 2. the band records of every tile on every rank: [failed?], then the records as three words each
  std::vector<PairsBandRec> every;
  if (m->distributed) {
    std::vector<uint64_t> mine(1, err ? 1u : 0u);
    if (!err)
      for (const auto& b : bands) {
        const size_t at = mine.size();
        mine.resize(at + 3u * b.size());
        if (!b.empty()) std::memcpy(&mine[at], b.data(), b.size() * sizeof(PairsBandRec));
      }
    std::vector<std::vector<unsigned char>> parts;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), parts)) {
      m->poison(rc, m->error);
      return SIZE_MAX;
    }
    for (const auto& part : parts) {
      uint64_t failed = 1u;
      if (part.size() >= sizeof failed) std::memcpy(&failed, part.data(), sizeof failed);
      if (failed || (part.size() - sizeof(uint64_t)) % sizeof(PairsBandRec)) {
        if (!err) {
          err = 90;
          why = "a tile of another rank failed while listing pairs";
        }
        continue;
      }
      const size_t k = (part.size() - sizeof(uint64_t)) / sizeof(PairsBandRec), at = every.size();
      every.resize(at + k);
      if (k) std::memcpy(&every[at], part.data() + sizeof(uint64_t), k * sizeof(PairsBandRec));
    }
  } else {
    for (const auto& b : bands) every.insert(every.end(), b.begin(), b.end());
  }
  // 3. every local tile's band against the records of the tiles with a higher index: each cross-tile pair once
  for (size_t k = 0; k < m->tiles.size() && !err; ++k) {
    const uint32_t index = m->index_of[k];
    std::vector<PairsBandRec> foreign;
    for (const PairsBandRec& r : every)
      if ((r.bits >> 2) > index) foreign.push_back(r);
    std::vector<PairRec> part;
    uint64_t c = 0;
    bool many = false;
    err = pairs_cross(m->tiles[k], bands[k], foreign, dist2, want, want_d2, &part, &c, &many);
    if (err && why.empty()) why = cs_last_error(m->tiles[k]);
    too_many = too_many || many;
    total += c;
    all.insert(all.end(), part.begin(), part.end());
    ends.push_back(all.size());
  }
  pairs_merge_runs(all, ends);
  if (all.size() > want) all.resize(want);
  // 4. the pairs (or only the counts) of every rank: [0 ok / 1 failed / 2 too many, count, n listed, keys, d2]
  if (m->distributed) {
    std::vector<uint64_t> mine{err ? 1u : (too_many ? 2u : 0u), total, (err || too_many) ? 0u : all.size()};
    if (mine[2]) {
      const size_t n = all.size();
      mine.resize(3u + 2u * n);
      for (size_t i = 0; i < n; ++i) {
        mine[3u + i] = all[i].key;
        std::memcpy(&mine[3u + n + i], &all[i].d2, sizeof(double));
      }
    }
    std::vector<std::vector<unsigned char>> parts;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), parts)) {
      m->poison(rc, m->error);
      return SIZE_MAX;
    }
    all.clear();
    ends.clear();
    total = 0;
    for (const auto& part : parts) {
      const size_t words = part.size() / sizeof(uint64_t);
      std::vector<uint64_t> w(words);
      if (words) std::memcpy(w.data(), part.data(), words * sizeof(uint64_t));
      if (words < 3u || w[0] == 1u || words != 3u + 2u * w[2]) {
        if (!err) {
          err = 90;
          why = "a tile of another rank failed while listing pairs";
        }
        continue;
      }
      if (w[0] == 2u) too_many = true;
      total += w[1];
      const size_t n = (size_t)w[2];
      for (size_t i = 0; i < n; ++i) {
        PairRec r;
        r.key = w[3u + i];
        std::memcpy(&r.d2, &w[3u + n + i], sizeof(double));
        all.push_back(r);
      }
      ends.push_back(all.size());
    }
    pairs_merge_runs(all, ends);
    if (all.size() > want) all.resize(want);
  }
  if (err) {
    m->error = why;
    return SIZE_MAX;
  }
  if (want && (too_many || total > CS_PAIRS_MAX)) {
    pairs_too_many(&m->error);
    return SIZE_MAX;
  }
  if (want && !m->tiles.empty()) pairs_copy_out(m->tiles[0], all, out_pairs, out_d2, cap);
  return (size_t)total;
}

}  // extern "C"
