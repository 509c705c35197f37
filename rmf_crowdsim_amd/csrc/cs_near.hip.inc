// cs_near.hip.inc — what the between-step distance queries share: cs_close_pairs.hip.inc, cs_clusters.hip.inc and
// cs_neighbours.hip.inc (include/crowdstep_state.h).  Part of the single translation unit crowdstep_hip.hip (included
// there, after cs_field.hip.inc and before the three; it uses sel_load / sel_pred / sel_check of cs_select.hip.inc,
// k_ids_scan of cs_kernels_ids.hip.inc and mesh_host_gatherv of cs_mesh.hip.inc, none of which it changes).  Each piece
// is written ONCE, here; the three files hold what is their own: what they do with a candidate that passed.
//
//   near_walk      the walk of one lane over the slots of the CELL-SORTED arrays around its own agent: the rectangle of
//                  `reach` cells each way, clipped to the (owned) grid, row by row.  The cells (row, y_lo .. y_hi) of
//                  one row are ONE run of slots, cell_start[row * nx + y_lo] .. cell_start[row * nx + y_hi + 1], so the
//                  walk is a loop over slots, however many of them one cell holds.  A visitor says which slots it wants
//                  before anything else of them is read (take) and gets every candidate with dx * dx + dy * dy <
//                  distance^2, in f64, with its rebuilt position (hit).
//   candidates     are RECOMPUTED FROM THEIR COLUMNS (cell, off, id: 16 bytes), not staged in LDS: the lanes of a
//                  workgroup are slots in cell order, their rectangles overlap but differ (a workgroup would have to
//                  stage the union of them, several times what one lane reads, and index into it per lane), the reach
//                  and the occupancy of a cell are the caller's, so no fixed LDS budget fits, and the reads of
//                  neighbouring lanes hit the same cache lines anyway.  What costs more than the test, the
//                  candidate's own rectangle test (pairs_in_grid) and its role bits (near_roles: meta, group table,
//                  velocity, two selections), is evaluated only for candidates that passed the distance test.
//   no pre-reject  there is no f32 pre-reject: every decision is the f64 expression itself.
//   tally / place  a lane counts its own hits (its walk is its own, so there is no ballot to take per candidate); the
//                  counts are summed over the wave by shuffles, over the workgroup in LDS, and leave with ONE 64-bit
//                  atomic per workgroup (pairs_block_tally), or take the workgroup's place in a list with one atomic
//                  and a prefix sum over its lanes (pairs_block_place).
//   sort           LSD radix over 4-bit digits of 64-bit keys with an optional f64 payload, k_pairs_hist / k_ids_scan /
//                  k_pairs_scatter (pairs_radix); the digits above the bits of the largest word listed are skipped.
//   mesh           near_in_band + near_wave_place: the band of a tile, the agents whose cell lies within `reach` cells
//                  of an owned edge behind which another tile lies, compacted with one atomic per wave (k_pairs_band
//                  for the pairs and the neighbours; the clusters keep a record of their own).  near_cross: one lane
//                  per local band record against the gathered foreign records, staged in LDS, the same f64 expression.
//                  mesh_gather_bands brings every rank's band records to every rank.
//
// WHY THE WALK IS CONSERVATIVE.  Only participants can be in a pair: agents whose reported position is finite and inside
// the grid's own rectangle.  The agents whose stored offset does not lie in the cell they are indexed under are the ones
// clamped into row or column 0 from below the low edge (reported below gx0 / gy0), the ones aliased beyond the row
// stride (reported at or above gy1) and the ones with a NaN position: none of them takes part.  For a participant the
// offset lies in [0, cell_size] of its cell (up to one rounding), so two participants closer than `distance` along an axis
// stand in cells at most distance / cell_size + 1 apart along it; the walk reaches ceil(distance / cell_size) + 1.
//
// Scratch: a count needs 256 bytes of the by-id scratch (pairs_header).  The lists live in cs_engine::pairs_scratch while
// they need at most PAIRS_SCRATCH_KEEP bytes (16 MiB: kept and counted by cs_device_bytes); a larger need is allocated
// for the call and freed before it returns (PairsScratch).

#define PAIRS_BLOCK 256u
#define PAIRS_WAVES (PAIRS_BLOCK / 64u)
#define PAIRS_SCRATCH_KEEP ((size_t)16u << 20)
#define NEAR_NO_PLACE 0xFFFFFFFFu

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

// The walk of one lane whose agent stands at (sx, sy) in cell (scx, scy).  v.take(a, j): does slot j count at all (asked
// before its cell and offset are read); v.hit(g, a, P, j, xq, yq, d2): slot j stands at (xq, yq), d2 < dist2 away.
// A visitor holds what is its own and gets g, a and P from the walk: one that kept references to these kernel arguments
// cost k_neighbours the select forms of sel_pred and 36 bytes of private segment.
template <class V>
__device__ __forceinline__ void near_walk(const GridDev& g, const AgentArrays& a, uint32_t limit,
                                          const uint32_t* __restrict__ cell_start, const PairsArgs& P, double sx, double sy,
                                          uint32_t scx, uint32_t scy, V& v) {
  // the rectangle of cells, clipped to the (owned) grid: rows are x, g.ny of them; columns are y, g.nx of them
  const long long lo_x = P.owned_only ? g.own_x0 : 0u, hi_x = P.owned_only ? g.own_x1 : g.ny;
  const long long lo_y = P.owned_only ? g.own_y0 : 0u, hi_y = P.owned_only ? g.own_y1 : g.nx;
  const long long R = P.reach;
  const long long xl = max((long long)scx - R, lo_x), xh = min((long long)scx + R, hi_x - 1);
  const long long yl = max((long long)scy - R, lo_y), yh = min((long long)scy + R, hi_y - 1);
  if (yl > yh) return;
  for (long long xr = xl; xr <= xh; ++xr) {
    const uint32_t rowbase = (uint32_t)xr * g.nx;  // (below ncells, which fits 32 bits)
    const uint32_t b = cell_start[rowbase + (uint32_t)yl];
    const uint32_t e = min(cell_start[rowbase + (uint32_t)yh + 1u], limit);  // (index <= ncells: the table has ncells + 1)
    const double bx = (double)((uint64_t)g.org_x + (uint64_t)xr) * P.cell_size;
    for (uint32_t j = b; j < e; ++j) {
      if (!v.take(a, j)) continue;
      const uint32_t cyj = a.cell[j] - rowbase;
      if (cyj > (uint32_t)yh) continue;  // (a slot that is not of this row's run: cannot happen in sorted arrays)
      const float2 off = a.off[j];
      const double xq = P.off_x + (bx + (double)off.x);
      const double yq = P.off_y + ((double)((uint64_t)g.org_y + cyj) * P.cell_size + (double)off.y);
      const double dx = sx - xq, dy = sy - yq;
      const double d2 = dx * dx + dy * dy;
      if (!(d2 < P.dist2)) continue;
      v.hit(g, a, P, j, xq, yq, d2);
    }
  }
}

// The role bits of the candidate in slot j at (xq, yq), of those in `want` (1: role A, 2: role B; a role whose selection
// is not given is everyone's).  0 also for a group beyond the table.  A selection that is not wanted is not evaluated.
// For callers with P.roles != 0: with no selection given, everyone is of both roles and nothing of slot j need be read.
__device__ __forceinline__ uint32_t near_roles(const GridDev& g, const AgentArrays& a, uint32_t j,
                                               const SelGroupDev* groups, const PairsArgs& P, double xq, double yq,
                                               uint32_t want) {
  const uint32_t meta = a.meta[j];
  const uint32_t grp = meta_group(g, meta);
  if (grp >= P.n_groups) return 0u;
  if (!(P.roles & want)) return want;
  const SelGroupDev gq = groups[grp];
  const uint32_t wp = meta_waypoint(g, meta);
  double vx = 0.0, vy = 0.0;
  if (P.want_vel) {
    const float2 v = a.vel[j];
    vx = (double)v.x;
    vy = (double)v.y;
  }
  const bool qa = !(P.roles & want & 1u) || sel_pred(P.a, xq, yq, vx, vy, wp, gq.sink, gq.hlp, gq.lp);
  const bool qb = !(P.roles & want & 2u) || sel_pred(P.b, xq, yq, vx, vy, wp, gq.sink, gq.hlp, gq.lp);
  return (qa ? 1u : 0u) | (qb ? 2u : 0u);
}

// What a counting or a listing walk gathers: n entries; EMIT: written from keys[at] on (below cap), and top raised to
// the largest word written.
template <bool EMIT>
struct PairsSink {
  unsigned long long at, cap;
  unsigned long long* __restrict__ keys;
  double* __restrict__ d2s;
  uint32_t n, top;
  __device__ __forceinline__ void put(uint32_t hi, uint32_t lo, double d2) {
    if (EMIT) {
      if (at + n < cap) {
        keys[at + n] = ((unsigned long long)hi << 32) | lo;
        if (d2s) d2s[at + n] = d2;
      }
      top = max(top, max(hi, lo));
    }
    ++n;
  }
};

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

// The band of a tile: is cell (cx, cy) within `reach` cells of an owned edge behind which another tile lies (edges: bit 0
// x low, 1 x high, 2 y low, 3 y high)?
__device__ __forceinline__ bool near_in_band(const GridDev& g, uint32_t reach, uint32_t edges, uint32_t cx, uint32_t cy) {
  const unsigned long long R = reach;
  return ((edges & 1u) && (unsigned long long)cx < g.own_x0 + R) || ((edges & 2u) && cx + R >= g.own_x1) ||
         ((edges & 4u) && (unsigned long long)cy < g.own_y0 + R) || ((edges & 8u) && cy + R >= g.own_y1);
}

// The place of a lane's record in a list compacted in no particular order: the wave raises *count by its hits with ONE
// atomic (every lane of the wave calls this).  NEAR_NO_PLACE for a lane without a hit.  *count ends as the full number;
// the caller drops what lies beyond its room.
__device__ __forceinline__ uint32_t near_wave_place(bool hit, uint32_t* __restrict__ count) {
  const unsigned long long m = __ballot(hit);
  if (!m) return NEAR_NO_PLACE;
  const uint32_t lane = __lane_id();
  const int first = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if ((int)lane == first) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = __shfl(base, first, 64);
  if (!hit) return NEAR_NO_PLACE;
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// The band of a tile for the pairs and the neighbours: the participants (of a role) in it, one record each, records beyond
// cap dropped (the host gives room for every slot).  out_slot (may be null): the slot of every record.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_pairs_band(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                 const SelGroupDev* __restrict__ groups, PairsArgs P, uint32_t edges, uint32_t tile_index,
                 PairsBandRec* __restrict__ out, uint32_t* __restrict__ out_slot, uint32_t cap,
                 uint32_t* __restrict__ count) {
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  PairsSelf s;
  const bool hit = pairs_self(g, a, i, limit, groups, P, &s) && near_in_band(g, P.reach, edges, s.cx, s.cy);
  const uint32_t at = near_wave_place(hit, count);
  if (at >= cap) return;  // (NEAR_NO_PLACE is beyond every cap)
  PairsBandRec r;
  r.x = s.x;
  r.y = s.y;
  r.id = s.id;
  r.bits = (s.ra ? 1u : 0u) | (s.rb ? 2u : 0u) | (tile_index << 2);
  out[at] = r;
  if (out_slot) out_slot[at] = i;
}

// One lane per band record of the local tile (`me`; live: it takes part) against the n_f foreign records, staged
// PAIRS_BLOCK at a time in s_f (LDS; every lane of a wave reads the same staged record: a broadcast).  v.hit(me, q, d2) for
// every staged q with d2 < dist2.  Every lane of the workgroup runs the staging loop, live or not.
template <class Rec, class V>
__device__ __forceinline__ void near_cross(const Rec& me, bool live, const Rec* __restrict__ foreign, uint32_t n_f,
                                           double dist2, Rec* s_f, V& v) {
  for (uint32_t base = 0; base < n_f; base += PAIRS_BLOCK) {
    __syncthreads();  // (the chunk before is read)
    if (base + threadIdx.x < n_f) s_f[threadIdx.x] = foreign[base + threadIdx.x];
    __syncthreads();
    const uint32_t m = min(PAIRS_BLOCK, n_f - base);
    if (!live) continue;
    for (uint32_t k = 0; k < m; ++k) {
      const Rec q = s_f[k];
      const double dx = me.x - q.x, dy = me.y - q.y;
      const double d2 = dx * dx + dy * dy;
      if (!(d2 < dist2)) continue;
      v.hit(me, q, d2);
    }
  }
}

// The sort of a list: k_ids_hist and k_ids_scatter over 64-bit keys with an optional f64 payload (the scan of the
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

// `call`: the distance is NaN or negative (3)
int near_check_distance(std::string* error, double distance, const char* call) {
  if (distance >= 0.0) return 0;
  *error = std::string(call) + ": the distance is NaN or negative";
  return 3;
}

// `call` on a mesh: across a cut the bands see as far as the halo (3)
int near_check_mesh_distance(cs_mesh* m, double distance, const char* call) {
  if (m->n_tiles() <= 1u || !(distance > (double)m->halo * m->grid.cell_size)) return 0;
  m->error = std::string(call) + ": on a mesh of more than one tile the distance is at most halo_cells * cell_size";
  return 3;
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

// The arrays of one listing: in cs_engine::pairs_scratch while they fit PAIRS_SCRATCH_KEEP, else (or when `own` says so)
// allocated for the call and freed when this goes out of scope.  It serves all three queries; its out-of-memory text
// names close_pairs whichever call ran out, as it did before the queries shared it (error strings stay byte for byte).
struct PairsScratch {
  cs_engine* e;
  DevBytes temp;
  explicit PairsScratch(cs_engine* e_) : e(e_) {}
  ~PairsScratch() {
    if (temp.get()) hipStreamSynchronize(e->stream);  // (then `temp` frees it)
  }
  // One get per instance: a second one would free the first one's `temp` without waiting for the stream.
  void* get(size_t need, bool own = false) {
    const bool kept = !own && need <= PAIRS_SCRATCH_KEEP;
    if ((kept ? e->pairs_scratch.reserve(e->stream, need) : temp.alloc(need)) != hipSuccess) {
      e->error = "close_pairs: out of device memory for the list of pairs";
      return nullptr;
    }
    return kept ? e->pairs_scratch.get() : temp.get();
  }
};

// the 256-byte header of a count or a listing, in the by-id scratch, zeroed on the stream
int pairs_header(cs_engine* e, unsigned long long** hdr) {
  if (int rc = write_scratch_reserve(e, 256u)) return rc;
  *hdr = static_cast<unsigned long long*>(e->write_scratch.get());
  HIP_OK_E(e, hipMemsetAsync(*hdr, 0, 256u, e->stream));
  return 0;
}

// one word of a header (a count, a cursor) back on the host: one copy, one synchronise
int pairs_read_count(cs_engine* e, const unsigned long long* word, unsigned long long* found) {
  *found = 0;
  HIP_OK_E(e, hipMemcpyAsync(found, word, sizeof *found, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  return 0;
}
// the three words of a header (count, cursor, largest word listed) back on the host: one copy, one synchronise
int pairs_read_header(cs_engine* e, const unsigned long long* hdr, unsigned long long (&back)[3]) {
  back[0] = back[1] = back[2] = 0;
  HIP_OK_E(e, hipMemcpyAsync(back, hdr, sizeof back, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  return 0;
}

// The radix passes over the `bits` bits from bit `from` on of n keys (n > 1), with an optional f64 payload (pay and
// pay_other null, or pointing at null pointers: none): three launches per 4 bits.  *keys (and *pay) are the sorted
// arrays afterwards.
int pairs_radix(cs_engine* e, unsigned long long** keys, unsigned long long** other, double** pay, double** pay_other,
                uint32_t* hist, uint32_t n, uint32_t from, uint32_t bits) {
  const uint32_t tiles = (n + IDS_TILE - 1u) / IDS_TILE;
  for (uint32_t shift = from; shift < from + bits; shift += 4u) {
    hipLaunchKernelGGL(k_pairs_hist, dim3(tiles), dim3(IDS_BLOCK), 0, e->stream, *keys, n, shift, hist, tiles);
    hipLaunchKernelGGL(k_ids_scan, dim3(1), dim3(IDS_BLOCK), 0, e->stream, hist, IDS_RADIX * tiles);
    hipLaunchKernelGGL(k_pairs_scatter, dim3(tiles), dim3(IDS_BLOCK), 0, e->stream, *keys, *other,
                       pay ? (const double*)*pay : nullptr, pay ? *pay_other : nullptr, n, shift, hist, tiles);
    std::swap(*keys, *other);
    if (pay) std::swap(*pay, *pay_other);
  }
  HIP_OK_E(e, hipGetLastError());
  return 0;
}
// the bits of the largest word of a key
uint32_t pairs_bits(uint32_t top) { return top ? 32u - (uint32_t)__builtin_clz(top) : 1u; }

// The band of one tile (its arrays sorted) through k_pairs_band into d_rec, which has room for a record per slot (d_slot:
// the same, or null), counted in *d_count; then to the host.  One memset, one kernel, one read back, one download.
int pairs_band_run(cs_engine* e, const PairsArgs& P, uint32_t edges, uint32_t tile_index, uint32_t* d_count,
                   PairsBandRec* d_rec, uint32_t* d_slot, const char* call, std::vector<PairsBandRec>* out) {
  const uint32_t n = e->n_slots;
  HIP_OK_E(e, hipMemsetAsync(d_count, 0, sizeof(uint32_t), e->stream));
  hipLaunchKernelGGL(k_pairs_band, dim3((n + PAIRS_BLOCK - 1u) / PAIRS_BLOCK), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev,
                     e->buf[e->cur], n, e->cell_start.get(), e->sel_groups_dev.get(), P, edges, tile_index, d_rec, d_slot, n, d_count);
  HIP_OK_E(e, hipGetLastError());
  uint32_t found = 0;
  HIP_OK_E(e, hipMemcpyAsync(&found, d_count, sizeof found, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  if (found > n) {
    e->error = std::string(call) + ": more band records than slots";
    return 90;
  }
  out->resize(found);
  if (found) {
    HIP_OK_E(e, hipMemcpyAsync(out->data(), d_rec, (size_t)found * sizeof(PairsBandRec), hipMemcpyDeviceToHost, e->stream));
    HIP_OK_E(e, hipStreamSynchronize(e->stream));
  }
  return 0;
}

// the edges of local tile k of a mesh behind which another tile lies (bit d: CS_DIR_XLO, XHI, YLO, YHI)
uint32_t mesh_tile_edges(const cs_mesh* m, size_t k) {
  uint32_t edges = 0;
  for (int d = 0; d < 4; ++d)
    if (m->neighbour(m->index_of[k], d) >= 0) edges |= 1u << d;
  return edges;
}

// The band records of every tile on every rank into `every`: [failed?], then the records as 8-byte words, in ONE gather
// of variable size.  A rank that failed (or sent nonsense) sets *err = 90 and *why = failed_text, unless an error of this
// rank's own stands there.  Non-zero: the transport failed and the mesh is poisoned.
template <class Rec>
int mesh_gather_bands(cs_mesh* m, const std::vector<std::vector<Rec>>& bands, const char* failed_text, int* err,
                      std::string* why, std::vector<Rec>* every) {
  static_assert(sizeof(Rec) % sizeof(uint64_t) == 0, "band records travel as 8-byte words");
  every->clear();
  if (!m->distributed) {
    for (const auto& b : bands) every->insert(every->end(), b.begin(), b.end());
    return 0;
  }
  std::vector<uint64_t> mine(1, *err ? 1u : 0u);
  if (!*err)
    for (const auto& b : bands) {
      const size_t at = mine.size();
      mine.resize(at + b.size() * (sizeof(Rec) / sizeof(uint64_t)));
      if (!b.empty()) std::memcpy(&mine[at], b.data(), b.size() * sizeof(Rec));
    }
  std::vector<std::vector<unsigned char>> parts;
  if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), parts)) return m->poison(rc, m->error);
  for (const auto& part : parts) {
    uint64_t failed = 1u;
    if (part.size() >= sizeof failed) std::memcpy(&failed, part.data(), sizeof failed);
    if (failed || (part.size() - sizeof(uint64_t)) % sizeof(Rec)) {
      if (!*err) {
        *err = 90;
        *why = failed_text;
      }
      continue;
    }
    const size_t k = (part.size() - sizeof(uint64_t)) / sizeof(Rec), at = every->size();
    every->resize(at + k);
    if (k) std::memcpy(&(*every)[at], part.data() + sizeof(uint64_t), k * sizeof(Rec));
  }
  return 0;
}

}  // namespace
