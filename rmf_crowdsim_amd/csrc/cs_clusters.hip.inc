// cs_clusters.hip.inc — which agents hang together, between steps: the connected components of the graph cs_close_pairs
// defines (include/crowdstep_state.h, "Clusters of agents between steps").  Part of the single translation unit
// crowdstep_hip.hip (included there, after cs_close_pairs.hip.inc; it uses the walk, the band, the cross loop, the block
// helpers, PairsScratch and the sort of cs_near.hip.inc and pairs_sort_download of cs_close_pairs.hip.inc, none of which
// it changes).
//
//   K_init     k_clusters_init, one lane per slot of the CELL-SORTED arrays: parent[slot] = slot for a member (pairs_self
//              with both roles set to `members`), CLU_NONE for everybody else.  Membership is judged once, here; every
//              later kernel reads it from parent[].
//   K_link     k_clusters_link, one lane per slot: near_walk; for every candidate in reach with a LARGER device id that
//              is a member it unites the two trees: find both roots (path halving), hook the HIGHER root slot under the
//              lower with one atomicCAS, and on a lost race find again.
//   why it ends  parent[s] <= s always: K_init writes s, a hook writes a lower root into a root, halving writes an
//              ancestor (lower still).  So every find walks strictly downwards, and every retry of a hook starts from a
//              root that just got a lower parent: both loops end, whatever the other lanes do.  No lane waits for another:
//              there is no flag, no spinning, no grid-wide barrier, and the host sees no "changed" word: ONE launch links
//              a chain of any length.
//   K_flatten  k_clusters_flatten, a launch of its own: parent[slot] = the root.
//   K_label    k_clusters_label: the smallest device id and the number of members per root.  Ascending device id is
//              ascending external id.  The lanes of a wave are neighbours in cell order and mostly share a root: what
//              shares a root is reduced in the wave by shuffles first, then ONE atomicMin and ONE atomicAdd per distinct
//              root and wave.
//   K_tally    k_clusters_tally: the reported clusters (size >= min_size), their members and the largest label, one atomic
//              each per workgroup.  The count-only form ends here.
//   K_rank     k_clusters_rank: a row per reported cluster, in no order, and its sort key (label << 32 | row).
//   K_stats    k_clusters_stats: box and f64 sums per row, reduced per root in the wave like K_label, then one f64
//              atomicMin / atomicMax / atomicAdd each per distinct root and wave; a cluster of one writes its row plainly.
//   K_members  k_clusters_members: (id << 32 | label) of every member of a reported cluster, one atomic per workgroup.
//   sort       pairs_radix over the HIGH word of the keys; k_clusters_gather brings the rows into label order; only the
//              first `cap` entries of either list are downloaded.
//   mesh       k_clusters_band exports (position, id, local label, tile) of the members in the band; k_clusters_cross_*
//              find the links between a tile's band and the records of higher tiles (near_cross) and emit (local label,
//              foreign label); k_clusters_relabel applies the merged label map to the member keys a tile holds.
//
// Scratch: 16 bytes per slot (parent, smallest id, size, row) plus, when listing, 64 + 16 bytes per reported cluster and
// 16 per reported member, through PairsScratch: in cs_engine::pairs_scratch while at most PAIRS_SCRATCH_KEEP bytes, else
// allocated for the call and freed before it returns.

#define CLU_NONE 0xFFFFFFFFu

// a band record of the mesh: a member near a cut, with the label its own tile gave it
struct ClusterBandRec {
  double x, y;
  uint32_t id, tile, label, pad;
};
static_assert(sizeof(ClusterBandRec) == 32, "band records travel as four 8-byte words");
static_assert(sizeof(cs_cluster) == 64, "cs_cluster is eight 8-byte words");

__device__ __forceinline__ uint32_t clu_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void clu_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, halving the path on the way.  Every step goes to a strictly lower slot (parent[s] <= s).
__device__ __forceinline__ uint32_t clu_find(uint32_t* __restrict__ parent, uint32_t x) {
  for (;;) {
    const uint32_t p = clu_load(&parent[x]);
    if (p == x) return x;
    const uint32_t gp = clu_load(&parent[p]);
    if (gp != p) clu_store(&parent[x], gp);  // (an ancestor of x: still below x)
    x = gp;
  }
}

// One tree of the trees of a and b.  A lost hook means the higher root got a lower parent meanwhile: find again.
__device__ __forceinline__ void clu_unite(uint32_t* __restrict__ parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = clu_find(parent, a);
    b = clu_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&parent[a], a, b) == a) return;
  }
}

// the f64 position of slot i, the expression of cs_engine::to_global (as sel_load and near_walk compute it)
__device__ __forceinline__ void clu_position(const GridDev& g, const AgentArrays& a, uint32_t i, const PairsArgs& P, double* x,
                                             double* y) {
  const uint32_t c = a.cell[i];
  const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
  const float2 off = a.off[i];
  *x = P.off_x + ((double)((uint64_t)g.org_x + cx) * P.cell_size + (double)off.x);
  *y = P.off_y + ((double)((uint64_t)g.org_y + cy) * P.cell_size + (double)off.y);
}

// K_init.  parent has n_ub entries.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_init(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                    const SelGroupDev* __restrict__ groups, PairsArgs P, uint32_t* __restrict__ parent) {
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  if (i >= n_ub) return;
  PairsSelf s;
  parent[i] = pairs_self(g, a, i, limit, groups, P, &s) ? i : CLU_NONE;
}

// What a member does on its walk: one tree with every member in reach that has a larger id.
struct ClustersLink {
  uint32_t* parent;
  uint32_t i, sid;
  __device__ __forceinline__ bool take(const AgentArrays& a, uint32_t j) { return a.id[j] > sid; }
  __device__ __forceinline__ void hit(const GridDev&, const AgentArrays&, const PairsArgs&, uint32_t j, double, double, double) {
    if (clu_load(&parent[j]) != CLU_NONE) clu_unite(parent, i, j);  // (not a member: it links nobody)
  }
};

// K_link.  A candidate's membership is its parent[] entry.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_link(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start, PairsArgs P,
                    uint32_t* __restrict__ parent) {
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  if (i >= limit || clu_load(&parent[i]) == CLU_NONE) return;
  double sx, sy;
  clu_position(g, a, i, P, &sx, &sy);
  ClustersLink v{parent, i, a.id[i]};
  const uint32_t c = a.cell[i];
  const uint32_t scx = c / g.nx, scy = c - scx * g.nx;
  near_walk(g, a, limit, cell_start, P, sx, sy, scx, scy, v);
}

// K_flatten.
__global__ void __launch_bounds__(PAIRS_BLOCK) k_clusters_flatten(uint32_t* __restrict__ parent, uint32_t n) {
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t x = clu_load(&parent[i]);
  if (x == CLU_NONE || x == i) return;
  for (;;) {
    const uint32_t p = clu_load(&parent[x]);
    if (p == x) break;
    x = p;
  }
  clu_store(&parent[i], x);
}

__device__ __forceinline__ uint32_t clu_wave_min(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ double clu_shfl_xor(double v, int d) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = __shfl_xor((uint32_t)u, d, 64), hi = __shfl_xor((uint32_t)(u >> 32), d, 64);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// K_label.  min_id[] starts at CLU_NONE, size[] at 0; both are indexed by root slot.  Every lane of a wave runs the loop.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_label(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ parent, uint32_t n,
                     uint32_t* __restrict__ min_id, uint32_t* __restrict__ size) {
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const uint32_t root = i < n ? parent[i] : CLU_NONE;
  const bool member = root != CLU_NONE;
  const uint32_t id = member ? ids[i] : CLU_NONE;
  const uint32_t lane = __lane_id();
  unsigned long long todo = __ballot(member);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t r = __shfl(root, leader, 64);
    const bool mine = member && root == r;
    const unsigned long long same = __ballot(mine);
    const uint32_t count = (uint32_t)__popcll(same);
    uint32_t low = id;
    if (count > 1u) low = clu_wave_min(mine ? id : CLU_NONE);
    if ((int)lane == leader) {
      atomicMin(&min_id[r], low);
      atomicAdd(&size[r], count);
    }
    todo &= ~same;
  }
}

// K_tally.  hdr[0] += the reported clusters, hdr[1] += their members, the low word of hdr[2]: the largest label.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_tally(const uint32_t* __restrict__ parent, uint32_t n, const uint32_t* __restrict__ min_id,
                     const uint32_t* __restrict__ size, unsigned long long min_size, unsigned long long* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const bool hit = i < n && parent[i] == i && (unsigned long long)size[i] >= min_size;
  pairs_block_tally(hit ? 1u : 0u, &hdr[0]);
  __shared__ unsigned long long s_members[PAIRS_WAVES];
  const unsigned long long w = pairs_wave_sum(hit ? size[i] : 0u);
  if (__lane_id() == 0u) s_members[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0u) {
    unsigned long long t = 0;
    for (uint32_t k = 0; k < PAIRS_WAVES; ++k) t += s_members[k];
    if (t) atomicAdd(&hdr[1], t);
  }
  pairs_block_top(hit ? min_id[i] + 1u : 0u, reinterpret_cast<uint32_t*>(&hdr[2]));  // (+ 1: label 0 counts, too)
}

// K_rank.  hdr[3]: the cursor of the rows (starts at 0).  row_of[root] = the row of a reported cluster, CLU_NONE otherwise.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_rank(const uint32_t* __restrict__ parent, uint32_t n, const uint32_t* __restrict__ min_id,
                    const uint32_t* __restrict__ size, unsigned long long min_size, unsigned long long* __restrict__ hdr,
                    uint32_t* __restrict__ row_of, cs_cluster* __restrict__ rows, unsigned long long* __restrict__ keys,
                    unsigned long long cap) {
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const bool root = i < n && parent[i] == i;
  const bool hit = root && (unsigned long long)size[i] >= min_size;
  const unsigned long long at = pairs_block_place(hit ? 1u : 0u, &hdr[3]);
  if (i >= n) return;
  row_of[i] = (hit && at < cap) ? (uint32_t)at : CLU_NONE;
  if (!hit || at >= cap) return;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  cs_cluster c;
  c.label = min_id[i];
  c.size = size[i];
  c.min_x = inf;
  c.min_y = inf;
  c.max_x = -inf;
  c.max_y = -inf;
  c.sum_x = 0.0;
  c.sum_y = 0.0;
  rows[at] = c;
  keys[at] = ((unsigned long long)min_id[i] << 32) | (unsigned long long)at;
}

// K_stats.  Every lane of a wave runs the loop.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_stats(GridDev g, AgentArrays a, uint32_t n, PairsArgs P, const uint32_t* __restrict__ parent,
                     const uint32_t* __restrict__ row_of, cs_cluster* __restrict__ rows) {
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const uint32_t root = i < n ? parent[i] : CLU_NONE;
  const uint32_t row = root != CLU_NONE ? row_of[root] : CLU_NONE;
  const bool member = row != CLU_NONE;
  double x = 0.0, y = 0.0;
  if (member) clu_position(g, a, i, P, &x, &y);
  const uint32_t lane = __lane_id();
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  unsigned long long todo = __ballot(member);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t r = __shfl(row, leader, 64);
    const bool mine = member && row == r;
    const unsigned long long same = __ballot(mine);
    todo &= ~same;
    if (__popcll(same) == 1) {  // (the same for the whole wave)
      if ((int)lane == leader) {
        cs_cluster* c = &rows[r];
        if (c->size == 1u) {  // a cluster of one: its position, exactly
          c->min_x = x;
          c->max_x = x;
          c->sum_x = 0.0 + x;
          c->min_y = y;
          c->max_y = y;
          c->sum_y = 0.0 + y;
        } else {
          atomicMin(&c->min_x, x);
          atomicMin(&c->min_y, y);
          atomicMax(&c->max_x, x);
          atomicMax(&c->max_y, y);
          atomicAdd(&c->sum_x, x);
          atomicAdd(&c->sum_y, y);
        }
      }
      continue;
    }
    double lx = mine ? x : inf, ly = mine ? y : inf, hx = mine ? x : -inf, hy = mine ? y : -inf;
    double sx = mine ? x : 0.0, sy = mine ? y : 0.0;
    for (int d = 32; d >= 1; d >>= 1) {
      lx = fmin(lx, clu_shfl_xor(lx, d));
      ly = fmin(ly, clu_shfl_xor(ly, d));
      hx = fmax(hx, clu_shfl_xor(hx, d));
      hy = fmax(hy, clu_shfl_xor(hy, d));
      sx += clu_shfl_xor(sx, d);
      sy += clu_shfl_xor(sy, d);
    }
    if ((int)lane == leader) {
      cs_cluster* c = &rows[r];
      atomicMin(&c->min_x, lx);
      atomicMin(&c->min_y, ly);
      atomicMax(&c->max_x, hx);
      atomicMax(&c->max_y, hy);
      atomicAdd(&c->sum_x, sx);
      atomicAdd(&c->sum_y, sy);
    }
  }
}

// K_members.  hdr[4]: the cursor of the list (starts at 0), the low word of hdr[5]: the largest id listed (+ 1).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_members(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ parent, uint32_t n,
                       const uint32_t* __restrict__ min_id, const uint32_t* __restrict__ size, unsigned long long min_size,
                       unsigned long long* __restrict__ hdr, unsigned long long* __restrict__ keys, unsigned long long cap) {
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const uint32_t root = i < n ? parent[i] : CLU_NONE;
  const bool hit = root != CLU_NONE && (unsigned long long)size[root] >= min_size;
  const unsigned long long at = pairs_block_place(hit ? 1u : 0u, &hdr[4]);
  const uint32_t id = hit ? ids[i] : 0u;
  pairs_block_top(hit ? id + 1u : 0u, reinterpret_cast<uint32_t*>(&hdr[5]));
  if (hit && at < cap) keys[at] = ((unsigned long long)id << 32) | (unsigned long long)min_id[root];
}

// the rows in the order of the sorted keys (label << 32 | row)
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_gather(const unsigned long long* __restrict__ keys, const cs_cluster* __restrict__ rows,
                      cs_cluster* __restrict__ out, uint32_t take) {
  const uint32_t k = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  if (k < take) out[k] = rows[(uint32_t)keys[k]];
}

// The band of a tile (near_in_band): the members in it, with the label of their cluster on this tile.  Records beyond cap
// are dropped (the host gives room for all).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_band(GridDev g, AgentArrays a, uint32_t n, PairsArgs P, const uint32_t* __restrict__ parent,
                    const uint32_t* __restrict__ min_id, uint32_t edges, uint32_t tile_index,
                    ClusterBandRec* __restrict__ out, uint32_t cap, uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const uint32_t root = i < n ? parent[i] : CLU_NONE;
  bool hit = root != CLU_NONE;
  if (hit) {
    const uint32_t c = a.cell[i];
    const uint32_t cx = c / g.nx;
    hit = near_in_band(g, P.reach, edges, cx, c - cx * g.nx);
  }
  const uint32_t at = near_wave_place(hit, count);
  if (at >= cap) return;  // (NEAR_NO_PLACE is beyond every cap)
  ClusterBandRec r;
  clu_position(g, a, i, P, &r.x, &r.y);
  r.id = a.id[i];
  r.tile = tile_index;
  r.label = min_id[root];
  r.pad = 0u;
  out[at] = r;
}

// What a band record does with a foreign record in reach: a link, the key (local label << 32 | foreign label).
template <bool EMIT>
struct ClustersCrossVisit {
  PairsSink<EMIT> out;
  __device__ __forceinline__ void hit(const ClusterBandRec& me, const ClusterBandRec& q, double d2) {
    out.put(me.label, q.label, d2);
  }
};

// near_cross for clusters (s_f: 8 KiB).  Every lane of the workgroup calls this.
template <bool EMIT>
__device__ __forceinline__ uint32_t clusters_cross_walk(const ClusterBandRec& me, bool live,
                                                        const ClusterBandRec* __restrict__ foreign, uint32_t n_f,
                                                        double dist2, ClusterBandRec* s_f, unsigned long long at,
                                                        unsigned long long cap, unsigned long long* __restrict__ keys,
                                                        uint32_t* top) {
  ClustersCrossVisit<EMIT> v{{at, cap, keys, nullptr, 0u, 0u}};
  near_cross(me, live, foreign, n_f, dist2, s_f, v);
  if (EMIT) *top = v.out.top;
  return v.out.n;
}

__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_cross_count(const ClusterBandRec* __restrict__ local, uint32_t n_l, const ClusterBandRec* __restrict__ foreign,
                           uint32_t n_f, double dist2, unsigned long long* __restrict__ hdr) {
  __shared__ ClusterBandRec s_f[PAIRS_BLOCK];
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const bool live = i < n_l;
  ClusterBandRec me = {};
  if (live) me = local[i];
  const uint32_t n = clusters_cross_walk<false>(me, live, foreign, n_f, dist2, s_f, 0ull, 0ull, nullptr, nullptr);
  pairs_block_tally(n, &hdr[0]);
}

__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_cross_emit(const ClusterBandRec* __restrict__ local, uint32_t n_l, const ClusterBandRec* __restrict__ foreign,
                          uint32_t n_f, double dist2, unsigned long long* __restrict__ hdr,
                          unsigned long long* __restrict__ keys, unsigned long long cap) {
  __shared__ ClusterBandRec s_f[PAIRS_BLOCK];
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const bool live = i < n_l;
  ClusterBandRec me = {};
  if (live) me = local[i];
  const uint32_t n = clusters_cross_walk<false>(me, live, foreign, n_f, dist2, s_f, 0ull, 0ull, nullptr, nullptr);
  const unsigned long long at = pairs_block_place(n, &hdr[1]);
  uint32_t top = 0;
  clusters_cross_walk<true>(me, live && n, foreign, n_f, dist2, s_f, at, cap, keys, &top);
  pairs_block_top(top, reinterpret_cast<uint32_t*>(&hdr[2]));
}

// The label map of the mesh applied to the member keys a tile holds: the low word of a key that is in `from` (ascending)
// becomes the entry of `to` at the same place.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_clusters_relabel(unsigned long long* __restrict__ keys, uint32_t n, const uint32_t* __restrict__ from,
                       const uint32_t* __restrict__ to, uint32_t n_map) {
  const uint32_t k = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  if (k >= n) return;
  const unsigned long long key = keys[k];
  const uint32_t label = (uint32_t)key;
  uint32_t lo = 0, hi = n_map;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (from[mid] < label) lo = mid + 1u;
    else hi = mid;
  }
  if (lo < n_map && from[lo] == label) keys[k] = (key & 0xFFFFFFFF00000000ull) | to[lo];
}

namespace {

// a NaN or negative distance, a selection cs_select_agents refuses, labels without ids (3)
int clusters_check(std::string* error, double distance, const cs_selection* members, const uint64_t* out_ids,
                   const uint64_t* out_labels) {
  if (int rc = near_check_distance(error, distance, "agent_clusters")) return rc;
  if (members)
    if (int rc = sel_check(error, members, "agent_clusters")) return rc;
  if (out_labels && !out_ids) {
    *error = "agent_clusters: out_labels without out_ids";
    return 3;
  }
  return 0;
}

// The scratch of one call: a first block through PairsScratch (the kept scratch while it fits), later blocks behind it
// while there is room, else allocated for the call and freed when this goes out of scope.
struct ClustersArena {
  PairsScratch sc;
  unsigned char* base = nullptr;
  size_t used = 0, room = 0;
  std::vector<DevBytes> extra;
  explicit ClustersArena(cs_engine* e) : sc(e) {}
  ~ClustersArena() {
    if (!extra.empty()) hipStreamSynchronize(sc.e->stream);  // (then `extra` frees them)
  }
  // `first` bytes now; `wish`: what the call may need in all (asked for at once while that keeps it in the kept scratch)
  int open(size_t first, size_t wish) {
    size_t need = first;
    if (first <= PAIRS_SCRATCH_KEEP) need = std::max(first, std::min<size_t>(PAIRS_SCRATCH_KEEP, wish));
    base = static_cast<unsigned char*>(sc.get(need));
    if (!base) return 90;
    room = need;
    return 0;
  }
  // room for `bytes` more in ONE block
  int reserve(size_t bytes) {
    if (used + bytes <= room) return 0;
    DevBytes q;
    if (q.alloc(bytes) != hipSuccess) {
      sc.e->error = "agent_clusters: out of device memory";
      return 90;
    }
    base = static_cast<unsigned char*>(q.get());
    extra.push_back(std::move(q));
    used = 0;
    room = bytes;
    return 0;
  }
  unsigned char* take(size_t bytes) {  // (after open / reserve gave room)
    unsigned char* p = base + used;
    used += sel_up(bytes);
    return p;
  }
};

size_t clusters_hist_bytes(size_t count) {
  return sel_up(IDS_RADIX * std::max<size_t>((count + IDS_TILE - 1u) / IDS_TILE, 1u) * sizeof(uint32_t));
}

// The radix passes over the HIGH word of n keys, the largest of which is `top`.  *keys is the sorted array afterwards.
int clusters_sort(cs_engine* e, unsigned long long** keys, unsigned long long** other, uint32_t* hist, uint32_t n,
                  uint32_t top) {
  if (n < 2u) return 0;
  return pairs_radix(e, keys, other, nullptr, nullptr, hist, n, 32u, pairs_bits(top));
}

// what one engine answers, in DEVICE ids: members as (id << 32 | label) ascending, rows ascending by label
struct ClustersOut {
  uint64_t n_agents = 0, n_clusters = 0;
  std::vector<uint64_t> members;
  std::vector<cs_cluster> rows;
};

// mesh: the sorted member keys of a tile stay on its device until the label map is applied
struct ClustersHold {
  cs_engine* e = nullptr;
  DevBytes mem;
  unsigned long long* keys = nullptr;
  uint32_t n = 0;
  ~ClustersHold() {
    if (mem.get()) hipStreamSynchronize(e->stream);  // (then `mem` frees it)
  }
};

// The clusters among the agents one engine holds (after sel_begin).  The counts always; with want_ids / want_rows > 0 the
// first min(count, want) members / rows.  hold: the member keys stay on the device instead (all of them).  band (mesh):
// the band of the tile with these edges, exported while the labels are on the device.
int clusters_run(cs_engine* e, const PairsArgs& P, uint64_t min_size, size_t want_ids, size_t want_rows, ClustersOut* out,
                 ClustersHold* hold, uint32_t edges, uint32_t tile_index, std::vector<ClusterBandRec>* band) {
  *out = ClustersOut();
  if (band) band->clear();
  if (int rc = e->refresh_counts()) return rc;
  if (int rc = e->ensure_index()) return rc;
  const uint32_t n = e->n_slots;
  if (!n) return 0;
  const bool want_band = band && edges && P.dist2 > 0.0;
  const size_t b_col = sel_up((size_t)n * sizeof(uint32_t));
  const size_t b_band = want_band ? 256u + sel_up((size_t)n * sizeof(ClusterBandRec)) : 0u;
  const size_t first = 256u + 4u * b_col + b_band;
  const size_t b_keys = sel_up((size_t)n * sizeof(uint64_t));
  const size_t most = sel_up((size_t)n * sizeof(cs_cluster)) * 2u + 4u * b_keys + 2u * clusters_hist_bytes(n);
  ClustersArena A(e);
  if (int rc = A.open(first, first + most)) return rc;
  unsigned long long* hdr = reinterpret_cast<unsigned long long*>(A.take(256u));
  uint32_t* parent = reinterpret_cast<uint32_t*>(A.take(b_col));
  uint32_t* min_id = reinterpret_cast<uint32_t*>(A.take(b_col));
  uint32_t* size = reinterpret_cast<uint32_t*>(A.take(b_col));
  uint32_t* row_of = reinterpret_cast<uint32_t*>(A.take(b_col));
  uint32_t* band_count = nullptr;
  ClusterBandRec* band_rec = nullptr;
  if (want_band) {
    band_count = reinterpret_cast<uint32_t*>(A.take(256u));
    band_rec = reinterpret_cast<ClusterBandRec*>(A.take((size_t)n * sizeof(ClusterBandRec)));
  }
  const uint32_t blocks = (n + PAIRS_BLOCK - 1u) / PAIRS_BLOCK;
  const dim3 grid(blocks), block(PAIRS_BLOCK);
  HIP_OK_E(e, hipMemsetAsync(hdr, 0, 256u, e->stream));
  HIP_OK_E(e, hipMemsetAsync(min_id, 0xFF, (size_t)n * sizeof(uint32_t), e->stream));
  HIP_OK_E(e, hipMemsetAsync(size, 0, (size_t)n * sizeof(uint32_t), e->stream));
  hipLaunchKernelGGL(k_clusters_init, grid, block, 0, e->stream, e->gdev, e->buf[e->cur], n, e->cell_start.get(), e->sel_groups_dev.get(), P,
                     parent);
  if (P.dist2 > 0.0) {  // (distance 0: the comparison is strict, every member is its own cluster)
    hipLaunchKernelGGL(k_clusters_link, grid, block, 0, e->stream, e->gdev, e->buf[e->cur], n, e->cell_start.get(), P, parent);
    hipLaunchKernelGGL(k_clusters_flatten, grid, block, 0, e->stream, parent, n);
  }
  hipLaunchKernelGGL(k_clusters_label, grid, block, 0, e->stream, e->buf[e->cur].id, parent, n, min_id, size);
  hipLaunchKernelGGL(k_clusters_tally, grid, block, 0, e->stream, parent, n, min_id, size, (unsigned long long)min_size, hdr);
  if (want_band) {
    HIP_OK_E(e, hipMemsetAsync(band_count, 0, sizeof(uint32_t), e->stream));
    hipLaunchKernelGGL(k_clusters_band, grid, block, 0, e->stream, e->gdev, e->buf[e->cur], n, P, parent, min_id, edges, tile_index,
                       band_rec, n, band_count);
  }
  HIP_OK_E(e, hipGetLastError());
  unsigned long long back[3] = {0, 0, 0};
  uint32_t n_band = 0;
  HIP_OK_E(e, hipMemcpyAsync(back, hdr, sizeof back, hipMemcpyDeviceToHost, e->stream));
  if (want_band) HIP_OK_E(e, hipMemcpyAsync(&n_band, band_count, sizeof n_band, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  if (back[0] > n || back[1] > n || n_band > n) {
    e->error = "agent_clusters: more clusters, members or band records than slots";
    return 90;
  }
  out->n_clusters = back[0];
  out->n_agents = back[1];
  if (n_band) {
    band->resize(n_band);
    HIP_OK_E(e, hipMemcpyAsync(band->data(), band_rec, (size_t)n_band * sizeof(ClusterBandRec), hipMemcpyDeviceToHost,
                               e->stream));
    HIP_OK_E(e, hipStreamSynchronize(e->stream));
  }
  const uint32_t nc = (uint32_t)back[0], na = (uint32_t)back[1];
  const uint32_t top_label = (uint32_t)back[2] ? (uint32_t)back[2] - 1u : 0u;
  const bool list_rows = want_rows && nc, list_ids = (want_ids || hold) && na;
  if (!list_rows && !list_ids) return 0;
  const size_t b_rows = sel_up((size_t)nc * sizeof(cs_cluster)), b_ck = sel_up((size_t)nc * sizeof(uint64_t));
  const size_t b_mk = sel_up((size_t)na * sizeof(uint64_t));
  const size_t need_rows = list_rows ? 2u * b_rows + 2u * b_ck + clusters_hist_bytes(nc) : 0u;
  const size_t need_ids = list_ids ? 2u * b_mk + clusters_hist_bytes(na) : 0u;
  if (int rc = A.reserve(need_rows + (hold ? 0u : need_ids))) return rc;
  if (list_rows) {
    cs_cluster* rows = reinterpret_cast<cs_cluster*>(A.take(b_rows));
    cs_cluster* sorted = reinterpret_cast<cs_cluster*>(A.take(b_rows));
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(A.take(b_ck));
    unsigned long long* other = reinterpret_cast<unsigned long long*>(A.take(b_ck));
    uint32_t* hist = reinterpret_cast<uint32_t*>(A.take(clusters_hist_bytes(nc)));
    hipLaunchKernelGGL(k_clusters_rank, grid, block, 0, e->stream, parent, n, min_id, size, (unsigned long long)min_size, hdr,
                       row_of, rows, keys, (unsigned long long)nc);
    hipLaunchKernelGGL(k_clusters_stats, grid, block, 0, e->stream, e->gdev, e->buf[e->cur], n, P, parent, row_of, rows);
    HIP_OK_E(e, hipGetLastError());
    if (int rc = clusters_sort(e, &keys, &other, hist, nc, top_label)) return rc;
    const uint32_t take = (uint32_t)std::min<size_t>(want_rows, nc);
    hipLaunchKernelGGL(k_clusters_gather, dim3((take + PAIRS_BLOCK - 1u) / PAIRS_BLOCK), block, 0, e->stream, keys, rows, sorted,
                       take);
    HIP_OK_E(e, hipGetLastError());
    out->rows.resize(take);
    HIP_OK_E(e, hipMemcpyAsync(out->rows.data(), sorted, (size_t)take * sizeof(cs_cluster), hipMemcpyDeviceToHost, e->stream));
    unsigned long long placed = 0;
    HIP_OK_E(e, hipMemcpyAsync(&placed, &hdr[3], sizeof placed, hipMemcpyDeviceToHost, e->stream));
    HIP_OK_E(e, hipStreamSynchronize(e->stream));
    if (placed != nc) {
      e->error = "agent_clusters: the listing found another number of clusters than the count";
      return 90;
    }
  }
  if (list_ids) {
    unsigned char* p = nullptr;
    if (hold) {
      if (hold->mem.alloc(need_ids) != hipSuccess) {
        e->error = "agent_clusters: out of device memory";
        return 90;
      }
      hold->e = e;
      p = static_cast<unsigned char*>(hold->mem.get());
    } else {
      p = A.take(need_ids);
    }
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(p);
    unsigned long long* other = reinterpret_cast<unsigned long long*>(p + b_mk);
    uint32_t* hist = reinterpret_cast<uint32_t*>(p + 2u * b_mk);
    hipLaunchKernelGGL(k_clusters_members, grid, block, 0, e->stream, e->buf[e->cur].id, parent, n, min_id, size,
                       (unsigned long long)min_size, hdr, keys, (unsigned long long)na);
    HIP_OK_E(e, hipGetLastError());
    unsigned long long placed[2] = {0, 0};
    HIP_OK_E(e, hipMemcpyAsync(placed, &hdr[4], sizeof placed, hipMemcpyDeviceToHost, e->stream));
    HIP_OK_E(e, hipStreamSynchronize(e->stream));
    if (placed[0] != na) {
      e->error = "agent_clusters: the listing found another number of members than the count";
      return 90;
    }
    const uint32_t top_id = (uint32_t)placed[1] ? (uint32_t)placed[1] - 1u : 0u;
    if (int rc = clusters_sort(e, &keys, &other, hist, na, top_id)) return rc;
    if (hold) {
      hold->keys = keys;
      hold->n = na;
      HIP_OK_E(e, hipStreamSynchronize(e->stream));
    } else {
      const size_t take = std::min<size_t>(want_ids, na);
      out->members.resize(take);
      HIP_OK_E(e, hipMemcpyAsync(out->members.data(), keys, take * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
      HIP_OK_E(e, hipStreamSynchronize(e->stream));
    }
  }
  return 0;
}

// device ids -> external ids, into the caller's arrays and counts
void clusters_copy_out(const cs_engine* ids_of, const ClustersOut& r, uint64_t* out_ids, uint64_t* out_labels, size_t agent_cap,
                       size_t* n_agents, cs_cluster* out_clusters, size_t cluster_cap, size_t* n_clusters) {
  if (out_ids) {
    const size_t k = std::min(r.members.size(), agent_cap);
    for (size_t i = 0; i < k; ++i) {
      out_ids[i] = ids_of->ext_id(r.members[i] >> 32);
      if (out_labels) out_labels[i] = ids_of->ext_id(r.members[i] & 0xFFFFFFFFull);
    }
  }
  if (out_clusters) {
    const size_t k = std::min(r.rows.size(), cluster_cap);
    for (size_t i = 0; i < k; ++i) {
      out_clusters[i] = r.rows[i];
      out_clusters[i].label = ids_of->ext_id(r.rows[i].label);
    }
  }
  if (n_agents) *n_agents = (size_t)r.n_agents;
  if (n_clusters) *n_clusters = (size_t)r.n_clusters;
}

// The distinct (local label << 32 | foreign label) of the links between the band of one local tile and the records of the
// tiles with a higher index, on that tile's device, ascending.
int clusters_cross(cs_engine* e, const std::vector<ClusterBandRec>& local, const std::vector<ClusterBandRec>& foreign,
                   double dist2, std::vector<uint64_t>* out) {
  out->clear();
  if (local.empty() || foreign.empty()) return 0;
  const uint32_t n_l = (uint32_t)local.size(), n_f = (uint32_t)foreign.size();
  const size_t b_l = sel_up((size_t)n_l * sizeof(ClusterBandRec)), b_f = sel_up((size_t)n_f * sizeof(ClusterBandRec));
  ClustersArena A(e);
  if (int rc = A.open(256u + b_l + b_f, 0u)) return rc;
  unsigned long long* hdr = reinterpret_cast<unsigned long long*>(A.take(256u));
  ClusterBandRec* d_l = reinterpret_cast<ClusterBandRec*>(A.take(b_l));
  ClusterBandRec* d_f = reinterpret_cast<ClusterBandRec*>(A.take(b_f));
  HIP_OK_E(e, hipMemsetAsync(hdr, 0, 256u, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(d_l, local.data(), (size_t)n_l * sizeof(ClusterBandRec), hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(d_f, foreign.data(), (size_t)n_f * sizeof(ClusterBandRec), hipMemcpyHostToDevice, e->stream));
  const uint32_t blocks = (n_l + PAIRS_BLOCK - 1u) / PAIRS_BLOCK;
  hipLaunchKernelGGL(k_clusters_cross_count, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, d_l, n_l, d_f, n_f, dist2, hdr);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long found = 0;
  if (int rc = pairs_read_count(e, hdr, &found)) return rc;
  if (!found) return 0;
  if (found > CS_PAIRS_MAX) {
    e->error = "agent_clusters: too many links across the cuts of the mesh";
    return 90;
  }
  const size_t b_keys = sel_up((size_t)found * sizeof(uint64_t));
  if (int rc = A.reserve(2u * b_keys + clusters_hist_bytes(found))) return rc;
  PairsArrays S;
  S.keys = reinterpret_cast<unsigned long long*>(A.take(b_keys));
  S.keys_other = reinterpret_cast<unsigned long long*>(A.take(b_keys));
  S.hist = reinterpret_cast<uint32_t*>(A.take(clusters_hist_bytes(found)));
  hipLaunchKernelGGL(k_clusters_cross_emit, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, d_l, n_l, d_f, n_f, dist2, hdr, S.keys,
                     (unsigned long long)found);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long back[3];
  if (int rc = pairs_read_header(e, hdr, back)) return rc;
  if (back[1] != found) {
    e->error = "agent_clusters: the listing found another number of links than the count";
    return 90;
  }
  std::vector<PairRec> list;
  if (int rc = pairs_sort_download(e, S, found, (uint32_t)back[2], (size_t)found, &list)) return rc;
  for (const PairRec& r : list)
    if (out->empty() || out->back() != r.key) out->push_back(r.key);
  return 0;
}

// the smallest label of the tree of x in a host union-find over labels (path halving)
uint32_t clusters_host_find(std::vector<uint32_t>& parent, uint32_t x) {
  while (parent[x] != x) {
    parent[x] = parent[parent[x]];
    x = parent[x];
  }
  return x;
}

}  // namespace

extern "C" {

int cs_agent_clusters(cs_engine* e, double distance, const cs_selection* members, uint64_t min_size, uint64_t* out_ids,
                      uint64_t* out_labels, size_t agent_cap, size_t* n_agents, cs_cluster* out_clusters, size_t cluster_cap,
                      size_t* n_clusters) {
  if (!e) return 3;
  hipSetDevice(e->device);
  if (int rc = clusters_check(&e->error, distance, members, out_ids, out_labels)) return rc;
  if (int rc = sel_begin(e)) return rc;
  const PairsArgs P = pairs_args(e, distance, members, members);
  ClustersOut r;
  if (int rc = clusters_run(e, P, min_size, out_ids ? agent_cap : 0u, out_clusters ? cluster_cap : 0u, &r, nullptr, 0u, 0u,
                            nullptr))
    return rc;
  clusters_copy_out(e, r, out_ids, out_labels, agent_cap, n_agents, out_clusters, cluster_cap, n_clusters);
  return 0;
}

// Collective: three gathers of variable size (two collectives each), whatever the crowd and the answer.  The first
// carries every rank's band records, the second its distinct label links, the third its part of the answer.
int cs_mesh_agent_clusters(cs_mesh* m, double distance, const cs_selection* members, uint64_t min_size, uint64_t* out_ids,
                           uint64_t* out_labels, size_t agent_cap, size_t* n_agents, cs_cluster* out_clusters,
                           size_t cluster_cap, size_t* n_clusters) {
  if (!m) return 3;
  if (m->dead()) return m->poison_rc;
  if (int rc = clusters_check(&m->error, distance, members, out_ids, out_labels)) return rc;
  if (int rc = near_check_mesh_distance(m, distance, "agent_clusters")) return rc;
  if (int rc = cs_mesh_synchronize(m)) return rc;
  hipSetDevice(m->device);
  const bool want_ids = out_ids != nullptr && agent_cap > 0u;
  const size_t n_local = m->tiles.size();
  const double dist2 = distance * distance;
  int err = 0;
  std::string why;
  // 1. every tile: all clusters among the agents it owns (rows to the host, member keys kept on the device), its band
  std::vector<ClustersOut> parts(n_local);
  std::vector<ClustersHold> holds(n_local);
  std::vector<std::vector<ClusterBandRec>> bands(n_local);
  for (size_t k = 0; k < n_local; ++k) {
    cs_engine* e = m->tiles[k];
    if (!err) err = sel_begin(e);
    const PairsArgs P = pairs_args(e, distance, members, members);
    if (!err)
      err = clusters_run(e, P, 1u, 0u, SIZE_MAX, &parts[k], want_ids ? &holds[k] : nullptr, mesh_tile_edges(m, k), m->index_of[k],
                         &bands[k]);
    if (err && why.empty()) why = cs_last_error(e);
  }
  // 2. the band records of every tile on every rank
  std::vector<ClusterBandRec> every;
  if (int rc = mesh_gather_bands(m, bands, "a tile of another rank failed while clustering agents", &err, &why, &every)) return rc;
  // 3. every local tile's band against the records of the tiles with a higher index: the distinct label links
  std::vector<uint64_t> links;
  for (size_t k = 0; k < n_local && !err; ++k) {
    std::vector<ClusterBandRec> foreign;
    for (const ClusterBandRec& r : every)
      if (r.tile > m->index_of[k]) foreign.push_back(r);
    std::vector<uint64_t> part;
    err = clusters_cross(m->tiles[k], bands[k], foreign, dist2, &part);
    if (err && why.empty()) why = cs_last_error(m->tiles[k]);
    links.insert(links.end(), part.begin(), part.end());
  }
  if (m->distributed) {
    std::vector<uint64_t> mine(1, err ? 1u : 0u);
    if (!err) mine.insert(mine.end(), links.begin(), links.end());
    std::vector<std::vector<unsigned char>> got;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), got)) return m->poison(rc, m->error);
    links.clear();
    for (const auto& part : got) {
      const size_t words = part.size() / sizeof(uint64_t);
      std::vector<uint64_t> w(words);
      if (words) std::memcpy(w.data(), part.data(), words * sizeof(uint64_t));
      if (!words || w[0]) {
        if (!err) {
          err = 90;
          why = "a tile of another rank failed while clustering agents";
        }
        continue;
      }
      links.insert(links.end(), w.begin() + 1, w.end());
    }
  }
  // 4. the same small union-find over labels on every rank: every linked label -> the smallest label of its tree
  std::vector<uint32_t> from, to;
  {
    for (uint64_t l : links) {
      from.push_back((uint32_t)(l >> 32));
      from.push_back((uint32_t)l);
    }
    std::sort(from.begin(), from.end());
    from.erase(std::unique(from.begin(), from.end()), from.end());
    std::vector<uint32_t> parent(from.size());
    for (uint32_t i = 0; i < parent.size(); ++i) parent[i] = i;
    for (uint64_t l : links) {
      uint32_t a = (uint32_t)(std::lower_bound(from.begin(), from.end(), (uint32_t)(l >> 32)) - from.begin());
      uint32_t b = (uint32_t)(std::lower_bound(from.begin(), from.end(), (uint32_t)l) - from.begin());
      a = clusters_host_find(parent, a);
      b = clusters_host_find(parent, b);
      if (a != b) parent[std::max(a, b)] = std::min(a, b);  // (`from` ascends: the lower index is the smaller label)
    }
    to.resize(from.size());
    for (uint32_t i = 0; i < parent.size(); ++i) to[i] = from[clusters_host_find(parent, i)];
  }
  auto mapped = [&](uint64_t label) {
    const auto it = std::lower_bound(from.begin(), from.end(), (uint32_t)label);
    return (it != from.end() && *it == (uint32_t)label) ? (uint64_t)to[(size_t)(it - from.begin())] : label;
  };
  // 5. the map on the device, onto the member keys every tile holds; the keys to the host
  std::vector<std::vector<uint64_t>> keys(n_local);
  for (size_t k = 0; k < n_local && !err && want_ids; ++k) {
    cs_engine* e = m->tiles[k];
    ClustersHold& h = holds[k];
    if (!h.n) continue;
    auto step = [&]() -> int {
      ClustersArena A(e);
      if (!from.empty()) {
        const size_t b_map = sel_up(from.size() * sizeof(uint32_t));
        if (int rc = A.open(2u * b_map, 0u)) return rc;
        uint32_t* d_from = reinterpret_cast<uint32_t*>(A.take(b_map));
        uint32_t* d_to = reinterpret_cast<uint32_t*>(A.take(b_map));
        HIP_OK_E(e, hipMemcpyAsync(d_from, from.data(), from.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        HIP_OK_E(e, hipMemcpyAsync(d_to, to.data(), to.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(k_clusters_relabel, dim3((h.n + PAIRS_BLOCK - 1u) / PAIRS_BLOCK), dim3(PAIRS_BLOCK), 0, e->stream, h.keys,
                           h.n, d_from, d_to, (uint32_t)from.size());
        HIP_OK_E(e, hipGetLastError());
      }
      keys[k].resize(h.n);
      HIP_OK_E(e, hipMemcpyAsync(keys[k].data(), h.keys, (size_t)h.n * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
      HIP_OK_E(e, hipStreamSynchronize(e->stream));
      return 0;
    };
    err = step();
    if (err && why.empty()) why = cs_last_error(e);
  }
  // 6. this rank's part of the answer: per tile [tile index, n rows, n keys, rows, keys]; (distributed) one gather
  struct TilePart {
    uint32_t tile;
    std::vector<cs_cluster> rows;
    std::vector<uint64_t> keys;
  };
  std::vector<TilePart> all;
  if (m->distributed) {
    std::vector<uint64_t> mine(1, err ? 1u : 0u);
    if (!err)
      for (size_t k = 0; k < n_local; ++k) {
        mine.push_back(m->index_of[k]);
        mine.push_back(parts[k].rows.size());
        mine.push_back(keys[k].size());
        const size_t at = mine.size();
        mine.resize(at + 8u * parts[k].rows.size());
        if (!parts[k].rows.empty()) std::memcpy(&mine[at], parts[k].rows.data(), parts[k].rows.size() * sizeof(cs_cluster));
        mine.insert(mine.end(), keys[k].begin(), keys[k].end());
      }
    std::vector<std::vector<unsigned char>> got;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), got)) return m->poison(rc, m->error);
    for (const auto& part : got) {
      const size_t words = part.size() / sizeof(uint64_t);
      std::vector<uint64_t> w(words);
      if (words) std::memcpy(w.data(), part.data(), words * sizeof(uint64_t));
      bool ok = words >= 1u && !w[0];
      size_t at = 1u;
      while (ok && at < words) {
        if (at + 3u > words || w[at + 1u] > words || w[at + 2u] > words || at + 3u + 8u * w[at + 1u] + w[at + 2u] > words) {
          ok = false;
          break;
        }
        TilePart t;
        t.tile = (uint32_t)w[at];
        t.rows.resize((size_t)w[at + 1u]);
        if (!t.rows.empty()) std::memcpy(t.rows.data(), &w[at + 3u], t.rows.size() * sizeof(cs_cluster));
        t.keys.assign(w.begin() + (long)(at + 3u + 8u * w[at + 1u]), w.begin() + (long)(at + 3u + 8u * w[at + 1u] + w[at + 2u]));
        at += 3u + 8u * (size_t)w[at + 1u] + (size_t)w[at + 2u];
        all.push_back(std::move(t));
      }
      if (!ok && !err) {
        err = 90;
        why = "a tile of another rank failed while clustering agents";
      }
    }
  } else {
    for (size_t k = 0; k < n_local; ++k) all.push_back(TilePart{m->index_of[k], std::move(parts[k].rows), std::move(keys[k])});
  }
  if (err) {
    m->error = why;
    return err;
  }
  // 7. the rows merged: by (mapped label, tile index); sizes add, boxes merge, sums add in tile-index order
  std::sort(all.begin(), all.end(), [](const TilePart& l, const TilePart& r) { return l.tile < r.tile; });
  std::vector<cs_cluster> rows;
  for (TilePart& t : all)
    for (cs_cluster& c : t.rows) {
      c.label = mapped(c.label);
      rows.push_back(c);
    }
  std::stable_sort(rows.begin(), rows.end(), [](const cs_cluster& l, const cs_cluster& r) { return l.label < r.label; });
  std::vector<cs_cluster> merged;
  for (const cs_cluster& c : rows) {
    if (!merged.empty() && merged.back().label == c.label) {
      cs_cluster& d = merged.back();
      d.size += c.size;
      d.min_x = std::min(d.min_x, c.min_x);
      d.min_y = std::min(d.min_y, c.min_y);
      d.max_x = std::max(d.max_x, c.max_x);
      d.max_y = std::max(d.max_y, c.max_y);
      d.sum_x += c.sum_x;
      d.sum_y += c.sum_y;
    } else {
      merged.push_back(c);
    }
  }
  ClustersOut r;
  for (const cs_cluster& c : merged)
    if (c.size >= min_size) {
      r.n_clusters += 1u;
      r.n_agents += c.size;
      if (out_clusters && r.rows.size() < cluster_cap) r.rows.push_back(c);
    }
  // 8. the members of the reported clusters, ascending by id
  if (want_ids) {
    std::vector<uint64_t> ids;
    std::vector<size_t> ends;
    for (const TilePart& t : all) {
      ids.insert(ids.end(), t.keys.begin(), t.keys.end());
      ends.push_back(ids.size());
    }
    mesh_merge_runs(ids, ends);  // (ids are distinct, so the keys ascend by id)
    for (uint64_t key : ids) {
      if (r.members.size() >= agent_cap) break;
      if (min_size > 1u) {
        const uint64_t label = key & 0xFFFFFFFFull;
        const auto it = std::lower_bound(merged.begin(), merged.end(), label,
                                         [](const cs_cluster& c, uint64_t l) { return c.label < l; });
        if (it == merged.end() || it->label != label || it->size < min_size) continue;
      }
      r.members.push_back(key);
    }
  }
  if (!m->tiles.empty())
    clusters_copy_out(m->tiles[0], r, out_ids, out_labels, agent_cap, n_agents, out_clusters, cluster_cap, n_clusters);
  else {
    if (n_agents) *n_agents = 0;
    if (n_clusters) *n_clusters = 0;
  }
  return 0;
}

}  // extern "C"
