// cs_close_pairs.hip.inc — the pairs of agents within a distance of one another, between steps: contacts, near misses,
// overlaps (include/crowdstep_state.h, "Pairs of agents between steps").  Part of the single translation unit
// crowdstep_hip.hip (included there, after cs_near.hip.inc, which holds the walk, the band, the cross loop, the block
// helpers and the sort this file shares with cs_clusters.hip.inc and cs_neighbours.hip.inc, and says why the walk is
// conservative; it uses sel_begin of cs_select.hip.inc, which it does not change).
//
//   K_pairs_count  k_pairs_count, one lane per slot of the CELL-SORTED arrays (the call sorts first, as the spatial
//                  queries do), so the lanes of a wave stand in the same or in adjacent cells and walk nearly the same
//                  slots at the same time.  A lane rebuilds its own f64 position (the expression of
//                  cs_engine::to_global, through sel_load) and its two role bits (sel_pred) once (pairs_self), then
//                  walks (near_walk).  It takes the candidates with a LARGER device id (each unordered pair is judged
//                  once, by its smaller id); one that passed the distance test is then checked for the grid's rectangle
//                  and for its roles (near_roles).  The count leaves through pairs_block_tally.
//   K_pairs_emit   k_pairs_emit, only when listing: the same walk twice, first to count, then, at the place the
//                  workgroup took with one atomic (pairs_block_place), to write (a << 32 | b, d2).
//   sort           pairs_radix over both halves of the key with the f64 payload; the digits above the bits of the largest
//                  listed id are zero in both halves and their passes are skipped.  Ascending device id is ascending
//                  external id, so the host maps min(count, cap) pairs and does nothing else per pair.
//   mesh           k_pairs_band exports (id, x, y, role bits, tile) of the participants within reach of an edge that has
//                  a neighbour tile; k_pairs_cross_count / _emit test a tile's band against the gathered records of the
//                  tiles with a higher index (near_cross).
//
// Scratch: the count needs 256 bytes of the by-id scratch.  The pair arrays (two key arrays, two payload arrays, the
// digit histogram) go through PairsScratch.

// What a lane does on its walk: the pairs (s, q) with id_q > id_s into `out`.
template <bool EMIT>
struct PairsVisit {
  const SelGroupDev* groups;
  uint32_t sid;
  bool ra, rb;  // the roles of the lane's own agent
  PairsSink<EMIT> out;
  uint32_t idj;
  __device__ __forceinline__ bool take(const AgentArrays& a, uint32_t j) {
    idj = a.id[j];
    return idj > sid;
  }
  __device__ __forceinline__ void hit(const GridDev& g, const AgentArrays& a, const PairsArgs& P, uint32_t j, double xq,
                                      double yq, double d2) {
    if (!pairs_in_grid(P, xq, yq)) return;
    if (P.roles) {
      const uint32_t q = near_roles(g, a, j, groups, P, xq, yq, 3u);
      if (!((ra && (q & 2u)) || ((q & 1u) && rb))) return;
    }
    out.put(sid, idj, d2);
  }
};

// The walk of one lane.  EMIT: written from keys[at] on (below cap), and *top is the largest id written.  Returns the
// number of its pairs.
template <bool EMIT>
__device__ __forceinline__ uint32_t pairs_walk(const GridDev& g, const AgentArrays& a, uint32_t limit,
                                               const uint32_t* __restrict__ cell_start,
                                               const SelGroupDev* __restrict__ groups, const PairsArgs& P,
                                               const PairsSelf& s, unsigned long long at, unsigned long long cap,
                                               unsigned long long* __restrict__ keys, double* __restrict__ d2s,
                                               uint32_t* top) {
  PairsVisit<EMIT> v{groups, s.id, s.ra, s.rb, {at, cap, keys, d2s, 0u, 0u}, 0u};
  near_walk(g, a, limit, cell_start, P, s.x, s.y, s.cx, s.cy, v);
  if (EMIT) *top = v.out.top;
  return v.out.n;
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

// What a band record does with a foreign record in reach: a pair if their roles allow, the smaller id first.
template <bool EMIT>
struct PairsCrossVisit {
  PairsSink<EMIT> out;
  __device__ __forceinline__ void hit(const PairsBandRec& me, const PairsBandRec& q, double d2) {
    if (((me.bits & 1u) && (q.bits & 2u)) || ((q.bits & 1u) && (me.bits & 2u))) out.put(min(me.id, q.id), max(me.id, q.id), d2);
  }
};

// near_cross for pairs (s_f: 6 KiB).  Every lane of the workgroup calls this.
template <bool EMIT>
__device__ __forceinline__ uint32_t pairs_cross_walk(const PairsBandRec& me, bool live,
                                                     const PairsBandRec* __restrict__ foreign, uint32_t n_f, double dist2,
                                                     PairsBandRec* s_f, unsigned long long at, unsigned long long cap,
                                                     unsigned long long* __restrict__ keys, double* __restrict__ d2s,
                                                     uint32_t* top) {
  PairsCrossVisit<EMIT> v{{at, cap, keys, d2s, 0u, 0u}};
  near_cross(me, live, foreign, n_f, dist2, s_f, v);
  if (EMIT) *top = v.out.top;
  return v.out.n;
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

namespace {

// one listed pair on the host: the key (device ids, a << 32 | b) and the left-hand side
struct PairRec {
  uint64_t key;
  double d2;
};
bool operator<(const PairRec& l, const PairRec& r) { return l.key < r.key; }

// a NaN or negative distance, a selection cs_select_agents refuses, distances without pairs (3)
int pairs_check(std::string* error, double distance, const cs_selection* sa, const cs_selection* sb,
                const cs_id_pair* out_pairs, const double* out_d2) {
  if (int rc = near_check_distance(error, distance, "close_pairs")) return rc;
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

// the pair arrays in one allocation (own: one of the call's own, whatever its size)
struct PairsArrays {
  unsigned long long *keys = nullptr, *keys_other = nullptr;
  double *d2 = nullptr, *d2_other = nullptr;
  uint32_t* hist = nullptr;
};
int pairs_arrays(PairsScratch* sc, uint64_t count, bool want_d2, bool own, PairsArrays* out) {
  const size_t b_keys = sel_up((size_t)count * sizeof(uint64_t)), b_d2 = want_d2 ? b_keys : 0u;
  const size_t tiles = ((size_t)count + IDS_TILE - 1u) / IDS_TILE;
  const size_t b_hist = sel_up(IDS_RADIX * std::max<size_t>(tiles, 1u) * sizeof(uint32_t));
  unsigned char* p = static_cast<unsigned char*>(sc->get(2u * b_keys + 2u * b_d2 + b_hist + 256u, own));
  if (!p) return 90;
  out->keys = reinterpret_cast<unsigned long long*>(p);
  out->keys_other = reinterpret_cast<unsigned long long*>(p + b_keys);
  out->d2 = want_d2 ? reinterpret_cast<double*>(p + 2u * b_keys) : nullptr;
  out->d2_other = want_d2 ? reinterpret_cast<double*>(p + 2u * b_keys + b_d2) : nullptr;
  out->hist = reinterpret_cast<uint32_t*>(p + 2u * b_keys + 2u * b_d2);
  return 0;
}

// The radix passes over `count` listed pairs whose largest id is `top`, then the first `take` of them to the host.
int pairs_sort_download(cs_engine* e, PairsArrays A, uint64_t count, uint32_t top, size_t take, std::vector<PairRec>* out) {
  const uint32_t n = (uint32_t)count;  // (at most CS_PAIRS_MAX)
  for (uint32_t word = 0; word < 64u && n > 1u; word += 32u)  // b in the low half, a in the high half, both at most `top`
    if (int rc = pairs_radix(e, &A.keys, &A.keys_other, &A.d2, &A.d2_other, A.hist, n, word, pairs_bits(top))) return rc;
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

// The end of a listing of `found` pairs, after its emitting kernel: the header back, then the sort and the download.
int pairs_list_end(cs_engine* e, const unsigned long long* hdr, const PairsArrays& A, uint64_t found, size_t want,
                   std::vector<PairRec>* out) {
  unsigned long long back[3];
  if (int rc = pairs_read_header(e, hdr, back)) return rc;
  if (back[1] != found) {
    e->error = "close_pairs: the listing found another number of pairs than the count";
    return 90;
  }
  return pairs_sort_download(e, A, found, (uint32_t)back[2], want, out);
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
  hipLaunchKernelGGL(k_pairs_count, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], n, e->cell_start.get(),
                     e->sel_groups_dev.get(), P, hdr);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long found = 0;
  if (int rc = pairs_read_count(e, hdr, &found)) return rc;
  *count = found;
  if (!want || !found) return 0;
  if (found > CS_PAIRS_MAX) {
    *too_many = true;
    return 0;
  }
  PairsScratch sc(e);
  PairsArrays A;
  if (int rc = pairs_arrays(&sc, found, want_d2, false, &A)) return rc;
  hipLaunchKernelGGL(k_pairs_emit, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], n, e->cell_start.get(),
                     e->sel_groups_dev.get(), P, hdr, A.keys, A.d2, (unsigned long long)found);
  HIP_OK_E(e, hipGetLastError());
  return pairs_list_end(e, hdr, A, found, want, out);
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
  const uint32_t n = e->n_slots, edges = mesh_tile_edges(m, local);
  if (!n || !edges || !(P.dist2 > 0.0)) return 0;
  PairsScratch sc(e);
  unsigned char* p = static_cast<unsigned char*>(sc.get(256u + (size_t)n * sizeof(PairsBandRec)));
  if (!p) return 90;
  return pairs_band_run(e, P, edges, m->index_of[local], reinterpret_cast<uint32_t*>(p),
                        reinterpret_cast<PairsBandRec*>(p + 256u), nullptr, "close_pairs", out);
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
  if (int rc = pairs_read_count(e, hdr, &found)) return rc;  // (synchronised: the host records are uploaded)
  *count = found;
  if (!want || !found) return 0;
  if (found > CS_PAIRS_MAX) {
    *too_many = true;
    return 0;
  }
  // the records stay where they are: where they lie in the kept scratch, the list takes an allocation of its own
  PairsScratch sc(e);
  PairsArrays A;
  if (int rc = pairs_arrays(&sc, found, want_d2, recs.temp.get() == nullptr, &A)) return rc;
  hipLaunchKernelGGL(k_pairs_cross_emit, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, d_l, n_l, d_f, n_f, dist2, hdr, A.keys,
                     A.d2, (unsigned long long)found);
  HIP_OK_E(e, hipGetLastError());
  return pairs_list_end(e, hdr, A, found, want, out);
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
  if (near_check_mesh_distance(m, distance, "close_pairs")) return SIZE_MAX;
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
  // 2. the band records of every tile on every rank
  std::vector<PairsBandRec> every;
  if (mesh_gather_bands(m, bands, "a tile of another rank failed while listing pairs", &err, &why, &every)) return SIZE_MAX;
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
  mesh_merge_runs(all, ends);
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
    mesh_merge_runs(all, ends);
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
