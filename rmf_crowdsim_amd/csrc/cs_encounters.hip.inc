// cs_encounters.hip.inc — the pairs of agents that come within a distance of one another inside a time horizon, between
// steps: closest approach under constant velocities (include/crowdstep_state.h, "Encounters between steps").  Part of the
// single translation unit crowdstep_hip.hip (included there, after cs_near.hip.inc and the three position queries; it is
// the fourth visitor of near_walk / near_cross and the first that reads velocities in the walk and in the band records.
// It uses sel_load / sel_pred / sel_begin of cs_select.hip.inc, pairs_args, the block helpers, pairs_radix, PairsScratch
// and mesh_gather_bands of cs_near.hip.inc, pairs_too_many of cs_close_pairs.hip.inc, and changes none of them).
//
//   K_enc_count    k_encounters_count, one lane per slot of the CELL-SORTED arrays.  A lane rebuilds its own f64 position,
//                  its widened velocity and its two role bits once (enc_self: sel_load with velocities on), then walks
//                  (near_walk) with the walk's own distance test set to `range`.  It takes the candidates with a LARGER
//                  device id; one that is in range has its 8-byte velocity loaded only now, and the rule (enc_rule) is
//                  evaluated from the d2 and the rebuilt position the walk hands over; the survivors are checked for the
//                  grid's rectangle and for their roles as the pairs are.  The count leaves through pairs_block_tally.
//   K_enc_emit     k_encounters_emit, only when listing: the same walk twice, first to count, then, at the place the
//                  workgroup took with one atomic (pairs_block_place), to write (a << 32 | b, its own list index, t, m2).
//   sort           pairs_radix as it is: the 8-byte payload it moves is the row's LIST INDEX (the bits of a 64-bit integer
//                  in an f64 word, moved by loads and stores only), and k_encounters_gather fetches t and m2 by it after
//                  the sort, into the two arrays the sort no longer needs.  The existing queries launch what they did.
//   mesh           k_encounters_band exports (position, widened velocity, id, role bits, tile) of the participants within
//                  reach of an edge that has a neighbour tile, 40 bytes each; k_encounters_cross_count / _emit test a
//                  tile's band against the gathered records of the tiles with a higher index (near_cross).
//
// THE RULE is symmetric to the bit: swapping the two agents negates r, w and c exactly, so t, d2 and m2 do not depend on
// who walks and who is the candidate.  Every operation is one f64 operation (the library is built without contraction
// and without fast-math, so the division is the correctly rounded one).
//
// Scratch: the count needs 256 bytes of the by-id scratch.  A listing of n rows takes six arrays of n 8-byte words (two
// key arrays, two index arrays, t and m2) and the digit histogram, through PairsScratch.

struct EncArgs {
  double lim2;     // distance * distance
  double horizon;
};

// a band record of the mesh: a participant near a cut, with its widened velocity
struct EncBandRec {
  double x, y, vx, vy;
  uint32_t id;
  uint32_t bits;  // 1: role A, 2: role B, tile index << 2
};
static_assert(sizeof(EncBandRec) == 40, "band records travel as five 8-byte words");

// The rule for r = q - p, w = v_q - v_p (in range already): the time of closest approach within the horizon and the squared
// distance then; true: an encounter.
__device__ __forceinline__ bool enc_rule(const EncArgs& E, double rx, double ry, double wx, double wy, double* t_out,
                                         double* m2_out) {
  const double ww = wx * wx + wy * wy;
  const double rw = rx * wx + ry * wy;
  double t = 0.0;
  if (rw < 0.0) {
    t = -rw / ww;
    if (!(t < E.horizon)) t = E.horizon;
  }
  const double cx = rx + wx * t, cy = ry + wy * t;
  const double m2 = cx * cx + cy * cy;
  *t_out = t;
  *m2_out = m2;
  return m2 < E.lim2;
}

// what a lane knows of its own agent
struct EncSelf {
  double x, y, vx, vy;
  uint32_t id, cx, cy;
  bool ra, rb;
};

// Slot i as a party to encounters (pairs_self with the velocity kept); false: no live (owned) agent, not a participant, or
// of neither role.
__device__ __forceinline__ bool enc_self(const GridDev& g, const AgentArrays& a, uint32_t i, uint32_t limit,
                                         const SelGroupDev* __restrict__ groups, const PairsArgs& P, EncSelf* s) {
  SelAgent ag;
  if (!sel_load(g, a, i, limit, P.owned_only, groups, P.n_groups, P.off_x, P.off_y, P.cell_size, true, &ag)) return false;
  if (!pairs_in_grid(P, ag.x, ag.y)) return false;
  s->ra = !(P.roles & 1u) || sel_pred(P.a, ag.x, ag.y, ag.vx, ag.vy, ag.wp, ag.g.sink, ag.g.hlp, ag.g.lp);
  s->rb = !(P.roles & 2u) || sel_pred(P.b, ag.x, ag.y, ag.vx, ag.vy, ag.wp, ag.g.sink, ag.g.hlp, ag.g.lp);
  if (!(s->ra || s->rb)) return false;
  const uint32_t c = a.cell[i];
  s->cx = c / g.nx;
  s->cy = c - s->cx * g.nx;
  s->x = ag.x;
  s->y = ag.y;
  s->vx = ag.vx;
  s->vy = ag.vy;
  s->id = a.id[i];
  return true;
}

// What a counting or a listing walk gathers: n rows; EMIT: row k of the lane goes to list place at + k (below cap) with
// that place as its payload, and top is raised to the largest id written.
template <bool EMIT>
struct EncSink {
  unsigned long long at, cap;
  unsigned long long* __restrict__ keys;
  double* __restrict__ index;
  double* __restrict__ ts;
  double* __restrict__ m2s;
  uint32_t n, top;
  __device__ __forceinline__ void put(uint32_t lo_id, uint32_t hi_id, double t, double m2) {
    if (EMIT) {
      const unsigned long long k = at + n;
      if (k < cap) {
        keys[k] = ((unsigned long long)lo_id << 32) | hi_id;
        index[k] = __longlong_as_double((long long)k);
        ts[k] = t;
        m2s[k] = m2;
      }
      top = max(top, hi_id);
    }
    ++n;
  }
};

// What a lane does on its walk: the encounters (s, q) with id_q > id_s into `out`.
template <bool EMIT>
struct EncVisit {
  const SelGroupDev* groups;
  EncArgs E;
  double sx, sy, svx, svy;
  uint32_t sid;
  bool ra, rb;  // the roles of the lane's own agent
  EncSink<EMIT> out;
  uint32_t idj;
  __device__ __forceinline__ bool take(const AgentArrays& a, uint32_t j) {
    idj = a.id[j];
    return idj > sid;
  }
  __device__ __forceinline__ void hit(const GridDev& g, const AgentArrays& a, const PairsArgs& P, uint32_t j, double xq,
                                      double yq, double d2) {
    const float2 vq = a.vel[j];
    double t, m2;
    if (!enc_rule(E, xq - sx, yq - sy, (double)vq.x - svx, (double)vq.y - svy, &t, &m2)) return;
    if (!pairs_in_grid(P, xq, yq)) return;
    if (P.roles) {
      const uint32_t q = near_roles(g, a, j, groups, P, xq, yq, 3u);
      if (!((ra && (q & 2u)) || ((q & 1u) && rb))) return;
    }
    out.put(sid, idj, t, m2);
  }
};

template <bool EMIT>
__device__ __forceinline__ uint32_t enc_walk(const GridDev& g, const AgentArrays& a, uint32_t limit,
                                             const uint32_t* __restrict__ cell_start,
                                             const SelGroupDev* __restrict__ groups, const PairsArgs& P, const EncArgs& E,
                                             const EncSelf& s, unsigned long long at, unsigned long long cap,
                                             unsigned long long* __restrict__ keys, double* __restrict__ index,
                                             double* __restrict__ ts, double* __restrict__ m2s, uint32_t* top) {
  EncVisit<EMIT> v{groups, E, s.x, s.y, s.vx, s.vy, s.id, s.ra, s.rb, {at, cap, keys, index, ts, m2s, 0u, 0u}, 0u};
  near_walk(g, a, limit, cell_start, P, s.x, s.y, s.cx, s.cy, v);
  if (EMIT) *top = v.out.top;
  return v.out.n;
}

// K_enc_count.  hdr[0] += the encounters (starts at 0).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_encounters_count(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                       const SelGroupDev* __restrict__ groups, PairsArgs P, EncArgs E,
                       unsigned long long* __restrict__ hdr) {
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);  // the sorted arrays hold the live agents in front
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  EncSelf s;
  uint32_t n = 0;
  if (enc_self(g, a, i, limit, groups, P, &s))
    n = enc_walk<false>(g, a, limit, cell_start, groups, P, E, s, 0ull, 0ull, nullptr, nullptr, nullptr, nullptr, nullptr);
  pairs_block_tally(n, &hdr[0]);
}

// K_enc_emit.  hdr[1]: the cursor of the list (starts at 0), the low word of hdr[2]: the largest id listed.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_encounters_emit(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                      const SelGroupDev* __restrict__ groups, PairsArgs P, EncArgs E, unsigned long long* __restrict__ hdr,
                      unsigned long long* __restrict__ keys, double* __restrict__ index, double* __restrict__ ts,
                      double* __restrict__ m2s, unsigned long long cap) {
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  EncSelf s;
  const bool live = enc_self(g, a, i, limit, groups, P, &s);
  uint32_t n = 0;
  if (live)
    n = enc_walk<false>(g, a, limit, cell_start, groups, P, E, s, 0ull, 0ull, nullptr, nullptr, nullptr, nullptr, nullptr);
  const unsigned long long at = pairs_block_place(n, &hdr[1]);
  uint32_t top = 0;
  if (live && n) enc_walk<true>(g, a, limit, cell_start, groups, P, E, s, at, cap, keys, index, ts, m2s, &top);
  pairs_block_top(top, reinterpret_cast<uint32_t*>(&hdr[2]));
}

// After the sort: row k of the sorted list was written at list place index[k]; its t and m2 from there.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_encounters_gather(const double* __restrict__ index, const double* __restrict__ ts, const double* __restrict__ m2s,
                        uint32_t n_rows, uint32_t n_list, double* __restrict__ t_out, double* __restrict__ m2_out) {
  const uint32_t k = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  if (k >= n_rows) return;
  const unsigned long long from = (unsigned long long)__double_as_longlong(index[k]);
  if (from >= n_list) return;  // (cannot happen: the payloads are the places 0 .. n_list - 1)
  t_out[k] = ts[from];
  m2_out[k] = m2s[from];
}

// The band of a tile for the encounters: k_pairs_band with the velocity in the record.  Records beyond cap are dropped
// (the host gives room for every slot).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_encounters_band(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                      const SelGroupDev* __restrict__ groups, PairsArgs P, uint32_t edges, uint32_t tile_index,
                      EncBandRec* __restrict__ out, uint32_t cap, uint32_t* __restrict__ count) {
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  EncSelf s;
  const bool hit = enc_self(g, a, i, limit, groups, P, &s) && near_in_band(g, P.reach, edges, s.cx, s.cy);
  const uint32_t at = near_wave_place(hit, count);
  if (at >= cap) return;  // (NEAR_NO_PLACE is beyond every cap)
  EncBandRec r;
  r.x = s.x;
  r.y = s.y;
  r.vx = s.vx;
  r.vy = s.vy;
  r.id = s.id;
  r.bits = (s.ra ? 1u : 0u) | (s.rb ? 2u : 0u) | (tile_index << 2);
  out[at] = r;
}

// What a band record does with a foreign record in range: an encounter if the rule and their roles say so, the smaller id
// first.
template <bool EMIT>
struct EncCrossVisit {
  EncArgs E;
  EncSink<EMIT> out;
  __device__ __forceinline__ void hit(const EncBandRec& me, const EncBandRec& q, double d2) {
    if (!(((me.bits & 1u) && (q.bits & 2u)) || ((q.bits & 1u) && (me.bits & 2u)))) return;
    double t, m2;
    if (!enc_rule(E, q.x - me.x, q.y - me.y, q.vx - me.vx, q.vy - me.vy, &t, &m2)) return;
    out.put(min(me.id, q.id), max(me.id, q.id), t, m2);
  }
};

// near_cross for encounters (s_f: 10 KiB).  Every lane of the workgroup calls this.
template <bool EMIT>
__device__ __forceinline__ uint32_t enc_cross_walk(const EncBandRec& me, bool live, const EncBandRec* __restrict__ foreign,
                                                   uint32_t n_f, double range2, const EncArgs& E, EncBandRec* s_f,
                                                   unsigned long long at, unsigned long long cap,
                                                   unsigned long long* __restrict__ keys, double* __restrict__ index,
                                                   double* __restrict__ ts, double* __restrict__ m2s, uint32_t* top) {
  EncCrossVisit<EMIT> v{E, {at, cap, keys, index, ts, m2s, 0u, 0u}};
  near_cross(me, live, foreign, n_f, range2, s_f, v);
  if (EMIT) *top = v.out.top;
  return v.out.n;
}

__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_encounters_cross_count(const EncBandRec* __restrict__ local, uint32_t n_l, const EncBandRec* __restrict__ foreign,
                             uint32_t n_f, double range2, EncArgs E, unsigned long long* __restrict__ hdr) {
  __shared__ EncBandRec s_f[PAIRS_BLOCK];
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const bool live = i < n_l;
  EncBandRec me = {};
  if (live) me = local[i];
  const uint32_t n = enc_cross_walk<false>(me, live, foreign, n_f, range2, E, s_f, 0ull, 0ull, nullptr, nullptr, nullptr,
                                           nullptr, nullptr);
  pairs_block_tally(n, &hdr[0]);
}

__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_encounters_cross_emit(const EncBandRec* __restrict__ local, uint32_t n_l, const EncBandRec* __restrict__ foreign,
                            uint32_t n_f, double range2, EncArgs E, unsigned long long* __restrict__ hdr,
                            unsigned long long* __restrict__ keys, double* __restrict__ index, double* __restrict__ ts,
                            double* __restrict__ m2s, unsigned long long cap) {
  __shared__ EncBandRec s_f[PAIRS_BLOCK];
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const bool live = i < n_l;
  EncBandRec me = {};
  if (live) me = local[i];
  const uint32_t n = enc_cross_walk<false>(me, live, foreign, n_f, range2, E, s_f, 0ull, 0ull, nullptr, nullptr, nullptr,
                                           nullptr, nullptr);
  const unsigned long long at = pairs_block_place(n, &hdr[1]);
  uint32_t top = 0;
  enc_cross_walk<true>(me, live && n, foreign, n_f, range2, E, s_f, at, cap, keys, index, ts, m2s, &top);
  pairs_block_top(top, reinterpret_cast<uint32_t*>(&hdr[2]));
}

namespace {

// one listed encounter on the host: the key (device ids, a << 32 | b), the time and the squared distance then
struct EncRec {
  uint64_t key;
  double t, m2;
};
bool operator<(const EncRec& l, const EncRec& r) { return l.key < r.key; }

// a NaN or negative distance, horizon or range, a selection cs_select_agents refuses (3)
int enc_check(std::string* error, double distance, double horizon, double range, const cs_selection* sa,
              const cs_selection* sb) {
  if (int rc = near_check_distance(error, distance, "encounters")) return rc;
  if (!(horizon >= 0.0)) {
    *error = "encounters: the horizon is NaN or negative";
    return 3;
  }
  if (!(range >= 0.0)) {
    *error = "encounters: the range is NaN or negative";
    return 3;
  }
  if (sa)
    if (int rc = sel_check(error, sa, "encounters")) return rc;
  if (sb)
    if (int rc = sel_check(error, sb, "encounters")) return rc;
  return 0;
}

// the arrays of a listing in one allocation (own: one of the call's own, whatever its size)
struct EncArrays {
  unsigned long long *keys = nullptr, *keys_other = nullptr;
  double *index = nullptr, *index_other = nullptr, *t = nullptr, *m2 = nullptr;
  uint32_t* hist = nullptr;
};
int enc_arrays(PairsScratch* sc, uint64_t count, bool own, EncArrays* out) {
  const size_t b = sel_up((size_t)count * sizeof(uint64_t));
  const size_t tiles = ((size_t)count + IDS_TILE - 1u) / IDS_TILE;
  const size_t b_hist = sel_up(IDS_RADIX * std::max<size_t>(tiles, 1u) * sizeof(uint32_t));
  unsigned char* p = static_cast<unsigned char*>(sc->get(6u * b + b_hist + 256u, own));
  if (!p) return 90;
  out->keys = reinterpret_cast<unsigned long long*>(p);
  out->keys_other = reinterpret_cast<unsigned long long*>(p + b);
  out->index = reinterpret_cast<double*>(p + 2u * b);
  out->index_other = reinterpret_cast<double*>(p + 3u * b);
  out->t = reinterpret_cast<double*>(p + 4u * b);
  out->m2 = reinterpret_cast<double*>(p + 5u * b);
  out->hist = reinterpret_cast<uint32_t*>(p + 6u * b);
  return 0;
}

// The end of a listing of `found` rows, after its emitting kernel: the header back, the radix passes over both halves of
// the key with the list index as the payload, the gather of t and m2 of the first `want` rows into the two arrays the sort
// is done with, and their download.
int enc_list_end(cs_engine* e, const unsigned long long* hdr, EncArrays A, uint64_t found, size_t want,
                 std::vector<EncRec>* out) {
  unsigned long long back[3];
  if (int rc = pairs_read_header(e, hdr, back)) return rc;
  if (back[1] != found) {
    e->error = "encounters: the listing found another number of encounters than the count";
    return 90;
  }
  const uint32_t n = (uint32_t)found;  // (at most CS_PAIRS_MAX)
  const uint32_t top = (uint32_t)back[2];
  for (uint32_t word = 0; word < 64u && n > 1u; word += 32u)  // b in the low half, a in the high half, both at most `top`
    if (int rc = pairs_radix(e, &A.keys, &A.keys_other, &A.index, &A.index_other, A.hist, n, word, pairs_bits(top))) return rc;
  const uint32_t take = (uint32_t)std::min<size_t>(want, n);
  double* t_sorted = reinterpret_cast<double*>(A.keys_other);
  double* m2_sorted = A.index_other;
  std::vector<uint64_t> keys(take);
  std::vector<double> t(take), m2(take);
  if (take) {
    hipLaunchKernelGGL(k_encounters_gather, dim3((take + PAIRS_BLOCK - 1u) / PAIRS_BLOCK), dim3(PAIRS_BLOCK), 0, e->stream,
                       A.index, A.t, A.m2, take, n, t_sorted, m2_sorted);
    HIP_OK_E(e, hipGetLastError());
    HIP_OK_E(e, hipMemcpyAsync(keys.data(), A.keys, take * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK_E(e, hipMemcpyAsync(t.data(), t_sorted, take * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK_E(e, hipMemcpyAsync(m2.data(), m2_sorted, take * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  }
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  out->resize(take);
  for (size_t k = 0; k < take; ++k) (*out)[k] = EncRec{keys[k], t[k], m2[k]};
  return 0;
}

// The encounters among the agents one engine holds (after sel_begin): *count = all of them; with want > 0 the first
// min(*count, want) of them in `out`, ascending, as device ids, unless *count is above CS_PAIRS_MAX (*too_many).
// One memset, one kernel and one read back for the count; for the list one more kernel, one read back, three launches
// per 4 bits of the largest id and half of the key, one gather, one download.
int enc_run(cs_engine* e, const PairsArgs& P, const EncArgs& E, size_t want, std::vector<EncRec>* out, uint64_t* count,
            bool* too_many) {
  out->clear();
  *count = 0;
  *too_many = false;
  if (int rc = e->refresh_counts()) return rc;
  if (int rc = e->ensure_index()) return rc;
  const uint32_t n = e->n_slots;
  if (!n || !(P.dist2 > 0.0) || !(E.lim2 > 0.0)) return 0;  // (range or distance 0: the comparisons are strict)
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  const uint32_t blocks = (n + PAIRS_BLOCK - 1u) / PAIRS_BLOCK;
  hipLaunchKernelGGL(k_encounters_count, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], n,
                     e->cell_start.get(), e->sel_groups_dev.get(), P, E, hdr);
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
  EncArrays A;
  if (int rc = enc_arrays(&sc, found, false, &A)) return rc;
  hipLaunchKernelGGL(k_encounters_emit, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], n,
                     e->cell_start.get(), e->sel_groups_dev.get(), P, E, hdr, A.keys, A.index, A.t, A.m2, (unsigned long long)found);
  HIP_OK_E(e, hipGetLastError());
  return enc_list_end(e, hdr, A, found, want, out);
}

int enc_too_many(std::string* error) {
  *error = "encounters: too many encounters to list (more than CS_PAIRS_MAX = 67108864); the count-only form has no limit";
  return 3;
}

// device ids -> external ids, into the caller's rows
void enc_copy_out(const cs_engine* ids_of, const std::vector<EncRec>& list, cs_encounter* out, size_t cap) {
  const size_t k = std::min(list.size(), cap);
  for (size_t i = 0; i < k; ++i) {
    out[i].a = ids_of->ext_id(list[i].key >> 32);
    out[i].b = ids_of->ext_id(list[i].key & 0xFFFFFFFFull);
    out[i].t = list[i].t;
    out[i].d2 = list[i].m2;
  }
}

// The band of one tile of a mesh (after enc_run on it: sorted) to the host.  One memset, one kernel, one read back, one
// download.
int enc_band_export(cs_mesh* m, size_t local, const PairsArgs& P, const EncArgs& E, std::vector<EncBandRec>* out) {
  cs_engine* e = m->tiles[local];
  out->clear();
  const uint32_t n = e->n_slots, edges = mesh_tile_edges(m, local);
  if (!n || !edges || !(P.dist2 > 0.0) || !(E.lim2 > 0.0)) return 0;
  PairsScratch sc(e);
  unsigned char* p = static_cast<unsigned char*>(sc.get(256u + (size_t)n * sizeof(EncBandRec)));
  if (!p) return 90;
  uint32_t* d_count = reinterpret_cast<uint32_t*>(p);
  EncBandRec* d_rec = reinterpret_cast<EncBandRec*>(p + 256u);
  HIP_OK_E(e, hipMemsetAsync(d_count, 0, sizeof(uint32_t), e->stream));
  hipLaunchKernelGGL(k_encounters_band, dim3((n + PAIRS_BLOCK - 1u) / PAIRS_BLOCK), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev,
                     e->buf[e->cur], n, e->cell_start.get(), e->sel_groups_dev.get(), P, edges, m->index_of[local], d_rec, n, d_count);
  HIP_OK_E(e, hipGetLastError());
  uint32_t found = 0;
  HIP_OK_E(e, hipMemcpyAsync(&found, d_count, sizeof found, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  if (found > n) {
    e->error = "encounters: more band records than slots";
    return 90;
  }
  out->resize(found);
  if (found) {
    HIP_OK_E(e, hipMemcpyAsync(out->data(), d_rec, (size_t)found * sizeof(EncBandRec), hipMemcpyDeviceToHost, e->stream));
    HIP_OK_E(e, hipStreamSynchronize(e->stream));
  }
  return 0;
}

// The encounters between the band of one local tile and the records of the tiles with a higher index, on that tile's
// device.
int enc_cross(cs_engine* e, const std::vector<EncBandRec>& local, const std::vector<EncBandRec>& foreign, double range2,
              const EncArgs& E, size_t want, std::vector<EncRec>* out, uint64_t* count, bool* too_many) {
  out->clear();
  *count = 0;
  *too_many = false;
  if (local.empty() || foreign.empty()) return 0;
  const uint32_t n_l = (uint32_t)local.size(), n_f = (uint32_t)foreign.size();
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  PairsScratch recs(e);
  const size_t b_l = sel_up((size_t)n_l * sizeof(EncBandRec)), b_f = sel_up((size_t)n_f * sizeof(EncBandRec));
  unsigned char* p = static_cast<unsigned char*>(recs.get(b_l + b_f));
  if (!p) return 90;
  EncBandRec* d_l = reinterpret_cast<EncBandRec*>(p);
  EncBandRec* d_f = reinterpret_cast<EncBandRec*>(p + b_l);
  HIP_OK_E(e, hipMemcpyAsync(d_l, local.data(), (size_t)n_l * sizeof(EncBandRec), hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(d_f, foreign.data(), (size_t)n_f * sizeof(EncBandRec), hipMemcpyHostToDevice, e->stream));
  const uint32_t blocks = (n_l + PAIRS_BLOCK - 1u) / PAIRS_BLOCK;
  hipLaunchKernelGGL(k_encounters_cross_count, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, d_l, n_l, d_f, n_f, range2, E,
                     hdr);
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
  EncArrays A;
  if (int rc = enc_arrays(&sc, found, recs.temp.get() == nullptr, &A)) return rc;
  hipLaunchKernelGGL(k_encounters_cross_emit, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, d_l, n_l, d_f, n_f, range2, E,
                     hdr, A.keys, A.index, A.t, A.m2, (unsigned long long)found);
  HIP_OK_E(e, hipGetLastError());
  return enc_list_end(e, hdr, A, found, want, out);
}

}  // namespace

extern "C" {

size_t cs_encounters(cs_engine* e, double distance, double horizon, double range, const cs_selection* sel_a,
                     const cs_selection* sel_b, cs_encounter* out, size_t cap) {
  if (!e) return SIZE_MAX;
  hipSetDevice(e->device);
  if (enc_check(&e->error, distance, horizon, range, sel_a, sel_b)) return SIZE_MAX;
  if (sel_begin(e)) return SIZE_MAX;
  const size_t want = out ? cap : 0u;
  const PairsArgs P = pairs_args(e, range, sel_a, sel_b);
  const EncArgs E{distance * distance, horizon};
  std::vector<EncRec> list;
  uint64_t count = 0;
  bool too_many = false;
  if (enc_run(e, P, E, want, &list, &count, &too_many)) return SIZE_MAX;
  if (too_many) {
    enc_too_many(&e->error);
    return SIZE_MAX;
  }
  if (want) enc_copy_out(e, list, out, cap);
  return (size_t)count;
}

// Collective: two gathers of variable size (two collectives each), whatever the crowd and the answer.  The first carries
// every rank's band records, the second its rows (the count-only form: its counts).
size_t cs_mesh_encounters(cs_mesh* m, double distance, double horizon, double range, const cs_selection* sel_a,
                          const cs_selection* sel_b, cs_encounter* out, size_t cap) {
  if (!m) return SIZE_MAX;
  if (m->dead()) return SIZE_MAX;
  if (enc_check(&m->error, distance, horizon, range, sel_a, sel_b)) return SIZE_MAX;
  if (near_check_mesh_distance(m, range, "encounters")) return SIZE_MAX;
  if (cs_mesh_synchronize(m)) return SIZE_MAX;
  hipSetDevice(m->device);
  const size_t want = out ? cap : 0u;
  const EncArgs E{distance * distance, horizon};
  const double range2 = range * range;
  int err = 0;
  bool too_many = false;
  std::string why;
  uint64_t total = 0;
  std::vector<EncRec> all;  // the sorted runs, one behind the other
  std::vector<size_t> ends;
  std::vector<std::vector<EncBandRec>> bands(m->tiles.size());
  // 1. every tile: the encounters among the agents it holds, and its band
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    cs_engine* e = m->tiles[k];
    std::vector<EncRec> part;
    uint64_t c = 0;
    bool many = false;
    if (!err) err = sel_begin(e);
    const PairsArgs P = pairs_args(e, range, sel_a, sel_b);
    if (!err) err = enc_run(e, P, E, want, &part, &c, &many);
    if (!err && m->n_tiles() > 1u) err = enc_band_export(m, k, P, E, &bands[k]);
    if (err && why.empty()) why = cs_last_error(e);
    too_many = too_many || many;
    total += c;
    all.insert(all.end(), part.begin(), part.end());
    ends.push_back(all.size());
  }
  // 2. the band records of every tile on every rank
  std::vector<EncBandRec> every;
  if (mesh_gather_bands(m, bands, "a tile of another rank failed while listing encounters", &err, &why, &every))
    return SIZE_MAX;
  // 3. every local tile's band against the records of the tiles with a higher index: each cross-tile pair once
  for (size_t k = 0; k < m->tiles.size() && !err; ++k) {
    const uint32_t index = m->index_of[k];
    std::vector<EncBandRec> foreign;
    for (const EncBandRec& r : every)
      if ((r.bits >> 2) > index) foreign.push_back(r);
    std::vector<EncRec> part;
    uint64_t c = 0;
    bool many = false;
    err = enc_cross(m->tiles[k], bands[k], foreign, range2, E, want, &part, &c, &many);
    if (err && why.empty()) why = cs_last_error(m->tiles[k]);
    too_many = too_many || many;
    total += c;
    all.insert(all.end(), part.begin(), part.end());
    ends.push_back(all.size());
  }
  mesh_merge_runs(all, ends);
  if (all.size() > want) all.resize(want);
  // 4. the rows (or only the counts) of every rank: [0 ok / 1 failed / 2 too many, count, n listed, keys, t, m2]
  if (m->distributed) {
    std::vector<uint64_t> mine{err ? 1u : (too_many ? 2u : 0u), total, (err || too_many) ? 0u : all.size()};
    if (mine[2]) {
      const size_t n = all.size();
      mine.resize(3u + 3u * n);
      for (size_t i = 0; i < n; ++i) {
        mine[3u + i] = all[i].key;
        std::memcpy(&mine[3u + n + i], &all[i].t, sizeof(double));
        std::memcpy(&mine[3u + 2u * n + i], &all[i].m2, sizeof(double));
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
      if (words < 3u || w[0] == 1u || words != 3u + 3u * w[2]) {
        if (!err) {
          err = 90;
          why = "a tile of another rank failed while listing encounters";
        }
        continue;
      }
      if (w[0] == 2u) too_many = true;
      total += w[1];
      const size_t n = (size_t)w[2];
      for (size_t i = 0; i < n; ++i) {
        EncRec r;
        r.key = w[3u + i];
        std::memcpy(&r.t, &w[3u + n + i], sizeof(double));
        std::memcpy(&r.m2, &w[3u + 2u * n + i], sizeof(double));
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
    enc_too_many(&m->error);
    return SIZE_MAX;
  }
  if (want && !m->tiles.empty()) enc_copy_out(m->tiles[0], all, out, cap);
  return (size_t)total;
}

}  // extern "C"
