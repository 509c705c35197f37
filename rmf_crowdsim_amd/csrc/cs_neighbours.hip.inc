// cs_neighbours.hip.inc — what surrounds each agent, between steps: how many others stand within a distance of it and
// which of them is the closest (include/crowdstep_state.h, "Neighbours of each agent between steps").  Part of the single
// translation unit crowdstep_hip.hip (included there, after cs_clusters.hip.inc; it uses the walk, the band, the cross
// loop, the block helpers and PairsScratch of cs_near.hip.inc and clusters_sort of cs_clusters.hip.inc, none of which it
// changes).
//
//   K_neighbours   k_neighbours<FORM>, one lane per slot of the CELL-SORTED arrays.  pairs_self judges the lane's own
//                  agent with role A = subjects and role B = others; only a subject goes on.  It walks (near_walk)
//                  over ALL candidate slots j != i: the statistic is per subject, so nothing is judged "once per pair".
//                  A candidate that passes the distance test is then checked for the grid's rectangle and, only then,
//                  for the others role (near_roles).  A hit raises the lane's count and replaces (best d2, best id)
//                  when (d2, id) is lexicographically smaller, so the row does not depend on the order of the walk.
//   forms          NEIGH_COUNT  the number of subjects with count >= min_count: summed over the wave by shuffles, over
//                               the workgroup in LDS, ONE 64-bit atomic per workgroup (pairs_block_tally); no row exists.
//                  NEIGH_LIST   the workgroup takes its place in the list with one atomic (pairs_block_place) and writes
//                               a key (id << 32 | row) and the 24-byte row (count, nearest, d2).
//                  NEIGH_STAGE  (mesh) every slot writes its subject id (or none) and its row at its own slot, for the
//                               merge with what lies behind the cuts; k_neighbours_report applies min_count afterwards.
//   order          the radix passes over the id word of the keys (clusters_sort), then k_neighbours_gather writes the
//                  first min(count, cap) rows as cs_neighbour_stat in key order.  The host maps id and nearest to
//                  external ids and does nothing else per row.
//   mesh           k_pairs_band, which here also notes the slot of every record, exports (id, x, y, role bits, tile) of
//                  the participants in the band (bit 0 a subject, bit 1 an other); k_neighbours_cross tests a tile's
//                  band SUBJECTS against the gathered band OTHERS of every other tile (near_cross) and merges count and
//                  (d2, id) into the subject's staged row: one lane owns one subject, so the merge needs no atomic.
//
// Scratch: the count-only form needs 256 bytes of the by-id scratch.  The listing (two key arrays, the rows, the ordered
// rows, the digit histogram: at most 72 bytes per slot) goes through PairsScratch: kept in cs_engine::pairs_scratch
// while it needs at most PAIRS_SCRATCH_KEEP bytes, else allocated for the call and freed before it returns.  On a mesh
// the staged rows and the band of a tile live in an allocation of the call's own.

#define NEIGH_COUNT 0
#define NEIGH_LIST 1
#define NEIGH_STAGE 2
#define NEIGH_NONE 0xFFFFFFFFu

// the payload of a subject: what cs_neighbour_stat holds beside the id, in device ids
struct NeighRow {
  unsigned long long count;
  unsigned long long nearest;  // CS_NO_NEIGHBOUR when count == 0
  double d2;                   // +inf when count == 0
};
static_assert(sizeof(NeighRow) == 24, "a row is three 8-byte words");
static_assert(sizeof(cs_neighbour_stat) == 32, "cs_neighbour_stat is four 8-byte words");

// what a lane gathers on its walk
struct NeighStat {
  uint32_t count, best;
  double d2;
};

__device__ __forceinline__ NeighStat neigh_none() { return NeighStat{0u, NEIGH_NONE, __builtin_inf()}; }

__device__ __forceinline__ void neigh_take(NeighStat* st, double d2, uint32_t id) {
  ++st->count;
  if (d2 < st->d2 || (d2 == st->d2 && id < st->best)) {
    st->d2 = d2;
    st->best = id;
  }
}

__device__ __forceinline__ NeighRow neigh_row(const NeighStat& st) {
  NeighRow r;
  r.count = st.count;
  r.nearest = st.count ? (unsigned long long)st.best : CS_NO_NEIGHBOUR;
  r.d2 = st.d2;
  return r;
}

// What a subject in slot i does on its walk: every other q != s in reach that is inside the grid and an other.
struct NeighVisit {
  const SelGroupDev* groups;
  uint32_t i;
  NeighStat* st;
  __device__ __forceinline__ bool take(const AgentArrays&, uint32_t j) { return j != i; }
  __device__ __forceinline__ void hit(const GridDev& g, const AgentArrays& a, const PairsArgs& P, uint32_t j, double xq,
                                      double yq, double d2) {
    if (!pairs_in_grid(P, xq, yq)) return;
    if (!P.roles || (near_roles(g, a, j, groups, P, xq, yq, 2u) & 2u)) neigh_take(st, d2, a.id[j]);
  }
};

// K_neighbours.  NEIGH_COUNT: hdr[0] += the reported subjects.  NEIGH_LIST: hdr[1] is the cursor of the list, the low
// word of hdr[2] the largest id listed; keys and rows have room for `cap` entries (the host gives one per slot).
// NEIGH_STAGE: stage_id and rows have n_ub entries, indexed by slot.
template <int FORM>
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_neighbours(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                 const SelGroupDev* __restrict__ groups, PairsArgs P, unsigned long long min_count,
                 unsigned long long* __restrict__ hdr, unsigned long long* __restrict__ keys, NeighRow* __restrict__ rows,
                 uint32_t* __restrict__ stage_id, uint32_t cap) {
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);  // the sorted arrays hold the live agents in front
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  PairsSelf s;
  const bool subject = pairs_self(g, a, i, limit, groups, P, &s) && s.ra;
  NeighStat st = neigh_none();
  NeighVisit v{groups, i, &st};
  if (subject && P.dist2 > 0.0) near_walk(g, a, limit, cell_start, P, s.x, s.y, s.cx, s.cy, v);  // (distance 0: strict)
  if (FORM == NEIGH_STAGE) {
    if (i < n_ub) {
      stage_id[i] = subject ? s.id : NEIGH_NONE;
      rows[i] = neigh_row(st);
    }
    return;
  }
  const bool hit = subject && (unsigned long long)st.count >= min_count;
  if (FORM == NEIGH_COUNT) {
    pairs_block_tally(hit ? 1u : 0u, &hdr[0]);
  } else {
    const unsigned long long at = pairs_block_place(hit ? 1u : 0u, &hdr[1]);
    pairs_block_top(hit ? s.id : 0u, reinterpret_cast<uint32_t*>(&hdr[2]));
    if (hit && at < cap) {
      keys[at] = ((unsigned long long)s.id << 32) | at;
      rows[at] = neigh_row(st);
    }
  }
}

// K_report (mesh, after the merge): min_count on the staged rows.  LIST: the key of a reported subject is
// (id << 32 | slot), its row stays where it is.
template <bool LIST>
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_neighbours_report(const uint32_t* __restrict__ stage_id, const NeighRow* __restrict__ rows, uint32_t n,
                        unsigned long long min_count, unsigned long long* __restrict__ hdr,
                        unsigned long long* __restrict__ keys, uint32_t cap) {
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  const uint32_t id = i < n ? stage_id[i] : NEIGH_NONE;
  const bool hit = id != NEIGH_NONE && rows[i].count >= min_count;
  if (!LIST) {
    pairs_block_tally(hit ? 1u : 0u, &hdr[0]);
  } else {
    const unsigned long long at = pairs_block_place(hit ? 1u : 0u, &hdr[1]);
    pairs_block_top(hit ? id : 0u, reinterpret_cast<uint32_t*>(&hdr[2]));
    if (hit && at < cap) keys[at] = ((unsigned long long)id << 32) | i;
  }
}

// the rows in the order of the sorted keys (id << 32 | row), as cs_neighbour_stat in device ids
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_neighbours_gather(const unsigned long long* __restrict__ keys, const NeighRow* __restrict__ rows,
                        cs_neighbour_stat* __restrict__ out, uint32_t take) {
  const uint32_t k = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  if (k >= take) return;
  const unsigned long long key = keys[k];
  const NeighRow r = rows[(uint32_t)key];
  cs_neighbour_stat o;
  o.id = key >> 32;
  o.count = r.count;
  o.nearest = r.nearest;
  o.nearest_d2 = r.d2;
  out[k] = o;
}

// What a band subject does with a foreign record in reach: the others among them count.
struct NeighCrossVisit {
  NeighStat* st;
  __device__ __forceinline__ void hit(const PairsBandRec&, const PairsBandRec& q, double d2) {
    if (q.bits & 2u) neigh_take(st, d2, q.id);
  }
};

// One lane per band record of the local tile; the subjects among them against the n_f foreign OTHERS (records of other
// tiles with bit 1, chosen by the host) through near_cross (s_f: 6 KiB).  What a subject finds is merged into its
// staged row: its slot is this lane's alone.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_neighbours_cross(const PairsBandRec* __restrict__ local, const uint32_t* __restrict__ local_slot, uint32_t n_l,
                       const PairsBandRec* __restrict__ foreign, uint32_t n_f, double dist2, NeighRow* __restrict__ rows,
                       uint32_t n_rows) {
  __shared__ PairsBandRec s_f[PAIRS_BLOCK];
  const uint32_t i = blockIdx.x * PAIRS_BLOCK + threadIdx.x;
  PairsBandRec me = {};
  if (i < n_l) me = local[i];
  const bool live = i < n_l && (me.bits & 1u);
  NeighStat st = neigh_none();
  NeighCrossVisit v{&st};
  near_cross(me, live, foreign, n_f, dist2, s_f, v);
  if (!live || !st.count) return;
  const uint32_t slot = local_slot[i];
  if (slot >= n_rows) return;
  NeighRow r = rows[slot];
  r.count += st.count;
  if (st.d2 < r.d2 || (st.d2 == r.d2 && (unsigned long long)st.best < r.nearest)) {
    r.d2 = st.d2;
    r.nearest = st.best;
  }
  rows[slot] = r;
}

namespace {

// a NaN or negative distance, a selection cs_select_agents refuses (3)
int neigh_check(std::string* error, double distance, const cs_selection* subjects, const cs_selection* others) {
  if (int rc = near_check_distance(error, distance, "agent_neighbours")) return rc;
  if (subjects)
    if (int rc = sel_check(error, subjects, "agent_neighbours")) return rc;
  if (others)
    if (int rc = sel_check(error, others, "agent_neighbours")) return rc;
  return 0;
}

bool neigh_by_id(const cs_neighbour_stat& l, const cs_neighbour_stat& r) { return l.id < r.id; }

// the arrays of one listing over n slots, in one allocation through PairsScratch
struct NeighArrays {
  unsigned long long *keys = nullptr, *keys_other = nullptr;
  NeighRow* rows = nullptr;        // null: the rows lie elsewhere (mesh: staged by slot)
  cs_neighbour_stat* out = nullptr;
  uint32_t* hist = nullptr;
};
int neigh_arrays(PairsScratch* sc, uint32_t n, size_t want, bool with_rows, NeighArrays* A) {
  const size_t b_keys = sel_up((size_t)n * sizeof(uint64_t));
  const size_t b_rows = with_rows ? sel_up((size_t)n * sizeof(NeighRow)) : 0u;
  const size_t b_out = sel_up(std::min<size_t>(n, want) * sizeof(cs_neighbour_stat));
  const size_t b_hist = clusters_hist_bytes(n);
  unsigned char* p = static_cast<unsigned char*>(sc->get(2u * b_keys + b_rows + b_out + b_hist));
  if (!p) return 90;
  A->keys = reinterpret_cast<unsigned long long*>(p);
  A->keys_other = reinterpret_cast<unsigned long long*>(p + b_keys);
  A->rows = with_rows ? reinterpret_cast<NeighRow*>(p + 2u * b_keys) : nullptr;
  A->out = reinterpret_cast<cs_neighbour_stat*>(p + 2u * b_keys + b_rows);
  A->hist = reinterpret_cast<uint32_t*>(p + 2u * b_keys + b_rows + b_out);
  return 0;
}

// The listed keys in id order, then the first min(found, want) rows to the host (device ids).
int neigh_sort_download(cs_engine* e, NeighArrays A, const NeighRow* rows, uint32_t found, uint32_t top, size_t want,
                        std::vector<cs_neighbour_stat>* out) {
  if (int rc = clusters_sort(e, &A.keys, &A.keys_other, A.hist, found, top)) return rc;
  const uint32_t take = (uint32_t)std::min<size_t>(found, want);
  out->resize(take);
  if (!take) return 0;
  hipLaunchKernelGGL(k_neighbours_gather, dim3((take + PAIRS_BLOCK - 1u) / PAIRS_BLOCK), dim3(PAIRS_BLOCK), 0, e->stream, A.keys,
                     rows, A.out, take);
  HIP_OK_E(e, hipGetLastError());
  HIP_OK_E(e, hipMemcpyAsync(out->data(), A.out, (size_t)take * sizeof(cs_neighbour_stat), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  return 0;
}

// The neighbours among the agents one engine holds (after sel_begin): *count = the reported subjects; with want > 0 the
// first min(*count, want) rows in `out`, ascending, in device ids.  The count-only form: one memset, one kernel, one read
// back.  The listing: one kernel, one read back, three launches per 4 bits of the largest id, one gather, one download.
int neigh_run(cs_engine* e, const PairsArgs& P, uint64_t min_count, size_t want, std::vector<cs_neighbour_stat>* out,
              uint64_t* count) {
  out->clear();
  *count = 0;
  if (int rc = e->refresh_counts()) return rc;
  if (int rc = e->ensure_index()) return rc;
  const uint32_t n = e->n_slots;
  if (!n) return 0;
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  const uint32_t blocks = (n + PAIRS_BLOCK - 1u) / PAIRS_BLOCK;
  if (!want) {
    hipLaunchKernelGGL(k_neighbours<NEIGH_COUNT>, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], n,
                       e->cell_start.get(), e->sel_groups_dev.get(), P, (unsigned long long)min_count, hdr, (unsigned long long*)nullptr,
                       (NeighRow*)nullptr, (uint32_t*)nullptr, 0u);
    HIP_OK_E(e, hipGetLastError());
    unsigned long long found = 0;
    const int rc = pairs_read_count(e, hdr, &found);
    *count = found;
    return rc;
  }
  PairsScratch sc(e);
  NeighArrays A;
  if (int rc = neigh_arrays(&sc, n, want, true, &A)) return rc;
  hipLaunchKernelGGL(k_neighbours<NEIGH_LIST>, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], n,
                     e->cell_start.get(), e->sel_groups_dev.get(), P, (unsigned long long)min_count, hdr, A.keys, A.rows, (uint32_t*)nullptr,
                     n);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long back[3];
  if (int rc = pairs_read_header(e, hdr, back)) return rc;
  if (back[1] > n) {
    e->error = "agent_neighbours: more rows than slots";
    return 90;
  }
  *count = back[1];
  return neigh_sort_download(e, A, A.rows, (uint32_t)back[1], (uint32_t)back[2], want, out);
}

// device ids -> external ids, into the caller's array
void neigh_copy_out(const cs_engine* ids_of, const std::vector<cs_neighbour_stat>& rows, cs_neighbour_stat* out, size_t cap) {
  const size_t k = std::min(rows.size(), cap);
  for (size_t i = 0; i < k; ++i) {
    out[i] = rows[i];
    out[i].id = ids_of->ext_id(rows[i].id);
    if (rows[i].nearest != CS_NO_NEIGHBOUR) out[i].nearest = ids_of->ext_id(rows[i].nearest);
  }
}

// mesh: the staged rows and the band of one tile, on its device for the length of the call
struct NeighHold {
  cs_engine* e = nullptr;
  DevBytes mem;
  uint32_t n = 0, n_band = 0;
  uint32_t* stage_id = nullptr;
  NeighRow* rows = nullptr;
  PairsBandRec* band = nullptr;
  uint32_t* band_slot = nullptr;
  ~NeighHold() {
    if (mem.get()) hipStreamSynchronize(e->stream);  // (then `mem` frees it)
  }
};

// mesh, step 1 on one tile (after sel_begin): the rows of the subjects it owns against the others it owns, staged by
// slot, and its band (on the device and in `band`).
int neigh_stage(cs_engine* e, const PairsArgs& P, uint32_t edges, uint32_t tile_index, NeighHold* h,
                std::vector<PairsBandRec>* band) {
  band->clear();
  h->e = e;
  if (int rc = e->refresh_counts()) return rc;
  if (int rc = e->ensure_index()) return rc;
  const uint32_t n = e->n_slots;
  h->n = n;
  if (!n) return 0;
  const bool want_band = edges && P.dist2 > 0.0;
  const size_t b_id = sel_up((size_t)n * sizeof(uint32_t)), b_rows = sel_up((size_t)n * sizeof(NeighRow));
  const size_t b_band = want_band ? sel_up((size_t)n * sizeof(PairsBandRec)) : 0u, b_slot = want_band ? b_id : 0u;
  if (h->mem.alloc(256u + b_id + b_rows + b_band + b_slot) != hipSuccess) {
    e->error = "agent_neighbours: out of device memory";
    return 90;
  }
  unsigned char* p = static_cast<unsigned char*>(h->mem.get());
  uint32_t* d_count = reinterpret_cast<uint32_t*>(p);
  h->stage_id = reinterpret_cast<uint32_t*>(p + 256u);
  h->rows = reinterpret_cast<NeighRow*>(p + 256u + b_id);
  h->band = reinterpret_cast<PairsBandRec*>(p + 256u + b_id + b_rows);
  h->band_slot = reinterpret_cast<uint32_t*>(p + 256u + b_id + b_rows + b_band);
  const uint32_t blocks = (n + PAIRS_BLOCK - 1u) / PAIRS_BLOCK;
  hipLaunchKernelGGL(k_neighbours<NEIGH_STAGE>, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], n,
                     e->cell_start.get(), e->sel_groups_dev.get(), P, 0ull, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                     h->rows, h->stage_id, n);
  HIP_OK_E(e, hipGetLastError());
  if (!want_band) {
    HIP_OK_E(e, hipStreamSynchronize(e->stream));
    return 0;
  }
  if (int rc = pairs_band_run(e, P, edges, tile_index, d_count, h->band, h->band_slot, "agent_neighbours", band)) return rc;
  h->n_band = (uint32_t)band->size();
  return 0;
}

// mesh, step 3 on one tile: its band subjects against the band others of the other tiles, merged into the staged rows
int neigh_cross(NeighHold* h, const std::vector<PairsBandRec>& foreign, double dist2) {
  cs_engine* e = h->e;
  if (!h->n_band || foreign.empty()) return 0;
  const uint32_t n_f = (uint32_t)foreign.size();
  PairsScratch sc(e);
  PairsBandRec* d_f = static_cast<PairsBandRec*>(sc.get(sel_up((size_t)n_f * sizeof(PairsBandRec))));
  if (!d_f) return 90;
  HIP_OK_E(e, hipMemcpyAsync(d_f, foreign.data(), (size_t)n_f * sizeof(PairsBandRec), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_neighbours_cross, dim3((h->n_band + PAIRS_BLOCK - 1u) / PAIRS_BLOCK), dim3(PAIRS_BLOCK), 0, e->stream,
                     h->band, h->band_slot, h->n_band, d_f, n_f, dist2, h->rows, h->n);
  HIP_OK_E(e, hipGetLastError());
  HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (the host records are uploaded)
  return 0;
}

// mesh, step 4 on one tile: min_count on the merged rows; the count, and with want > 0 the first rows, ascending
int neigh_report(NeighHold* h, uint64_t min_count, size_t want, std::vector<cs_neighbour_stat>* out, uint64_t* count) {
  cs_engine* e = h->e;
  out->clear();
  *count = 0;
  const uint32_t n = h->n;
  if (!n) return 0;
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  const uint32_t blocks = (n + PAIRS_BLOCK - 1u) / PAIRS_BLOCK;
  if (!want) {
    hipLaunchKernelGGL(k_neighbours_report<false>, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, h->stage_id, h->rows, n,
                       (unsigned long long)min_count, hdr, (unsigned long long*)nullptr, 0u);
    HIP_OK_E(e, hipGetLastError());
    unsigned long long found = 0;
    const int rc = pairs_read_count(e, hdr, &found);
    *count = found;
    return rc;
  }
  PairsScratch sc(e);
  NeighArrays A;
  if (int rc = neigh_arrays(&sc, n, want, false, &A)) return rc;
  hipLaunchKernelGGL(k_neighbours_report<true>, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, h->stage_id, h->rows, n,
                     (unsigned long long)min_count, hdr, A.keys, n);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long back[3];
  if (int rc = pairs_read_header(e, hdr, back)) return rc;
  if (back[1] > n) {
    e->error = "agent_neighbours: more rows than slots";
    return 90;
  }
  *count = back[1];
  return neigh_sort_download(e, A, h->rows, (uint32_t)back[1], (uint32_t)back[2], want, out);
}

}  // namespace

extern "C" {

size_t cs_agent_neighbours(cs_engine* e, double distance, const cs_selection* subjects, const cs_selection* others,
                           uint64_t min_count, cs_neighbour_stat* out, size_t cap) {
  if (!e) return SIZE_MAX;
  hipSetDevice(e->device);
  if (neigh_check(&e->error, distance, subjects, others)) return SIZE_MAX;
  if (sel_begin(e)) return SIZE_MAX;
  const size_t want = out ? cap : 0u;
  const PairsArgs P = pairs_args(e, distance, subjects, others);
  std::vector<cs_neighbour_stat> rows;
  uint64_t count = 0;
  if (neigh_run(e, P, min_count, want, &rows, &count)) return SIZE_MAX;
  if (want) neigh_copy_out(e, rows, out, cap);
  return (size_t)count;
}

// Collective: two gathers of variable size (two collectives each), whatever the crowd and the answer.  The first carries
// every rank's band records, the second its reported rows (the count-only form: its counts).
size_t cs_mesh_agent_neighbours(cs_mesh* m, double distance, const cs_selection* subjects, const cs_selection* others,
                                uint64_t min_count, cs_neighbour_stat* out, size_t cap) {
  if (!m) return SIZE_MAX;
  if (m->dead()) return SIZE_MAX;
  if (neigh_check(&m->error, distance, subjects, others)) return SIZE_MAX;
  if (near_check_mesh_distance(m, distance, "agent_neighbours")) return SIZE_MAX;
  if (cs_mesh_synchronize(m)) return SIZE_MAX;
  hipSetDevice(m->device);
  const size_t want = out ? cap : 0u;
  const size_t n_local = m->tiles.size();
  const double dist2 = distance * distance;
  int err = 0;
  std::string why;
  // 1. every tile: the rows of its own subjects against its own others, staged on its device, and its band
  std::vector<NeighHold> holds(n_local);
  std::vector<std::vector<PairsBandRec>> bands(n_local);
  for (size_t k = 0; k < n_local; ++k) {
    cs_engine* e = m->tiles[k];
    holds[k].e = e;
    if (!err) err = sel_begin(e);
    const PairsArgs P = pairs_args(e, distance, subjects, others);
    if (!err) err = neigh_stage(e, P, mesh_tile_edges(m, k), m->index_of[k], &holds[k], &bands[k]);
    if (err && why.empty()) why = cs_last_error(e);
  }
  // 2. the band records of every tile on every rank
  std::vector<PairsBandRec> every;
  if (mesh_gather_bands(m, bands, "a tile of another rank failed while counting neighbours", &err, &why, &every)) return SIZE_MAX;
  // 3. every local tile's band subjects against the band others of every other tile, merged on the device; then
  //    min_count, the order and the download of each tile's run
  uint64_t total = 0;
  std::vector<cs_neighbour_stat> all;  // the sorted runs, one behind the other
  std::vector<size_t> ends;
  for (size_t k = 0; k < n_local && !err; ++k) {
    const uint32_t index = m->index_of[k];
    std::vector<PairsBandRec> foreign;
    for (const PairsBandRec& r : every)
      if ((r.bits >> 2) != index && (r.bits & 2u)) foreign.push_back(r);
    err = neigh_cross(&holds[k], foreign, dist2);
    std::vector<cs_neighbour_stat> part;
    uint64_t c = 0;
    if (!err) err = neigh_report(&holds[k], min_count, want, &part, &c);
    if (err && why.empty()) why = cs_last_error(m->tiles[k]);
    total += c;
    all.insert(all.end(), part.begin(), part.end());
    ends.push_back(all.size());
  }
  mesh_merge_runs(all, ends, neigh_by_id);
  if (all.size() > want) all.resize(want);
  // 4. the rows (or only the counts) of every rank: [0 ok / 1 failed, count, n listed, rows as four words each]
  if (m->distributed) {
    std::vector<uint64_t> mine{err ? 1u : 0u, total, err ? 0u : all.size()};
    if (mine[2]) {
      mine.resize(3u + 4u * all.size());
      std::memcpy(&mine[3], all.data(), all.size() * sizeof(cs_neighbour_stat));
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
      uint64_t head[3] = {1u, 0u, 0u};
      if (words >= 3u) std::memcpy(head, part.data(), sizeof head);
      if (words < 3u || head[0] != 0u || words != 3u + 4u * head[2]) {
        if (!err) {
          err = 90;
          why = "a tile of another rank failed while counting neighbours";
        }
        continue;
      }
      total += head[1];
      const size_t n = (size_t)head[2], at = all.size();
      all.resize(at + n);
      if (n) std::memcpy(&all[at], part.data() + sizeof head, n * sizeof(cs_neighbour_stat));
      ends.push_back(all.size());
    }
    mesh_merge_runs(all, ends, neigh_by_id);
    if (all.size() > want) all.resize(want);
  }
  if (err) {
    m->error = why;
    return SIZE_MAX;
  }
  if (want && !m->tiles.empty()) neigh_copy_out(m->tiles[0], all, out, cap);
  return (size_t)total;
}

}  // extern "C"
