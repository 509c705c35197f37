// cs_mesh.hip.inc — a crowd cut into spatial tiles behind ONE handle (SURVEY.md section 8e): layout, tile engines,
// halo buffers, the exchange, the spawn flags, route-cache misses, re-cuts and merged spatial queries.
// Part of the single translation unit crowdstep_hip.hip (included there, last).
//
// The reference's single entry point is `Simulation` (lib.rs:69-192); a host in any language (the Rust shim,
// include/crowdsim.hpp, rmf_crowdsim_amd/tiles.py) gets the multi-tile form of it from these calls instead of
// re-implementing the orchestration around cs_tile_step_rccl.  Two forms:
//   n_ranks == 1   every tile of the layout in this process on one device (exchanges = device copies on the shared
//                  stream): the single-GPU double of the multi-GPU logic, and what the C++ / Python tests drive
//   n_ranks  > 1   one tile per rank (rank = tile index = tx * tiles_y + ty), halo records over RCCL from the engine
//                  itself (cs_tile_step_rccl when nothing has to reach the host between the phases), or over a
//                  transport the host brings (cs_mesh_host_transport: MPI, gloo, ...; staged through pinned host
//                  memory), which also carries what needs every rank's answer: route-cache misses, re-cuts, queries
// Everything a tile engine does stays in cs_engine; this file only decides who is asked what, in which order.

struct cs_mesh {
  cs_grid_desc grid{};
  uint32_t tiles_x = 1, tiles_y = 1, halo = 1, flags = 0;
  int32_t rank = 0, n_ranks = 1;
  bool distributed = false;  // one tile per rank (a communicator's unique id or a host transport was given), else all tiles here
  bool use_rccl = false;     // halo records and spawn flags over RCCL from the engine itself
  bool has_host = false;     // a transport of the host's: instead of RCCL, or beside it for the gathers
  cs_mesh_host_transport host{};
  PinnedBuf<unsigned char> stage_send[8];  // pinned host copies of the halo buffers (host transport without RCCL)
  PinnedBuf<unsigned char> stage_recv[8];
  int device = 0;
  double density_per_cell = 16.0;
  uint64_t capacity_hint = 0;
  uint32_t rows = 0, cols = 0;            // global cell rows (x) and columns (y)
  std::vector<uint32_t> x_edges, y_edges;  // tensor-product cuts
  std::vector<cs_engine*> tiles;           // the local tiles
  std::vector<uint32_t> index_of;          // their global tile indices
  struct Buf {
    DevBytes send, recv;
    uint32_t cap = 0;
  };
  std::vector<std::array<Buf, 8>> bufs;
  hipStream_t stream = nullptr;
  std::vector<DevBuf<int>> flag_bufs;  // device-side spawn flags, one vector per local tile
  size_t flag_cap = 0;
  bool has_sinks = false, host_planner = false, route_legs = false, recording = false;
  std::string error;
  // agents whose index insert failed in cs_mesh_add_agents (cs_engine::limbo; lib.rs:133-149): every rank sees the same
  // call and keeps the same list; they are counted and read once, removable, and fail every step until removed
  struct Limbo {
    cs_agent_view view;
    uint32_t hlp;
    uint32_t lp;  // (the selections ask for it: cs_select.hip.inc)
  };
  std::vector<Limbo> limbo;
  uint64_t field_gather_bytes = 0;  // what this rank contributed to the gather of the last cs_mesh_agent_field
  // CS_CFG_WIDE_IDS: an upper bound of the device ids the tiles have handed out, moved by the same calls on every rank
  // (adds, and one id per source-sink slot and step), so that every rank decides alike when to renumber (mesh_ids_room)
  uint64_t id_bound = 0;
  // A step that failed on ANY tile ends the run of the whole mesh: the tiles before the failing one have taken the
  // step, the ones behind it have not, and the next exchange would mix two time steps.  Every later call fails with
  // the first error, on every rank alike (the single engine commits nothing on "Index out of bounds", lib.rs:299-302
  // leaves the reference's index half-updated; a mesh can do neither and stops).
  bool poisoned = false;
  std::string poison_error;
  int poison_rc = 7;
  // Distributed form over RCCL, steps that do not wait for the host: a rank cannot leave the schedule on its own (its
  // peers' ncclSend / ncclRecv would wait for ever), so failures are AGREED on: every `check_every` steps every rank
  // all-reduces "has my tile failed" (its device-side error counters, fresher than what its host has seen) and all
  // stop together.  A rank whose host learns of its failure earlier issues only the collectives of its steps until then.
  uint32_t check_every = 32, steps_since_check = 0;
  int deferred_rc = 0;
  std::string deferred_error;
  // ... and, since round 5, AGREED ON WITHOUT A COLLECTIVE through the halo messages themselves: word 1 of every halo
  // header carries the sender's failure word (Counters::mesh_fail_step: 1 + the index u0 of the mesh step in whose
  // unpack the earliest known failure was first seen), every tile forwards the smallest it has seen, so after D = the
  // mesh's diameter in tiles exchanges every tile holds the same word, and EVERY rank leaves the schedule at the same
  // call: the one after step S = u0 + D + lag (lag = how stale a host's view of its device may be: 0 when the host waits
  // for every step anyway, kFlight + 1 steps in the fire-and-forget form).  Nobody issues a collective of a step beyond
  // S, nobody stops before it, whichever rank failed and however many did.  The all-reduce every `check_every` steps
  // stays as the backstop.  CS_MESH_HEADER_AGREE=0 (tests) leaves only the backstop.
  bool header_agree = true;
  uint64_t step_index = 0;   // calls of cs_mesh_step so far that issued their collectives: the same on every rank
  uint32_t fail_word = 0;    // the failure word as the host last read it from the device (exact on a rank that waits)
  uint32_t diameter() const { return std::max(tiles_x, tiles_y) - 1u; }  // (eight neighbours each: Chebyshev distance)
  uint32_t step_tag() const { return (uint32_t)std::min<uint64_t>(step_index + 1u, 0xFFFFFFF0ull); }
  DevBuf<int> agree_dev;       // device int for the agreed check
  PinnedBuf<int> agree_host;   // pinned

  uint32_t n_tiles() const { return tiles_x * tiles_y; }
  void rect(uint32_t index, uint32_t* x0, uint32_t* x1, uint32_t* y0, uint32_t* y1) const {
    const uint32_t tx = index / tiles_y, ty = index % tiles_y;
    *x0 = x_edges[tx]; *x1 = x_edges[tx + 1]; *y0 = y_edges[ty]; *y1 = y_edges[ty + 1];
  }
  // global index of the neighbour of `index` in direction d, or -1
  int neighbour(uint32_t index, int d) const {
    static const int step[8][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {-1, 1}, {1, -1}, {1, 1}};
    const int nx_ = (int)(index / tiles_y) + step[d][0], ny_ = (int)(index % tiles_y) + step[d][1];
    if (nx_ < 0 || ny_ < 0 || nx_ >= (int)tiles_x || ny_ >= (int)tiles_y) return -1;
    return nx_ * (int)tiles_y + ny_;
  }
  static int opposite(int d) {
    static const int opp[8] = {1, 0, 3, 2, 7, 6, 5, 4};
    return opp[d];
  }
  int local_of(uint32_t index) const {
    for (size_t k = 0; k < index_of.size(); ++k)
      if (index_of[k] == index) return (int)k;
    return -1;
  }
  int fail(cs_engine* e, int rc) {
    error = cs_last_error(e);
    return rc;
  }
  int poison(int rc, const std::string& why) {
    if (!poisoned) {
      poisoned = true;
      poison_rc = rc ? rc : 7;
      poison_error = why;
    }
    error = poison_error;
    return poison_rc;
  }
  // (first line of every call that touches the crowd)
  bool dead() {
    if (poisoned) error = poison_error;
    return poisoned;
  }
};

// ---- layout --------------------------------------------------------------------------------------------
// `parts` runs of about equal weight over range(hist.size()), each at least min_width wide: the cumulative
// histogram's quantiles, pushed apart where needed
static std::vector<uint32_t> mesh_weighted_edges(const std::vector<double>& hist, uint32_t parts, uint32_t min_width) {
  const uint32_t n = (uint32_t)hist.size();
  std::vector<double> cum(n + 1, 0.0);
  for (uint32_t k = 0; k < n; ++k) cum[k + 1] = cum[k] + hist[k];
  std::vector<uint32_t> edges{0u};
  for (uint32_t k = 1; k < parts; ++k) {
    const double want = cum[n] * (double)k / (double)parts;
    long long e = std::lower_bound(cum.begin(), cum.end(), want) - cum.begin();
    e = std::max<long long>(e, (long long)edges.back() + min_width);
    e = std::min<long long>(e, (long long)n - (long long)(parts - k) * min_width);
    edges.push_back((uint32_t)std::max<long long>(e, 0));
  }
  edges.push_back(n);
  return edges;
}
static std::vector<uint32_t> mesh_even_edges(uint32_t n, uint32_t parts) {
  std::vector<uint32_t> e(parts + 1);
  for (uint32_t k = 0; k <= parts; ++k) e[k] = (uint32_t)std::nearbyint((double)k * n / parts);
  return e;
}
static bool mesh_edges_ok(const cs_mesh* m) {
  for (size_t k = 0; k + 1 < m->x_edges.size(); ++k)
    if (m->x_edges[k + 1] < m->x_edges[k] + 2 * m->halo) return false;
  for (size_t k = 0; k + 1 < m->y_edges.size(); ++k)
    if (m->y_edges[k + 1] < m->y_edges[k] + 2 * m->halo) return false;
  return true;
}

// records of one direction's buffers; both ends of a link compute the same number (the cuts are a tensor
// product): an edge carries a band of 2 * halo cells along the shared edge, a corner the (2 * halo)^2 cells where
// two bands cross, with 2x slack
static uint32_t mesh_halo_capacity(const cs_mesh* m, uint32_t index, int d) {
  uint32_t x0, x1, y0, y1;
  m->rect(index, &x0, &x1, &y0, &y1);
  const double band = 2.0 * m->halo;
  double cells;
  if (d == CS_DIR_XLO || d == CS_DIR_XHI) cells = ((double)(y1 - y0) + 4.0 * m->halo) * band;
  else if (d == CS_DIR_YLO || d == CS_DIR_YHI) cells = ((double)(x1 - x0) + 4.0 * m->halo) * band;
  else cells = 4.0 * band * band;
  return (uint32_t)std::max(256.0, 2.0 * m->density_per_cell * cells);
}

static int mesh_set_buffers(cs_mesh* m, size_t local) {
  hipSetDevice(m->device);
  for (int d = 0; d < 8; ++d) {
    cs_mesh::Buf& b = m->bufs[local][d];
    b = cs_mesh::Buf{};
    if (m->neighbour(m->index_of[local], d) < 0) continue;
    b.cap = mesh_halo_capacity(m, m->index_of[local], d);
    const size_t bytes = ((size_t)b.cap + 1u) * CS_HALO_RECORD_BYTES;
    if (b.send.alloc(bytes) != hipSuccess || b.recv.alloc(bytes) != hipSuccess ||
        hipMemsetAsync(b.send.get(), 0, bytes, m->stream) != hipSuccess || hipMemsetAsync(b.recv.get(), 0, bytes, m->stream) != hipSuccess) {
      m->error = "HIP error while allocating halo buffers";
      return 90;
    }
    if (int rc = cs_halo_set_buffers(m->tiles[local], (uint32_t)d, b.send.get(), b.recv.get(), b.cap)) return m->fail(m->tiles[local], rc);
  }
  return 0;
}

static int mesh_set_peers(cs_mesh* m) {  // n_ranks > 1: rank of the tile behind every direction
  int32_t peers[8];
  for (int d = 0; d < 8; ++d) peers[d] = m->neighbour(m->index_of[0], d);
  return cs_halo_set_peers(m->tiles[0], peers);
}

// ---- a transport of the host's (cs_mesh_host_transport) ----------------------------------------------------
static int mesh_host_fail(cs_mesh* m, const char* what) {
  m->error = std::string("cs_mesh: the host transport's ") + what + " failed";
  return 91;
}
// The gathers of a distributed mesh (re-cuts, merged queries, route-cache misses, the whole crowd's agents): through
// the host's transport when there is one, else over RCCL from the engine (device staging around ncclAllGather).
// every rank's `bytes` bytes (the same number everywhere) to every rank, in rank order
static int mesh_allgather(cs_mesh* m, const void* mine, size_t bytes, void* all) {
  if (m->has_host) return m->host.allgather(m->host.user, mine, bytes, all) ? mesh_host_fail(m, "allgather") : 0;
  if (!bytes) return 0;
  cs_engine* e = m->tiles[0];
  hipSetDevice(m->device);
  DevBuf<unsigned char> mem;
  const size_t total = bytes * (size_t)m->n_ranks;
  int rc = 0;
  const hipError_t got = mem.alloc(bytes + total);
  unsigned char* dev = mem.get();
  if (got != hipSuccess ||
      hipMemcpyAsync(dev, mine, bytes, hipMemcpyHostToDevice, m->stream) != hipSuccess) {
    m->error = "HIP error in a gather of the mesh";
    rc = 90;
  }
  if (!rc && (rc = cs_allgather_bytes_rccl(e, dev, dev + bytes, bytes)) != 0) m->error = cs_last_error(e);
  if (!rc && (hipMemcpyAsync(all, dev + bytes, total, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
              hipStreamSynchronize(m->stream) != hipSuccess)) {
    m->error = "HIP error in a gather of the mesh";
    rc = 90;
  }
  return rc;
}
// element-wise maximum over the ranks, in place (host values)
static int mesh_allreduce_max(cs_mesh* m, int32_t* values, size_t n) {
  if (m->has_host) return m->host.allreduce_max_i32(m->host.user, values, n) ? mesh_host_fail(m, "allreduce_max_i32") : 0;
  if (!n) return 0;
  cs_engine* e = m->tiles[0];
  hipSetDevice(m->device);
  DevBuf<int> mem;
  int rc = 0;
  const hipError_t got = mem.alloc(n);
  int* dev = mem.get();
  if (got != hipSuccess ||
      hipMemcpyAsync(dev, values, n * sizeof(int), hipMemcpyHostToDevice, m->stream) != hipSuccess) {
    m->error = "HIP error in an all-reduce of the mesh";
    rc = 90;
  }
  if (!rc && (rc = cs_allreduce_max_i32_rccl(e, dev, n)) != 0) m->error = cs_last_error(e);
  if (!rc && (hipMemcpyAsync(values, dev, n * sizeof(int), hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
              hipStreamSynchronize(m->stream) != hipSuccess)) {
    m->error = "HIP error in an all-reduce of the mesh";
    rc = 90;
  }
  return rc;
}
// every rank's bytes, in rank order (sizes may differ: lengths first, then the padded payloads)
static int mesh_host_gatherv(cs_mesh* m, const void* mine, size_t bytes, std::vector<std::vector<unsigned char>>& out) {
  const size_t nr = (size_t)m->n_ranks;
  std::vector<uint64_t> sizes(nr, 0);
  const uint64_t my = bytes;
  if (int rc = mesh_allgather(m, &my, sizeof my, sizes.data())) return rc;
  uint64_t most = 0;
  for (uint64_t v : sizes) most = std::max(most, v);
  out.assign(nr, {});
  if (!most) return 0;
  std::vector<unsigned char> pad((size_t)most, 0), all((size_t)most * nr);
  if (bytes) std::memcpy(pad.data(), mine, bytes);
  if (int rc = mesh_allgather(m, pad.data(), (size_t)most, all.data())) return rc;
  for (size_t r = 0; r < nr; ++r) out[r].assign(all.begin() + r * most, all.begin() + r * most + sizes[r]);
  return 0;
}
// CS_CFG_WIDE_IDS: room for n_new more device ids.  While the rank-uniform bound allows, nothing happens; else every
// tile synchronises, and if the exact counter needs it the mesh renumbers: each tile sorts its live agents' external ids
// on the device, the mesh gathers them (counts, then ids: mesh_host_gatherv over the host transport or RCCL; the tiles of
// this process directly), every rank merges the same global table, and each tile maps its agents by binary search in it
// (k_ids_renumber_ext).  Between two mesh steps no tile holds ghosts, and what the step kernels packed is voided, so the
// next exchange carries the new ids.  Collective: every rank makes the same calls.
// merge the runs of v ending at `ends`, each ascending under `less` (pairwise, in place)
template <class T, class Less = std::less<T>>
static void mesh_merge_runs(std::vector<T>& v, std::vector<size_t> ends, Less less = Less()) {
  while (ends.size() > 1) {
    std::vector<size_t> next;
    for (size_t i = 0; i < ends.size(); i += 2) {
      if (i + 1 < ends.size()) {
        const size_t b = i ? ends[i - 1] : 0;
        std::inplace_merge(v.begin() + (long)b, v.begin() + (long)ends[i], v.begin() + (long)ends[i + 1], less);
      }
      next.push_back(ends[std::min(i + 1, ends.size() - 1)]);
    }
    ends.swap(next);
  }
}
static int mesh_ids_room(cs_mesh* m, uint64_t n_new) {
  if (!(m->flags & CS_CFG_WIDE_IDS) || m->tiles.empty()) return 0;
  cs_engine* t0 = m->tiles[0];
  if (m->id_bound + n_new < t0->id_limit) {
    m->id_bound += n_new;
    return 0;
  }
  const auto t_start = std::chrono::steady_clock::now();
  for (cs_engine* e : m->tiles) {
    hipSetDevice(e->device);
    if (int rc = e->sync_next_id()) return m->fail(e, rc);
  }
  if (t0->next_id + n_new < t0->id_limit) {  // the bound was loose: no renumbering yet
    m->id_bound = t0->next_id + n_new;
    return 0;
  }
  std::vector<uint64_t> all, mine;
  std::vector<size_t> ends;
  for (cs_engine* e : m->tiles) {
    hipSetDevice(e->device);
    if (int rc = e->wide_owned_ext(&mine)) return m->fail(e, rc);
    all.insert(all.end(), mine.begin(), mine.end());
    ends.push_back(all.size());
  }
  mesh_merge_runs(all, ends);  // every tile's list is sorted on its device
  if (m->distributed) {
    std::vector<std::vector<unsigned char>> parts;
    if (int rc = mesh_host_gatherv(m, all.data(), all.size() * sizeof(uint64_t), parts)) return rc;
    all.clear();
    ends.clear();
    for (const auto& p : parts) {
      const size_t k = p.size() / sizeof(uint64_t), at = all.size();
      all.resize(at + k);
      if (k) std::memcpy(all.data() + at, p.data(), k * sizeof(uint64_t));
      ends.push_back(all.size());
    }
    mesh_merge_runs(all, ends);  // (every rank's part is sorted)
  }
  const uint64_t live = all.size();
  if (2u * live + 1u + n_new >= t0->id_limit) {
    m->error = "agent id space exhausted: " + std::to_string(live) + " live agents need " + std::to_string(2u * live + 1u) +
               " device ids after a renumbering, and this allocation " + std::to_string(n_new) +
               " more; the device id limit is " + std::to_string(t0->id_limit);
    return 4;
  }
  const uint64_t next_ext = t0->ext_id(t0->next_id);
  for (cs_engine* e : m->tiles) {
    hipSetDevice(e->device);
    if (int rc = e->wide_apply_table(all, next_ext)) return m->fail(e, rc);
  }
  const uint64_t ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() -
                                                                                      t_start).count();
  for (cs_engine* e : m->tiles) e->renumber_ns += ns;
  m->id_bound = t0->next_id + n_new;
  return 0;
}

// pinned staging for the halo buffers of the local tile (after mesh_set_buffers)
static int mesh_host_stage_alloc(cs_mesh* m) {
  for (int d = 0; d < 8; ++d) {
    m->stage_send[d].release();
    m->stage_recv[d].release();
    const cs_mesh::Buf& b = m->bufs[0][d];
    if (!b.send.get()) continue;
    const size_t bytes = ((size_t)b.cap + 1u) * CS_HALO_RECORD_BYTES;
    if (m->stage_send[d].alloc(bytes) != hipSuccess || m->stage_recv[d].alloc(bytes) != hipSuccess) {
      m->error = "HIP error while allocating the halo staging buffers";
      return 90;
    }
  }
  return 0;
}
// 1 when the tile's cumulative error counters say that some step has failed (what cs_engine::refresh_counts turns
// into an error when the host gets to read them), OR-ed with what the host already knows
__global__ void k_mesh_fail_flag(const Counters* __restrict__ ctr, int host_failed, int* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    out[0] = (host_failed || ctr->n_out_of_bounds || ctr->n_halo_late || ctr->n_early_stalled || ctr->n_win_dropped || ctr->n_scan_stalled || ctr->n_halo_overflow) ? 1 : 0;
}

// The failure word of a tile that does not run its halo unpack (a failed rank that only keeps its peers' collectives
// company, or the moment the host learns of a failure the device cannot know of): what k_halo_unpack_all's first wave
// does, plus `raise` (0, or the tag of the mesh step in which the host noticed).  One wave.
__global__ void k_mesh_fail_merge(HaloBuffers8 recv, HaloBuffers8 send, Counters* __restrict__ ctr, uint32_t step_tag,
                                  uint32_t raise, uint32_t clear_counts, uint32_t* __restrict__ out) {
  const uint32_t t = threadIdx.x;
  uint32_t word = 0u;
  if (t < 8 && recv.p[t]) word = reinterpret_cast<const uint32_t*>(recv.p[t])[1];
  if (t == 8) {
    word = ctr->mesh_fail_step;
    if (!word && (ctr->n_out_of_bounds | ctr->n_halo_late | ctr->n_early_stalled | ctr->n_win_dropped | ctr->n_scan_stalled | ctr->n_halo_overflow))
      word = step_tag;
    if (!word) word = raise;
  }
  uint32_t key = word ? word : 0xFFFFFFFFu;
  for (int d = 8; d > 0; d >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, d, 64));
  word = key == 0xFFFFFFFFu ? 0u : key;
  if (t == 0) {
    ctr->mesh_fail_step = word;
    out[0] = word;
  }
  if (t < 8 && send.p[t]) {
    reinterpret_cast<uint32_t*>(send.p[t])[1] = word;
    // a failed tile no longer fills its send buffers: its neighbours get empty messages, not the records of its last step again
    if (clear_counts) reinterpret_cast<uint32_t*>(send.p[t])[0] = 0u;
  }
}

static const char* kPeerFailed =
    "a tile of this mesh failed its step on another rank (that rank's cs_mesh_last_error says why); the mesh has stopped "
    "on every rank";

// The ranks have agreed that the run is over: this rank says why.  Its own failure if it has one (what its host knows;
// what its engine says when asked; what the tile's counters say that the engine treats as fatal only in some states: a
// halo buffer that overflowed), else "another rank".  Waits for the device.  Poisons the mesh.
static int mesh_stop(cs_mesh* m, int local_rc, const std::string& local_error) {
  if (local_rc) return m->poison(local_rc, local_error);
  for (cs_engine* e : m->tiles) {
    if (int rc = cs_synchronize(e)) return m->poison(rc, cs_last_error(e));
    Counters c;
    if (e->read_counters(&c) == 0) {
      if (c.n_halo_overflow)
        return m->poison(7, "halo buffer overflow on this rank's tile (more records for a neighbour, or more arriving agents, "
                            "than the buffers of this mesh hold: raise density_per_cell / capacity_hint of cs_mesh_create)");
      if (c.n_halo_late || c.n_early_stalled || c.n_win_dropped || c.n_scan_stalled || c.n_out_of_bounds)
        return m->poison(7, "this rank's tile failed a step (its error counters are set) although its engine reports none");
    }
  }
  return m->poison(7, kPeerFailed);
}

// the failure word of this rank's tile, merged with what its neighbours sent in the last exchange and with `raise`, read
// back (waits for the stream: only ranks that wait anyway, or have failed, ask)
static int mesh_fail_word_now(cs_mesh* m, uint32_t raise, uint32_t* word) {
  cs_engine* e = m->tiles[0];
  hipSetDevice(m->device);
  if (!m->agree_dev.get() && (m->agree_dev.alloc(1) != hipSuccess || m->agree_host.alloc(1) != hipSuccess))
    return m->poison(90, "HIP error in the agreed check of the mesh");
  HaloBuffers8 recv, send;
  for (int d = 0; d < 8; ++d) {
    recv.p[d] = e->halo[d].recv;
    send.p[d] = e->halo[d].send;
    recv.cap[d] = send.cap[d] = e->halo[d].cap;
  }
  hipLaunchKernelGGL(k_mesh_fail_merge, dim3(1), dim3(64), 0, e->stream, recv, send, e->ctr.get(), m->step_tag(), raise,
                     m->deferred_rc ? 1u : 0u, reinterpret_cast<uint32_t*>(m->agree_dev.get()));
  if (hipMemcpyAsync(m->agree_host.get(), m->agree_dev.get(), sizeof(int), hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
      hipStreamSynchronize(e->stream) != hipSuccess)
    return m->poison(90, "HIP error in the agreed check of the mesh");
  *word = (uint32_t)*m->agree_host.get();
  return 0;
}

// Has the step arrived after which every rank leaves?  `lag`: see cs_mesh::header_agree.  0 = go on; *last = this call
// is the last that issues collectives (no exchange may be made ahead in it).
static bool mesh_past_the_agreed_stop(const cs_mesh* m, uint32_t word, uint32_t lag, bool* last) {
  *last = false;
  if (!word) return false;
  const uint64_t stop_after = (uint64_t)(word - 1u) + m->diameter() + lag;
  *last = m->step_index >= stop_after;
  return m->step_index > stop_after;
}

// Collective over the ranks of a distributed mesh: has any tile failed?  `local_rc` / `local_error`: what this rank's
// host knows (0 = nothing).  RCCL form: the flag is formed on the device from the tile's error counters (so a failure
// the host has not seen yet counts), all-reduced and read back: one wait for the device.  Host-transport form: the
// host's all-reduce.  Poisons the mesh and returns non-zero on every rank when any rank failed.
static int mesh_agree(cs_mesh* m, int local_rc, const std::string& local_error) {
  int failed = local_rc != 0 ? 1 : 0;
  if (m->use_rccl) {
    cs_engine* e = m->tiles[0];
    hipSetDevice(m->device);
    if (!m->agree_dev.get() && (m->agree_dev.alloc(1) != hipSuccess || m->agree_host.alloc(1) != hipSuccess))
      return m->poison(90, "HIP error in the agreed check of the mesh");
    hipLaunchKernelGGL(k_mesh_fail_flag, dim3(1), dim3(64), 0, m->stream, e->ctr.get(), failed, m->agree_dev.get());
    if (cs_allreduce_max_i32_rccl(e, m->agree_dev.get(), 1) != 0) return m->poison(8, cs_last_error(e));
    if (hipMemcpyAsync(m->agree_host.get(), m->agree_dev.get(), sizeof(int), hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
      return m->poison(90, "HIP error in the agreed check of the mesh");
    failed = *m->agree_host.get();
  } else if (m->has_host) {
    int32_t v = failed;
    if (m->host.allreduce_max_i32(m->host.user, &v, 1)) return m->poison(91, "cs_mesh: the host transport's allreduce_max_i32 failed");
    failed = v;
  }
  if (!failed) return 0;
  return mesh_stop(m, local_rc, local_error);
}

__global__ void k_i32_max(int* __restrict__ dst, const int* __restrict__ src, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = max(dst[i], src[i]);
}

static thread_local std::string g_mesh_create_error;

extern "C" {

// every rank's `bytes` bytes to every rank, in rank order (device buffers; recv holds n_ranks * bytes), on the
// engine's stream: what a mesh's re-cuts, merged queries and route-cache misses need
int cs_allgather_bytes_rccl(cs_engine* e, const void* send_dev, void* recv_dev, size_t bytes) {
  hipSetDevice(e->device);
  rccl_api::Api& a = rccl_api::api();
  if (!a.handle || !e->rccl_comm) {
    e->error = a.handle ? "no RCCL communicator: call cs_rccl_comm_init or cs_rccl_comm_adopt first" : a.why;
    return 8;
  }
  if (bytes == 0) return 0;
  // (ordered behind an exchange made ahead on the second stream, like cs_allreduce_max_i32_rccl)
  if (e->aux_stream && e->ev_xchg && hipStreamWaitEvent(e->stream, e->ev_xchg, 0) != hipSuccess) return 90;
  return rccl_api::ok(e, a.all_gather(send_dev, recv_dev, bytes, rccl_api::kUint8, e->rccl_comm, e->stream), "ncclAllGather") ? 0 : 8;
}


cs_mesh* cs_mesh_create(const cs_grid_desc* grid, const cs_mesh_desc* d) {
  auto bad = [&](cs_mesh* m, const std::string& why) -> cs_mesh* {
    g_mesh_create_error = why;
    if (m) cs_mesh_destroy(m);
    return nullptr;
  };
  if (!grid || !d || d->tiles_x == 0 || d->tiles_y == 0 || d->halo_cells == 0)
    return bad(nullptr, "cs_mesh_create: a grid, tiles_x, tiles_y >= 1 and halo_cells >= 1 are required");
  if (d->n_ranks > 1 && (uint32_t)d->n_ranks != d->tiles_x * d->tiles_y)
    return bad(nullptr, "cs_mesh_create: with n_ranks > 1 there is one tile per rank (n_ranks = tiles_x * tiles_y)");
  const cs_mesh_host_transport* ht = d->host_transport;
  if (ht && (!ht->exchange || !ht->allreduce_max_i32 || !ht->allgather))
    return bad(nullptr, "cs_mesh_create: a host transport brings exchange, allreduce_max_i32 and allgather");
  if (d->n_ranks > 1 && (d->rank < 0 || d->rank >= d->n_ranks || (!d->rccl_unique_id && !ht)))
    return bad(nullptr, "cs_mesh_create: rank in [0, n_ranks) and a transport (the communicator's unique id or a "
                        "cs_mesh_host_transport) are required");
  if ((d->rccl_unique_id || ht) && std::max(1, d->n_ranks) != (int32_t)(d->tiles_x * d->tiles_y))
    return bad(nullptr, "cs_mesh_create: a distributed mesh has one tile per rank (n_ranks = tiles_x * tiles_y)");
  cs_mesh* m = new cs_mesh();
  m->grid = *grid;
  m->tiles_x = d->tiles_x;
  m->tiles_y = d->tiles_y;
  m->halo = d->halo_cells;
  m->flags = d->flags;
  m->rank = d->n_ranks > 1 ? d->rank : 0;
  m->n_ranks = std::max(1, d->n_ranks);
  m->use_rccl = d->rccl_unique_id != nullptr;
  m->has_host = ht != nullptr;
  if (ht) m->host = *ht;
  m->distributed = m->use_rccl || m->has_host;  // (also with ONE rank: the same calls, a communicator of one)
  m->device = d->device_ordinal;
  m->density_per_cell = d->density_per_cell > 0.0 ? d->density_per_cell : 16.0;
  m->capacity_hint = d->capacity_hint;
  if (const char* v = getenv("CS_MESH_CHECK_EVERY")) m->check_every = (uint32_t)std::max(1, atoi(v));  // (tests)
  if (const char* v = getenv("CS_MESH_HEADER_AGREE")) m->header_agree = atoi(v) != 0;                   // (tests)
  m->cols = (uint32_t)(grid->width / grid->cell_size);   // the row stride: y cells per x row
  m->rows = (uint32_t)(grid->height / grid->cell_size);  // x rows
  if (d->weights_xy && d->n_weights) {  // cuts at the quantiles of where these points stand
    std::vector<double> hx(m->rows, 0.0), hy(m->cols, 0.0);
    for (size_t k = 0; k < d->n_weights; ++k) {
      const double cx = std::floor((d->weights_xy[2 * k] - grid->offset_x) / grid->cell_size);
      const double cy = std::floor((d->weights_xy[2 * k + 1] - grid->offset_y) / grid->cell_size);
      hx[(size_t)std::min(std::max(cx, 0.0), (double)m->rows - 1.0)] += 1.0;
      hy[(size_t)std::min(std::max(cy, 0.0), (double)m->cols - 1.0)] += 1.0;
    }
    m->x_edges = mesh_weighted_edges(hx, m->tiles_x, 2 * m->halo);
    m->y_edges = mesh_weighted_edges(hy, m->tiles_y, 2 * m->halo);
  } else {
    m->x_edges = mesh_even_edges(m->rows, m->tiles_x);
    m->y_edges = mesh_even_edges(m->cols, m->tiles_y);
  }
  if (!mesh_edges_ok(m)) return bad(m, "cs_mesh_create: a tile would be thinner than two halo rings");
  if (hipSetDevice(m->device) != hipSuccess || hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess)
    return bad(m, "cs_mesh_create: no such device, or hipStreamCreate failed");
  for (uint32_t index = 0; index < m->n_tiles(); ++index) {
    if (m->distributed && (int32_t)index != m->rank) continue;
    cs_device_cfg cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.device_ordinal = m->device;
    cfg.flags = m->flags;
    m->rect(index, &cfg.tile_cx0, &cfg.tile_cx1, &cfg.tile_cy0, &cfg.tile_cy1);
    cfg.halo_cells = m->halo;
    cfg.capacity_hint = m->capacity_hint;
    cfg.stream = m->stream;  // ONE stream orders pack -> copy -> unpack -> step over all local tiles
    cs_engine* e = cs_create(grid, &cfg);
    if (!e) return bad(m, std::string("cs_mesh_create: ") + cs_last_error(nullptr));
    cs_event_recording(e, 0);  // no listeners yet (lib.rs:88); cs_mesh_event_recording turns the events on
    m->tiles.push_back(e);
    m->index_of.push_back(index);
    m->bufs.emplace_back();
    if (mesh_set_buffers(m, m->tiles.size() - 1)) return bad(m, m->error);
  }
  if (m->distributed) {
    if (m->use_rccl && (cs_rccl_comm_init(m->tiles[0], m->n_ranks, m->rank, d->rccl_unique_id) || mesh_set_peers(m)))
      return bad(m, std::string("cs_mesh_create: ") + cs_last_error(m->tiles[0]));
    if (!m->use_rccl && mesh_host_stage_alloc(m)) return bad(m, m->error);
    // Layout and halo capacities are computed on every rank from its own descriptor and are not exchanged;
    // two ranks that disagree would post sends and receives of different sizes, which RCCL answers with a
    // hang.  One small all-reduce (the call the spawn flags use) compares a checksum of what the sizes
    // depend on: max(h) and max(-h) bracket every rank's h.
    uint64_t h = 0xCBF29CE484222325ull;
    auto mix = [&](uint64_t v) { h = (h ^ v) * 0x100000001B3ull; };
    auto mix_f64 = [&](double v) {
      uint64_t bits;
      memcpy(&bits, &v, sizeof(bits));
      mix(bits);
    };
    for (uint32_t v : m->x_edges) mix(v);
    for (uint32_t v : m->y_edges) mix(0x10000u + v);
    mix(m->halo);
    mix((uint64_t)m->n_ranks);
    mix_f64(m->density_per_cell);  // (the capacity rule is symmetric along a shared edge: equal cuts and densities
    mix_f64(grid->cell_size);      //  give matching ends)
    mix_f64(grid->width);
    mix_f64(grid->height);
    const int key = (int)((h ^ (h >> 32)) & 0x3FFFFFFFull);
    int pair_host[2] = {key, -key};
    if (m->use_rccl) {
      DevBuf<int> pair_mem;
      if (pair_mem.alloc(2) != hipSuccess) return bad(m, "cs_mesh_create: HIP error");
      int* pair_dev = pair_mem.get();
      if (hipMemcpyAsync(pair_dev, pair_host, sizeof(pair_host), hipMemcpyHostToDevice, m->stream) != hipSuccess)
        return bad(m, "cs_mesh_create: HIP error");
      const int rc = cs_allreduce_max_i32_rccl(m->tiles[0], pair_dev, 2);
      if (!rc && (hipMemcpyAsync(pair_host, pair_dev, sizeof(pair_host), hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
                  hipStreamSynchronize(m->stream) != hipSuccess))
        return bad(m, "cs_mesh_create: HIP error");
      if (rc) return bad(m, std::string("cs_mesh_create: ") + cs_last_error(m->tiles[0]));
    } else if (m->host.allreduce_max_i32(m->host.user, pair_host, 2)) {
      return bad(m, "cs_mesh_create: the host transport's allreduce_max_i32 failed");
    }
    if (pair_host[0] != key || pair_host[1] != -key)
      return bad(m, "cs_mesh_create: the ranks of this mesh were given different grids, cuts, halo widths or densities "
                    "(every rank passes the same cs_grid_desc and cs_mesh_desc but for `rank` and the device)");
  }
  if (hipStreamSynchronize(m->stream) != hipSuccess) return bad(m, "cs_mesh_create: HIP error");
  m->id_bound = m->tiles.empty() ? 0 : m->tiles[0]->next_id;
  return m;
}

void cs_mesh_destroy(cs_mesh* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->stream) hipStreamSynchronize(m->stream);
  for (cs_engine* e : m->tiles) cs_destroy(e);
  if (m->stream) hipStreamDestroy(m->stream);
  delete m;  // (its members free the halo, staging and flag buffers: the device is current, the stream was waited for)
}

const char* cs_mesh_last_error(const cs_mesh* m) { return m ? m->error.c_str() : g_mesh_create_error.c_str(); }
size_t cs_mesh_local_tiles(const cs_mesh* m) { return m->tiles.size(); }
cs_engine* cs_mesh_tile(cs_mesh* m, size_t local) { return local < m->tiles.size() ? m->tiles[local] : nullptr; }
int cs_mesh_tile_rect(const cs_mesh* m, size_t local, uint32_t* rect4) {
  if (local >= m->tiles.size()) return 3;
  m->rect(m->index_of[local], &rect4[0], &rect4[1], &rect4[2], &rect4[3]);
  return 0;
}

// planners: every tile registers every planner in the same order, so the handles agree
#define CS_MESH_REGISTER(call)                                                            \
  uint32_t handle = UINT32_MAX;                                                           \
  for (cs_engine* e : m->tiles) {                                                         \
    const uint32_t h = (call);                                                            \
    if (h == UINT32_MAX || (handle != UINT32_MAX && h != handle)) {                       \
      m->error = h == UINT32_MAX ? cs_last_error(e) : "the tiles of a mesh disagree on a planner handle"; \
      return UINT32_MAX;                                                                  \
    }                                                                                     \
    handle = h;                                                                           \
  }                                                                                       \
  return handle;
uint32_t cs_mesh_register_zanlungo(cs_mesh* m, const cs_zanlungo_params* p) { CS_MESH_REGISTER(cs_register_zanlungo(e, p)) }
uint32_t cs_mesh_register_no_local_plan(cs_mesh* m) { CS_MESH_REGISTER(cs_register_no_local_plan(e)) }
uint32_t cs_mesh_register_hlp(cs_mesh* m, const cs_hlp_desc* d) { CS_MESH_REGISTER(cs_register_hlp(e, d)) }
uint32_t cs_mesh_register_lp_callback(cs_mesh* m, cs_lp_batch_fn fn, void* user) {
  m->host_planner = true;  // (its answers must reach the device before the step integrates: the host path, every step)
  CS_MESH_REGISTER(cs_register_lp_callback(e, fn, user))
}
#undef CS_MESH_REGISTER

// Simulation::add_agents: every tile sees the global list and keeps what it owns (ids are allocated for all of it)
int cs_mesh_add_agents(cs_mesh* m, const double* xy, size_t n, uint32_t hlp, uint32_t lp, double eyesight, uint64_t* out_ids) {
  if (m->dead()) return m->poison_rc;
  // EVERY tile takes the call, also when it fails: the agents before the failing one stay added (lib.rs:146-149) and
  // every tile's id counter moves alike (the loop used to leave at the first tile that reported the failure: the tiles
  // behind it missed the agents before the failing one)
  if (int rc = mesh_ids_room(m, n)) return rc;
  int first = 0;
  cs_engine* failed = nullptr;
  for (cs_engine* e : m->tiles)
    if (int rc = cs_add_agents(e, xy, n, hlp, lp, eyesight, out_ids))
      if (!first) first = rc, failed = e;
  if (!first) return 0;
  if (first == 1 && failed->last_failed_add_index < n) {
    cs_mesh::Limbo l;
    std::memset(&l.view, 0, sizeof l.view);
    l.view.id = failed->last_failed_add_id;
    l.view.x = xy[2 * failed->last_failed_add_index];
    l.view.y = xy[2 * failed->last_failed_add_index + 1];
    l.view.eyesight_range = eyesight;
    l.hlp = hlp;
    l.lp = lp;
    m->limbo.push_back(l);
  }
  return m->fail(failed, first);
}

// every tile registers every sink; the owner of the source spawns
uint32_t cs_mesh_add_source_sink(cs_mesh* m, const cs_source_sink_desc* d) {
  if (m->dead()) return UINT32_MAX;
  uint32_t handle = UINT32_MAX;
  for (cs_engine* e : m->tiles) {
    handle = cs_add_source_sink(e, d);
    if (handle == UINT32_MAX) {
      m->error = cs_last_error(e);
      return UINT32_MAX;
    }
  }
  m->has_sinks = true;
  const cs_hlp_desc& h = m->tiles[0]->hlps[d->hlp];
  const bool legs = h.kind == CS_HLP_ROUTE && d->n_waypoints > 1;  // later legs may miss the route book
  m->route_legs = m->route_legs || legs;
  m->host_planner = m->host_planner || h.kind == CS_HLP_CALLBACK || legs;
  return handle;
}
void cs_mesh_remove_source_sink(cs_mesh* m, uint32_t handle) {
  for (cs_engine* e : m->tiles) cs_remove_source_sink(e, handle);
}

// Simulation::remove_agents: between steps every agent is held by exactly one tile.  0 = removed, 2 = no local tile
// holds it.  A distributed mesh answers for the whole crowd: 0 on every rank if some rank held the agent (collective).
int cs_mesh_remove_agent(cs_mesh* m, uint64_t id) {
  if (m->dead()) return m->poison_rc;
  for (size_t k = 0; k < m->limbo.size(); ++k)
    if (m->limbo[k].view.id == id) {  // (the same list on every rank: no collective needed)
      cs_engine* e = m->tiles[0];
      const cs_hlp_desc& p = e->hlps[m->limbo[k].hlp];
      if (p.kind == CS_HLP_CALLBACK && p.remove_agent && m->rank == 0) p.remove_agent(p.user, id);
      m->limbo.erase(m->limbo.begin() + (long)k);
      if (m->recording && m->rank == 0) {
        cs_event ev;
        ev.kind = CS_EVENT_DESTROYED;
        ev.source_sink = UINT32_MAX;
        ev.id = id;
        ev.x = ev.y = 0;
        e->events.push_back(ev);
      }
      return 0;
    }
  int out = 2;
  for (cs_engine* e : m->tiles) {
    const int rc = cs_remove_agent(e, id);
    if (rc == 0) out = 0;
    else if (rc != 2) return m->fail(e, rc);
  }
  if (m->distributed) {
    int32_t found = out == 0 ? 1 : 0;
    if (int rc = mesh_allreduce_max(m, &found, 1)) return rc;
    out = found ? 0 : 2;
  }
  if (out == 2) m->error = "unknown agent id";
  return out;
}

void cs_mesh_event_recording(cs_mesh* m, int on) {
  m->recording = on != 0;
  for (cs_engine* e : m->tiles) cs_event_recording(e, on);
}
// events of the local tiles, tile by tile (spawns in sink order inside a tile)
size_t cs_mesh_drain_events(cs_mesh* m, cs_event* out, size_t cap) {
  size_t n = 0;
  for (cs_engine* e : m->tiles) n += cs_drain_events(e, out + n, cap - n);
  return n;
}

// The exchanges below run their local parts (pack, unpack) only while `*rc` is 0, i.e. while no local tile has failed in
// this step, and note the first failure there; what other ranks take part in (the transport) runs regardless, so that
// a failing rank cannot leave its peers waiting.  A failure of the transport itself is returned (fatal).
static void mesh_note(cs_mesh* m, cs_engine* e, int r, int* rc, std::string* why) {
  (void)m;
  if (r && !*rc) {
    *rc = r;
    *why = cs_last_error(e);
  }
}

static int mesh_exchange_local(cs_mesh* m, int* rc, std::string* why) {
  for (cs_engine* e : m->tiles)
    if (!*rc) mesh_note(m, e, cs_halo_pack_all(e), rc, why);
  if (*rc) return 0;
  hipSetDevice(m->device);
  for (size_t k = 0; k < m->tiles.size(); ++k)
    for (int d = 0; d < 8; ++d) {
      const cs_mesh::Buf& b = m->bufs[k][d];
      if (!b.send.get()) continue;
      const int peer = m->local_of((uint32_t)m->neighbour(m->index_of[k], d));
      const cs_mesh::Buf& r = m->bufs[(size_t)peer][cs_mesh::opposite(d)];
      if (hipMemcpyAsync(r.recv.get(), b.send.get(), ((size_t)b.cap + 1u) * CS_HALO_RECORD_BYTES, hipMemcpyDeviceToDevice, m->stream) !=
          hipSuccess) {
        m->error = "HIP error in the halo exchange";
        return 90;
      }
    }
  for (cs_engine* e : m->tiles)
    if (!*rc) mesh_note(m, e, cs_halo_unpack_all(e), rc, why);
  return 0;
}

// pack -> device to host -> the host's exchange -> host to device -> unpack
static int mesh_exchange_host(cs_mesh* m, int* rc, std::string* why) {
  cs_engine* e = m->tiles[0];
  if (!*rc) mesh_note(m, e, cs_halo_pack_all(e), rc, why);
  hipSetDevice(m->device);
  int32_t peers[8], stag[8], rtag[8];
  const void* sp[8];
  void* rp[8];
  size_t bytes[8];
  size_t n = 0;
  for (int d = 0; d < 8; ++d) {
    const cs_mesh::Buf& b = m->bufs[0][d];
    if (!b.send.get()) continue;
    if (hipMemcpyAsync(m->stage_send[d].get(), b.send.get(), m->stage_send[d].bytes(), hipMemcpyDeviceToHost, m->stream) != hipSuccess) {
      m->error = "HIP error in the halo exchange";
      return 90;
    }
    peers[n] = m->neighbour(m->index_of[0], d);
    stag[n] = d;
    rtag[n] = cs_mesh::opposite(d);
    sp[n] = m->stage_send[d].get();
    rp[n] = m->stage_recv[d].get();
    bytes[n] = m->stage_send[d].bytes();
    ++n;
  }
  if (hipStreamSynchronize(m->stream) != hipSuccess) {
    m->error = "HIP error in the halo exchange";
    return 90;
  }
  if (m->host.exchange(m->host.user, n, peers, stag, rtag, sp, rp, bytes)) return mesh_host_fail(m, "exchange");
  for (int d = 0; d < 8; ++d) {
    const cs_mesh::Buf& b = m->bufs[0][d];
    if (!b.send.get()) continue;
    if (hipMemcpyAsync(b.recv.get(), m->stage_recv[d].get(), m->stage_recv[d].bytes(), hipMemcpyHostToDevice, m->stream) != hipSuccess) {
      m->error = "HIP error in the halo exchange";
      return 90;
    }
  }
  if (!*rc) mesh_note(m, e, cs_halo_unpack_all(e), rc, why);
  return 0;
}

// One step of the whole crowd (lib.rs:195-383 on every tile): halo exchange, spawn flags OR-ed over the tiles,
// cs_step, route-cache misses planned by every tile in agent order.  report (may be null): summed over the LOCAL
// tiles.  n_ranks > 1: collective (every rank calls it).
// Failure: the step phase runs on EVERY local tile whatever the others return; in the distributed forms the ranks
// agree on "somebody failed" before anybody leaves (after the step when the host waits for it anyway, every
// `check_every` steps when it does not); any failure stops the mesh on every rank (cs_mesh::poison).
int cs_mesh_step(cs_mesh* m, double dt, cs_step_report* report) {
  if (report) std::memset(report, 0, sizeof *report);
  if (m->dead()) return m->poison_rc;
  if (!m->limbo.empty()) {  // lib.rs:299-302, on every rank alike; nothing has been stepped, the mesh goes on once it is removed
    m->error = "Index out of bounds";
    return 1;
  }
  if (m->flags & CS_CFG_WIDE_IDS)  // (at most one spawn per source-sink slot and step)
    if (int rc = mesh_ids_room(m, m->has_sinks ? (uint64_t)cs_source_sink_slots(m->tiles[0]) : 0u)) return rc;
  auto add = [&](const cs_step_report& r) {
    if (!report) return;
    report->n_agents += r.n_agents; report->n_spawned += r.n_spawned; report->n_destroyed += r.n_destroyed;
    report->n_waypoint_hits += r.n_waypoint_hits; report->n_tti_zero += r.n_tti_zero; report->n_nonfinite += r.n_nonfinite;
    report->n_clamped += r.n_clamped;
  };
  const bool host_path = report != nullptr || m->host_planner || m->recording;
  // the spawn flags cross the ranks on the host when the host brings the transport
  const bool host_flags = host_path || (m->distributed && !m->use_rccl);

  // agreement on a failure through the halo headers (cs_mesh::header_agree): the forms in which nobody asked for this
  // step's outcome; with a report, listeners or host planners the ranks agree in the step itself (mesh_agree below)
  const bool headers = m->distributed && !host_path && m->header_agree && m->n_ranks > 1;
  for (cs_engine* e : m->tiles) e->mesh_step_tag = headers ? m->step_tag() : 0u;

  if (m->distributed && m->use_rccl && !host_path) {
    // nothing needs the host between the phases: the whole step is one call into the engine, nobody waits for the
    // device, and a failure is acted on at the agreed step (the halo headers), or at the next agreed check
    cs_engine* e = m->tiles[0];
    e->no_exchange_ahead = false;
    if (headers) {
      // a rank that still steps sees its device as it was when the step kernel of kFlight steps ago started (the
      // third pinned word); one that has failed reads the word itself after every exchange
      if (!m->deferred_rc) {
        e->flight_throttle();
        m->fail_word = e->peek_mesh_fail();
      }
      bool last = false;
      if (mesh_past_the_agreed_stop(m, m->fail_word, cs_engine::kFlight + 1u, &last))
        return mesh_stop(m, m->deferred_rc, m->deferred_error);
      e->no_exchange_ahead = last;  // (the exchange a step makes ahead belongs to the NEXT step, which nobody will take)
    }
    if (!m->deferred_rc) {
      if (const int rc = cs_tile_step_rccl(e, dt, nullptr)) {
        m->deferred_rc = rc;
        m->deferred_error = cs_last_error(e);
        if (const int z = tile_zombie_collectives(e, e->step_colls)) return m->poison(z, cs_last_error(e));
      }
    } else if (const int z = tile_zombie_collectives(e, 0u)) {
      return m->poison(z, cs_last_error(e));
    }
    if (headers && m->deferred_rc)  // (no unpack runs on a failed tile: forward the neighbours' words, add its own)
      if (const int r = mesh_fail_word_now(m, m->step_tag(), &m->fail_word)) return r;
    m->step_index += 1;
    if (++m->steps_since_check >= m->check_every) {
      m->steps_since_check = 0;
      return mesh_agree(m, m->deferred_rc, m->deferred_error);
    }
    return 0;
  }

  int rc = 0;  // the first failure of a local tile in this step
  std::string why;
  auto fatal = [&](int r) { return m->poison(r, m->error); };  // the transport itself failed: no agreement possible
  if (headers) {
    // (the host waits for every step of this form: it knows the word as the last unpack left it, lag 0)
    bool last = false;
    if (mesh_past_the_agreed_stop(m, m->fail_word, 0u, &last)) return mesh_stop(m, m->deferred_rc, m->deferred_error);
    rc = m->deferred_rc;  // a rank that has failed keeps only the transports company from here on
    why = m->deferred_error;
  }
  if (m->distributed && m->use_rccl) {
    cs_engine* e = m->tiles[0];
    mesh_note(m, e, cs_halo_pack_all(e), &rc, &why);
    if (int r = cs_halo_exchange_rccl(e, -1)) return fatal(m->fail(e, r));
    if (!rc) mesh_note(m, e, cs_halo_unpack_all(e), &rc, &why);
  } else if (m->distributed) {
    if (int r = mesh_exchange_host(m, &rc, &why)) return fatal(r);
  } else {
    if (int r = mesh_exchange_local(m, &rc, &why)) return fatal(r);
  }
  if (m->has_sinks) {
    const size_t ns = cs_source_sink_slots(m->tiles[0]);
    hipSetDevice(m->device);
    if (ns > m->flag_cap || m->flag_bufs.size() != m->tiles.size()) {
      hipStreamSynchronize(m->stream);
      m->flag_bufs.clear();
      m->flag_bufs.resize(m->tiles.size());
      m->flag_cap = 0;
      const size_t cap = 2 * ns + 64;
      for (DevBuf<int>& f : m->flag_bufs)
        if (f.alloc(cap) != hipSuccess || hipMemsetAsync(f.get(), 0, cap * sizeof(int), m->stream) != hipSuccess) {
          m->error = "HIP error while allocating spawn flags";
          return fatal(90);
        }
      m->flag_cap = cap;
    }
    if (!host_flags) {  // flags stay on the device (in-process form)
      for (size_t k = 0; k < m->tiles.size(); ++k)
        if (!rc) mesh_note(m, m->tiles[k], cs_spawn_probe_dev(m->tiles[k], dt, m->flag_bufs[k].get(), ns), &rc, &why);
      if (!rc)
        for (size_t k = 1; k < m->tiles.size(); ++k)
          hipLaunchKernelGGL(k_i32_max, dim3((uint32_t)((ns + 255) / 256)), dim3(256), 0, m->stream, m->flag_bufs[0].get(),
                             m->flag_bufs[k].get(), (uint32_t)ns);
      for (cs_engine* e : m->tiles)
        if (!rc) mesh_note(m, e, cs_spawn_commit_dev(e, m->flag_bufs[0].get(), ns), &rc, &why);
    } else {
      std::vector<uint8_t> all(std::max<size_t>(ns, 1), 0), mine(std::max<size_t>(ns, 1), 0);
      for (cs_engine* e : m->tiles) {
        if (rc) break;
        if (cs_spawn_probe(e, dt, mine.data(), ns) == SIZE_MAX) mesh_note(m, e, 1, &rc, &why);
        else
          for (size_t s = 0; s < ns; ++s) all[s] |= mine[s];
      }
      if (m->distributed && !m->use_rccl) {  // OR over the ranks: the host's all-reduce (max)
        std::vector<int32_t> host(std::max<size_t>(ns, 1), 0);
        for (size_t s = 0; s < ns; ++s) host[s] = all[s];
        if (m->host.allreduce_max_i32(m->host.user, host.data(), ns)) return fatal(mesh_host_fail(m, "allreduce_max_i32"));
        for (size_t s = 0; s < ns; ++s) all[s] = host[s] ? 1 : 0;
      } else if (m->distributed) {  // OR over the ranks: one small all-reduce (max) of device ints
        std::vector<int> host(std::max<size_t>(ns, 1), 0);
        for (size_t s = 0; s < ns; ++s) host[s] = all[s];
        if (hipMemcpyAsync(m->flag_bufs[0].get(), host.data(), ns * sizeof(int), hipMemcpyHostToDevice, m->stream) != hipSuccess)
          return fatal(90);
        if (int r = cs_allreduce_max_i32_rccl(m->tiles[0], m->flag_bufs[0].get(), ns)) return fatal(m->fail(m->tiles[0], r));
        if (hipMemcpyAsync(host.data(), m->flag_bufs[0].get(), ns * sizeof(int), hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
            hipStreamSynchronize(m->stream) != hipSuccess)
          return fatal(90);
        for (size_t s = 0; s < ns; ++s) all[s] = host[s] ? 1 : 0;
      }
      for (cs_engine* e : m->tiles)
        if (!rc) mesh_note(m, e, cs_spawn_commit(e, all.data(), ns), &rc, &why);
    }
  }
  // the step phase: every local tile is asked, whatever the tiles before it answered (a tile that fails rolls back
  // only itself; the others' answers decide nothing any more, but their error state must not depend on the order)
  if (!rc)
    for (cs_engine* e : m->tiles) {
      cs_step_report r;
      std::memset(&r, 0, sizeof r);
      if (const int step_rc = cs_step(e, dt, host_path ? &r : nullptr)) mesh_note(m, e, step_rc, &rc, &why);
      else add(r);
    }
  if (m->route_legs) {
    // legs of route followers that missed the route book on any tile: every tile plans them, in agent order, so
    // that all books number routes alike (n_ranks > 1: gathered over the ranks first)
    std::vector<cs_route_miss> misses;
    for (cs_engine* e : m->tiles) {
      const size_t k = rc ? 0 : cs_route_misses(e, nullptr, 0);
      if (!k) continue;
      const size_t at = misses.size();
      misses.resize(at + k);
      cs_route_misses(e, misses.data() + at, k);
    }
    if (m->distributed) {
      std::vector<std::vector<unsigned char>> parts;
      if (int r = mesh_host_gatherv(m, misses.data(), misses.size() * sizeof(cs_route_miss), parts)) return fatal(r);
      misses.clear();
      for (const auto& part : parts) {
        const size_t k = part.size() / sizeof(cs_route_miss), at = misses.size();
        misses.resize(at + k);
        if (k) std::memcpy(misses.data() + at, part.data(), k * sizeof(cs_route_miss));
      }
    }
    if (!misses.empty() && !rc) {
      std::sort(misses.begin(), misses.end(), [](const cs_route_miss& a, const cs_route_miss& b) {
        return std::tie(a.id, a.hlp, a.slot) < std::tie(b.id, b.hlp, b.slot);
      });
      for (cs_engine* e : m->tiles)
        if (!rc) mesh_note(m, e, cs_route_resolve(e, misses.data(), misses.size()), &rc, &why);
    }
  }
  if (headers) {
    if (rc && !m->deferred_rc) {
      m->deferred_rc = rc;
      m->deferred_error = why;
    }
    // the word after this step's exchange: merged by the unpack (or here, on a failed tile), read back
    if (const int r = mesh_fail_word_now(m, m->deferred_rc ? m->step_tag() : 0u, &m->fail_word)) return r;
    m->step_index += 1;
    if (++m->steps_since_check >= m->check_every) {  // the backstop
      m->steps_since_check = 0;
      return mesh_agree(m, m->deferred_rc, m->deferred_error);
    }
    return 0;
  }
  m->step_index += 1;
  if (m->distributed) return mesh_agree(m, rc, why);  // everybody learns of anybody's failure before anybody leaves
  return rc ? m->poison(rc, why) : 0;
}

// Waits for the device and surfaces what the steps made without a report have left behind.  Distributed forms:
// collective, and an agreed check (every rank learns of any rank's failure).
int cs_mesh_synchronize(cs_mesh* m) {
  if (m->dead()) return m->poison_rc;
  int rc = m->deferred_rc;
  std::string why = m->deferred_error;
  for (cs_engine* e : m->tiles)
    if (!rc)
      if (int r = cs_synchronize(e)) {
        rc = r;
        why = cs_last_error(e);
      }
  if (m->distributed) {
    m->steps_since_check = 0;
    return mesh_agree(m, rc, why);
  }
  return rc ? m->poison(rc, why) : 0;
}

// agents of the crowd: held by the local tiles (n_ranks == 1: the crowd), and summed over the ranks when the host
// brought a transport (collective then)
size_t cs_mesh_agent_count(cs_mesh* m) {
  if (m->dead()) return SIZE_MAX;
  size_t n = 0;
  for (cs_engine* e : m->tiles) n += cs_agent_count(e);
  if (m->distributed) {
    const uint64_t mine = n;
    std::vector<uint64_t> all((size_t)m->n_ranks, 0);
    if (mesh_allgather(m, &mine, sizeof mine, all.data())) return SIZE_MAX;
    n = 0;
    for (uint64_t v : all) n += (size_t)v;
  }
  return n + m->limbo.size();
}
// ... as the reference's `agents`, ascending id (lib.rs:71); the whole crowd on every rank when the host brought a
// transport or RCCL carries the gather (collective)
size_t cs_mesh_read_agents(cs_mesh* m, cs_agent_view* out, size_t cap) {
  if (m->dead()) return SIZE_MAX;
  const bool gather = m->distributed;
  std::vector<cs_agent_view> local;
  size_t n = 0;
  for (cs_engine* e : m->tiles) {
    const size_t k = cs_agent_count(e);
    if (gather) local.resize(n + k);
    else if (n + k > cap) return SIZE_MAX;
    cs_agent_view* dst = gather ? local.data() + n : out + n;
    if (cs_read_agents(e, dst, k) != k) {
      m->error = cs_last_error(e);
      return SIZE_MAX;
    }
    n += k;
  }
  if (gather) {
    std::vector<std::vector<unsigned char>> parts;
    if (mesh_host_gatherv(m, local.data(), n * sizeof(cs_agent_view), parts)) return SIZE_MAX;
    n = 0;
    for (const auto& part : parts) n += part.size() / sizeof(cs_agent_view);
    if (n > cap) {
      m->error = "cs_mesh_read_agents: the buffer is smaller than the crowd";
      return SIZE_MAX;
    }
    size_t at = 0;
    for (const auto& part : parts) {
      if (!part.empty()) std::memcpy(out + at, part.data(), part.size());
      at += part.size() / sizeof(cs_agent_view);
    }
  }
  for (const cs_mesh::Limbo& l : m->limbo) {
    if (n >= cap) return SIZE_MAX;
    out[n++] = l.view;
  }
  std::sort(out, out + n, [](const cs_agent_view& a, const cs_agent_view& b) { return a.id < b.id; });
  return n;
}

// bytes the local tiles send per step (the fixed-capacity halo buffers of every direction with a neighbour: the
// record count travels in the header, so the message size does not depend on the crowd)
uint64_t cs_mesh_exchange_bytes(const cs_mesh* m) {
  uint64_t bytes = 0;
  for (const auto& eight : m->bufs)
    for (const auto& b : eight)
      if (b.send.get()) bytes += ((uint64_t)b.cap + 1u) * CS_HALO_RECORD_BYTES;
  return bytes;
}

// agents owned per local tile, in local order
int cs_mesh_tile_counts(cs_mesh* m, uint64_t* out) {
  for (size_t k = 0; k < m->tiles.size(); ++k) out[k] = cs_agent_count(m->tiles[k]);
  return 0;
}

// Move the cuts to the quantiles of where the crowd stands NOW (a clustered crowd drifts: BASELINE.json configs[4]);
// between two steps; the state, and so every later step, is unchanged bit for bit.  A distributed mesh needs the
// gathers for it (the histograms and the exported records of every rank reach every rank: collective).
int cs_mesh_recut(cs_mesh* m) {
  if (m->dead()) return m->poison_rc;
  std::vector<uint64_t> rows(m->rows, 0), cols(m->cols, 0);
  for (cs_engine* e : m->tiles)
    if (int rc = cs_tile_histogram(e, rows.data(), cols.data())) return m->fail(e, rc);
  if (m->distributed) {  // sum over the ranks
    std::vector<uint64_t> mine(rows);
    mine.insert(mine.end(), cols.begin(), cols.end());
    std::vector<uint64_t> all(mine.size() * (size_t)m->n_ranks);
    if (int rc = mesh_allgather(m, mine.data(), mine.size() * sizeof(uint64_t), all.data())) return rc;
    std::fill(rows.begin(), rows.end(), 0);
    std::fill(cols.begin(), cols.end(), 0);
    for (size_t r = 0; r < (size_t)m->n_ranks; ++r) {
      const uint64_t* part = all.data() + r * mine.size();
      for (size_t k = 0; k < rows.size(); ++k) rows[k] += part[k];
      for (size_t k = 0; k < cols.size(); ++k) cols[k] += part[rows.size() + k];
    }
  }
  std::vector<double> hx(rows.begin(), rows.end()), hy(cols.begin(), cols.end());
  // the new cuts replace the old ones only once they are known to be good: until then (and after a refusal) the
  // mesh's rectangles are those its tiles have
  const std::vector<uint32_t> old_x = m->x_edges, old_y = m->y_edges;
  m->x_edges = mesh_weighted_edges(hx, m->tiles_x, 2 * m->halo);
  m->y_edges = mesh_weighted_edges(hy, m->tiles_y, 2 * m->halo);
  if (!mesh_edges_ok(m)) {
    m->x_edges = old_x;
    m->y_edges = old_y;
    m->error = "cs_mesh_recut: a tile would be thinner than two halo rings";
    return 3;
  }
  auto keep_old = [&](int rc) {  // nothing has been moved yet
    m->x_edges = old_x;
    m->y_edges = old_y;
    return rc;
  };
  // from the first retile on a failure leaves tiles with different cuts (or without their agents): the mesh stops
  auto broken = [&](cs_engine* e, int rc) { return m->poison(rc, std::string("cs_mesh_recut failed half way: ") + (e ? cs_last_error(e) : m->error.c_str())); };
  std::vector<std::vector<unsigned char>> exports(m->tiles.size());
  std::vector<size_t> counts(m->tiles.size(), 0);
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    const size_t n = cs_tile_export(m->tiles[k], nullptr, 0);
    if (n == SIZE_MAX) return keep_old(m->fail(m->tiles[k], 1));
    exports[k].resize(std::max<size_t>(n, 1) * CS_HALO_RECORD_BYTES);
    counts[k] = std::min(n, cs_tile_export(m->tiles[k], exports[k].data(), n));
  }
  if (m->distributed) {  // what every rank exported reaches every rank; each keeps what its new rectangle owns
    std::vector<std::vector<unsigned char>> parts;
    if (int rc = mesh_host_gatherv(m, exports[0].data(), counts[0] * CS_HALO_RECORD_BYTES, parts)) return m->poison(rc, m->error);
    exports = std::move(parts);
    counts.assign(exports.size(), 0);
    for (size_t k = 0; k < exports.size(); ++k) counts[k] = exports[k].size() / CS_HALO_RECORD_BYTES;
  }
  hipSetDevice(m->device);
  hipStreamSynchronize(m->stream);
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    uint32_t x0, x1, y0, y1;
    m->rect(m->index_of[k], &x0, &x1, &y0, &y1);
    if (int rc = cs_tile_retile(m->tiles[k], x0, x1, y0, y1)) return broken(m->tiles[k], rc);
    if (int rc = mesh_set_buffers(m, k)) return broken(nullptr, rc);
  }
  if (m->distributed && !m->use_rccl)
    if (int rc = mesh_host_stage_alloc(m)) return broken(nullptr, rc);
  hipStreamSynchronize(m->stream);
  for (cs_engine* e : m->tiles)
    for (size_t k = 0; k < exports.size(); ++k)
      if (counts[k])
        if (int rc = cs_tile_import(e, exports[k].data(), counts[k])) return broken(e, rc);
  return 0;
}

// SpatialIndex on a mesh (spatial_index.rs:4-14): every tile answers for the agents it holds; the answers are
// merged into the reference's order (cells x-major / y-minor by global cell number, ascending id inside a cell).
// A distributed mesh merges over the ranks when the host brought a transport (collective: every rank asks the same
// queries and gets the whole answer).  out_ids: cap_per_query per
// query; out_counts: full counts.
int cs_mesh_query_radius_batch(cs_mesh* m, size_t n, const double* xy, const double* radius, size_t cap, uint64_t* out_ids,
                               uint64_t* out_counts) {
  if (m->dead()) return m->poison_rc;
  struct Hit {
    uint32_t cell;
    uint64_t id;
  };
  std::vector<std::vector<Hit>> hits(n);
  std::vector<uint64_t> ids(n * cap), counts(n);
  std::vector<uint32_t> cells(n * cap);
  for (cs_engine* e : m->tiles) {
    size_t tile_cap = cap;
    for (;;) {  // (a tile may hold more of an answer than the caller's buffer has room for: the merged head matters)
      ids.assign(n * tile_cap, 0);
      cells.assign(n * tile_cap, 0);
      if (int rc = cs_query_radius_batch(e, n, xy, radius, tile_cap, ids.data(), counts.data(), nullptr, cells.data()))
        return m->fail(e, rc);
      uint64_t most = 0;
      for (size_t q = 0; q < n; ++q) most = std::max(most, counts[q]);
      if (most <= tile_cap) break;
      tile_cap = (size_t)most;
    }
    for (size_t q = 0; q < n; ++q)
      for (size_t k = 0; k < counts[q]; ++k) hits[q].push_back(Hit{cells[q * tile_cap + k], ids[q * tile_cap + k]});
  }
  if (m->distributed) {  // every rank's hits reach every rank (collective; same queries everywhere)
    struct Wire {
      uint32_t q, cell;
      uint64_t id;
    };
    std::vector<Wire> mine;
    for (size_t q = 0; q < n; ++q)
      for (const Hit& h : hits[q]) mine.push_back(Wire{(uint32_t)q, h.cell, h.id});
    std::vector<std::vector<unsigned char>> parts;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(Wire), parts)) return rc;
    for (auto& v : hits) v.clear();
    for (const auto& part : parts)
      for (size_t k = 0; k + sizeof(Wire) <= part.size(); k += sizeof(Wire)) {
        Wire w;
        std::memcpy(&w, part.data() + k, sizeof w);
        if (w.q < n) hits[w.q].push_back(Hit{w.cell, w.id});
      }
  }
  for (size_t q = 0; q < n; ++q) {
    std::sort(hits[q].begin(), hits[q].end(), [](const Hit& a, const Hit& b) { return std::tie(a.cell, a.id) < std::tie(b.cell, b.id); });
    if (out_counts) out_counts[q] = hits[q].size();
    for (size_t k = 0; k < hits[q].size() && k < cap; ++k) out_ids[q * cap + k] = hits[q][k].id;
  }
  return 0;
}

// k nearest over the tiles: every tile's k nearest held agents, merged by (distance, id)
int cs_mesh_query_knn_batch(cs_mesh* m, size_t n, const double* xy, size_t k, uint64_t* out_ids, uint64_t* out_counts) {
  if (m->dead()) return m->poison_rc;
  struct Hit {
    float d2;
    uint64_t id;
  };
  std::vector<std::vector<Hit>> hits(n);
  std::vector<uint64_t> ids(n * k), counts(n);
  std::vector<float> d2(n * k);
  for (cs_engine* e : m->tiles) {
    if (int rc = cs_query_knn_batch(e, n, xy, k, ids.data(), counts.data(), d2.data())) return m->fail(e, rc);
    for (size_t q = 0; q < n; ++q)
      for (size_t j = 0; j < counts[q] && j < k; ++j) hits[q].push_back(Hit{d2[q * k + j], ids[q * k + j]});
  }
  if (m->distributed) {  // every rank's candidates reach every rank (collective)
    struct Wire {
      uint32_t q;
      float d2;
      uint64_t id;
    };
    std::vector<Wire> mine;
    for (size_t q = 0; q < n; ++q)
      for (const Hit& h : hits[q]) mine.push_back(Wire{(uint32_t)q, h.d2, h.id});
    std::vector<std::vector<unsigned char>> parts;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(Wire), parts)) return rc;
    for (auto& v : hits) v.clear();
    for (const auto& part : parts)
      for (size_t j = 0; j + sizeof(Wire) <= part.size(); j += sizeof(Wire)) {
        Wire w;
        std::memcpy(&w, part.data() + j, sizeof w);
        if (w.q < n) hits[w.q].push_back(Hit{w.d2, w.id});
      }
  }
  for (size_t q = 0; q < n; ++q) {
    std::sort(hits[q].begin(), hits[q].end(), [](const Hit& a, const Hit& b) { return std::tie(a.d2, a.id) < std::tie(b.d2, b.id); });
    const size_t got = std::min(hits[q].size(), k);
    if (out_counts) out_counts[q] = got;
    for (size_t j = 0; j < got; ++j) out_ids[q * k + j] = hits[q][j].id;
  }
  return 0;
}

}  // extern "C"
