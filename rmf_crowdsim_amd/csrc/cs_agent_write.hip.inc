// cs_agent_write.hip.inc — writing agents between steps, by id (include/crowdstep_state.h)
// Part of the single translation unit crowdstep_hip.hip (included there, after cs_mesh.hip.inc).
//
// The reference's `pub agents` map (lib.rs:71) is written by its host between steps (`agents.get_mut(&id)`); the next
// step works from what was written.  Here a batch of (id, fields) records becomes the START-OF-STEP state of those
// agents (DESIGN.md section 2, "Writing agents between steps"):
//   host     validate, map external ids to device ids, sort by device id (which finds duplicates), place positions with
//            the engine's own to_cell and velocities in f32, upload the batch once
//   K_match  one pass over the slots of buf[cur]: every live slot binary-searches its id in the sorted batch (staged in
//            LDS when it fits) and records its slot; one wave-aggregated atomic per wave counts the matches
//   host     one read back: the match count (and the matched agents' meta words when next_waypoint is written, for the
//            group -> source-sink check); anything short refuses the whole batch, nothing has been changed yet
//   K_apply  one thread per record writes cell, offset, velocity and waypoint bits into its slot; on a mesh a record whose
//            new cell another tile owns leaves as a halo record (the cs_tile_export format) and its slot dies
// The step kernels are not touched: the flags that say "the agents changed between steps" (sorted, hist_valid,
// occ_valid, the kept band windows, halo_invalidate) make the next step sort, recount and re-pack as after add / remove.

#define WRITE_MATCH_BLOCK 256u
#define WRITE_STAGED_BLOCK 1024u
#define WRITE_LDS_BYTES (160u * 1024u)  // the CU's LDS: one workgroup may declare all of it
#define WRITE_STAGED_KEYS_MAX (WRITE_LDS_BYTES / 4u)

// one record of a batch as the device applies it (32 B); `cell` = CS_INVALID_CELL: another tile owns the new cell
struct WriteRec {
  uint32_t cell, gcx, gcy, wp;
  float ox, oy, vx, vy;
};

// index of `id` in the ascending keys, or 0xFFFFFFFF
__device__ __forceinline__ uint32_t write_find(const uint32_t* __restrict__ k, uint32_t n_keys, uint32_t id) {
  uint32_t lo = 0, hi = n_keys;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (k[mid] < id) lo = mid + 1u;
    else hi = mid;
  }
  return (lo < n_keys && k[lo] == id) ? lo : 0xFFFFFFFFu;
}

// K_match.  STAGED: the sorted keys are copied into LDS once per workgroup and the workgroups stride over the slots;
// otherwise each lane searches the keys in global memory (the top levels of the search stay in the caches).
// `owned_only`: a tile whose arrays hold ghosts (a halo exchange ran since its last step) matches only the agents in its
// owned cells, the rule of k_tile_export.  slot_of / meta_of start at 0xFFFFFFFF (a meta word never is: the group
// bits of an engine's groups are never all ones, cs_engine::room_for_group).
template <bool STAGED>
__global__ void __launch_bounds__(STAGED ? WRITE_STAGED_BLOCK : WRITE_MATCH_BLOCK)
    k_write_match(GridDev g, AgentArrays a, uint32_t n_ub, const Counters* __restrict__ ctr, uint32_t tile,
                  uint32_t owned_only, const uint32_t* __restrict__ keys, uint32_t n_keys, uint32_t* __restrict__ slot_of,
                  uint32_t* __restrict__ meta_of, uint32_t* __restrict__ count) {
  extern __shared__ uint32_t s_keys[];
  if (STAGED) {
    for (uint32_t j = threadIdx.x; j < n_keys; j += blockDim.x) s_keys[j] = keys[j];
    __syncthreads();
  }
  const uint32_t limit = tile ? min(n_ub, ctr->n_pending) : n_ub;
  const uint32_t stride = gridDim.x * blockDim.x;
  // (the loop bound is the same for every lane of a workgroup: the ballot below sees whole waves)
  for (uint32_t base = blockIdx.x * blockDim.x; base < limit; base += stride) {
    const uint32_t i = base + threadIdx.x;
    uint32_t r = 0xFFFFFFFFu;
    const uint32_t c = i < limit ? a.cell[i] : CS_INVALID_CELL;
    bool live = c != CS_INVALID_CELL;
    if (live && owned_only) {
      const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
      live = cx >= g.own_x0 && cx < g.own_x1 && cy >= g.own_y0 && cy < g.own_y1;
    }
    if (live) r = STAGED ? write_find(s_keys, n_keys, a.id[i]) : write_find(keys, n_keys, a.id[i]);
    if (r != 0xFFFFFFFFu) {
      slot_of[r] = i;
      if (meta_of) meta_of[r] = a.meta[i];
    }
    const unsigned long long m = __ballot(r != 0xFFFFFFFFu);
    if (m && __lane_id() == __ffsll((long long)m) - 1) atomicAdd(count, (uint32_t)__popcll(m));
  }
}

// K_apply: record r into slot slot_of[r] (below n_slots: checked, whatever the match found).  Movers (a written cell
// another tile owns) are appended to `movers` (room for n records) with the written state, and their slot dies.
__global__ void k_write_apply(GridDev g, AgentArrays a, uint32_t n_slots, const WriteRec* __restrict__ recs,
                              const uint32_t* __restrict__ slot_of, uint32_t n, uint32_t fields,
                              HaloRecord* __restrict__ movers, uint32_t* __restrict__ n_movers) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t i = slot_of[r];
  if (i >= n_slots) return;
  const WriteRec w = recs[r];
  uint32_t meta = a.meta[i];
  if (fields & CS_WRITE_NEXT_WAYPOINT) meta = meta_make(g, meta_group(g, meta), w.wp);
  const float2 vel = (fields & CS_WRITE_VELOCITY) ? make_float2(w.vx, w.vy) : a.vel[i];
  if ((fields & CS_WRITE_POSITION) && w.cell == CS_INVALID_CELL) {
    if (!movers) return;  // (the host refuses such records unless it takes movers)
    HaloRecord h;
    h.ox = w.ox; h.oy = w.oy; h.vx = vel.x; h.vy = vel.y;
    h.id = a.id[i];
    h.meta = meta;
    h.gcx = w.gcx;
    h.gcy = w.gcy;
    h.route = a.route ? a.route[i] : 0u;
    h.reserved = 0u;
    const uint32_t k = atomicAdd(n_movers, 1u);
    if (k < n) movers[k] = h;
    a.cell[i] = CS_INVALID_CELL;
    return;
  }
  if (fields & CS_WRITE_POSITION) {
    a.cell[i] = w.cell;
    a.off[i] = make_float2(w.ox, w.oy);
  }
  if (fields & CS_WRITE_VELOCITY) a.vel[i] = vel;
  if (fields & CS_WRITE_NEXT_WAYPOINT) a.meta[i] = meta;
}

namespace {

// A batch on its way: the records sorted by device id, as the device applies them.
struct WritePlan {
  uint32_t fields = 0;
  std::vector<uint32_t> keys;  // device ids, ascending
  std::vector<WriteRec> recs;  // same order
  std::vector<uint64_t> wp;    // next_waypoint as given (checked against the agent's sink after the match)
  bool any_mover = false;
  // after the match
  uint32_t matched = 0;
  std::vector<uint32_t> meta_of;  // (next_waypoint written) the matched agents' meta words, 0xFFFFFFFF = not here
  // device scratch of the call: [keys | recs] uploaded at once, then slot_of, [count | meta_of], the mover count, movers
  uint32_t* d_keys = nullptr;
  WriteRec* d_recs = nullptr;
  uint32_t* d_slot = nullptr;
  uint32_t* d_words = nullptr;
  uint32_t* d_nmov = nullptr;
  HaloRecord* d_movers = nullptr;
};

constexpr uint32_t kWriteFieldsAll = CS_WRITE_POSITION | CS_WRITE_VELOCITY | CS_WRITE_NEXT_WAYPOINT;

int write_check_mask(std::string* error, uint32_t fields) {
  if (fields == 0u) {
    *error = "write_agents: empty field mask";
    return 3;
  }
  if (fields & ~kWriteFieldsAll) {
    *error = "write_agents: unknown field mask bits";
    return 3;
  }
  return 0;
}

// Host part: validate every record, place it, sort by device id.  `movers`: a tile of a mesh, whose records may land in
// cells other tiles own (else such a record is refused).  Nothing on the device changes here.
int write_prepare(cs_engine* e, const cs_agent_view* in, size_t n, uint32_t fields, bool movers, WritePlan* p) {
  if (int rc = write_check_mask(&e->error, fields)) return rc;
  if (n && !in) {
    e->error = "write_agents: null record array";
    return 3;
  }
  if (n > (size_t)e->id_limit) {  // (more records than ids can be live: some id repeats or is unknown)
    e->error = "unknown agent id";
    return 2;
  }
  p->fields = fields;
  std::vector<std::pair<uint32_t, uint32_t>> order(n);  // (device id, record)
  std::vector<WriteRec> recs(n);
  for (size_t k = 0; k < n; ++k) {
    const cs_agent_view& v = in[k];
    uint64_t dev = 0;
    if (!e->dev_id(v.id, &dev) || dev >= e->id_limit) {
      e->error = "unknown agent id";
      return 2;
    }
    order[k] = {(uint32_t)dev, (uint32_t)k};
    WriteRec& w = recs[k];
    std::memset(&w, 0, sizeof w);
    if (fields & CS_WRITE_POSITION) {
      if (!std::isfinite(v.x) || !std::isfinite(v.y)) {
        e->error = "write_agents: a written position is not finite";
        return 3;
      }
      const int where = e->to_cell(v.x, v.y, &w.cell, &w.ox, &w.oy);
      if (where == 1) {
        e->error = "Index out of bounds";  // what the reference's next step returns for it (lib.rs:299-302)
        return 1;
      }
      if (where == 2) {
        if (!movers) {
          e->error = "write_agents: a written position lies in a cell this tile does not own (only a mesh moves agents between tiles)";
          return 3;
        }
        // the tile branch of to_cell, for a cell another tile owns (to_cell has checked the global bounds)
        const uint64_t xi = sat_usize((v.x - e->grid.offset_x) / e->grid.cell_size);
        const uint64_t yi = sat_usize((v.y - e->grid.offset_y) / e->grid.cell_size);
        w.cell = CS_INVALID_CELL;
        w.gcx = (uint32_t)xi;
        w.gcy = (uint32_t)yi;
        w.ox = (float)((v.x - e->grid.offset_x) - (double)xi * e->grid.cell_size);
        w.oy = (float)((v.y - e->grid.offset_y) - (double)yi * e->grid.cell_size);
        p->any_mover = true;
      }
      if (!std::isfinite(w.ox) || !std::isfinite(w.oy)) {
        e->error = "write_agents: a written position is not finite";
        return 3;
      }
    }
    if (fields & CS_WRITE_VELOCITY) {
      w.vx = (float)v.vx;
      w.vy = (float)v.vy;
      if (!std::isfinite(w.vx) || !std::isfinite(w.vy)) {  // (also a finite f64 beyond the f32 range)
        e->error = "write_agents: a written velocity is not finite";
        return 3;
      }
    }
    if (fields & CS_WRITE_NEXT_WAYPOINT) w.wp = (uint32_t)std::min<uint64_t>(v.next_waypoint, 0xFFFFFFFFull);
  }
  std::sort(order.begin(), order.end());
  for (size_t k = 1; k < n; ++k)
    if (order[k].first == order[k - 1].first) {
      e->error = "write_agents: an agent id appears twice in the batch";
      return 3;
    }
  p->keys.resize(n);
  p->recs.resize(n);
  p->wp.resize(n);
  for (size_t k = 0; k < n; ++k) {
    p->keys[k] = order[k].first;
    p->recs[k] = recs[order[k].second];
    p->wp[k] = in[order[k].second].next_waypoint;
  }
  return 0;
}

// the engine's scratch for calls that address agents by id (the write, and the batched read and remove of
// cs_agents_by_id.hip.inc): grown as needed, never shrunk
int write_scratch_reserve(cs_engine* e, size_t need) {
  if (e->write_scratch.reserve(e->stream, need, Grow::half) != hipSuccess) {
    // (still holding the old scratch: the wait for the stream failed, not the allocation)
    e->error = e->write_scratch.get() ? "HIP error while writing agents" : "HIP error while writing agents (scratch allocation)";
    return 90;
  }
  return 0;
}

int write_scratch(cs_engine* e, WritePlan* p) {
  const size_t n = p->keys.size();
  auto up = [](size_t b) { return (b + 255u) & ~(size_t)255u; };
  const size_t b_keys = up(n * sizeof(uint32_t)), b_recs = up(n * sizeof(WriteRec)), b_slot = up(n * sizeof(uint32_t));
  const size_t b_words = up((n + 1) * sizeof(uint32_t)), b_nmov = 256u;
  const size_t b_mov = p->any_mover ? up(n * sizeof(HaloRecord)) : 0u;
  const size_t need = b_keys + b_recs + b_slot + b_words + b_nmov + b_mov;
  if (int rc = write_scratch_reserve(e, need)) return rc;
  unsigned char* s = static_cast<unsigned char*>(e->write_scratch.get());
  p->d_keys = reinterpret_cast<uint32_t*>(s);
  p->d_recs = reinterpret_cast<WriteRec*>(s + b_keys);
  p->d_slot = reinterpret_cast<uint32_t*>(s + b_keys + b_recs);
  p->d_words = reinterpret_cast<uint32_t*>(s + b_keys + b_recs + b_slot);
  p->d_nmov = reinterpret_cast<uint32_t*>(s + b_keys + b_recs + b_slot + b_words);
  p->d_movers = b_mov ? reinterpret_cast<HaloRecord*>(s + b_keys + b_recs + b_slot + b_words + b_nmov) : nullptr;
  return 0;
}

// K_match of `n` ascending keys against the slots of buf[cur], on the engine's stream (shared with the batched read and
// remove, cs_agents_by_id.hip.inc).  d_slot (and meta_dev, when given) start at 0xFFFFFFFF, *d_count at 0.
void write_launch_match(cs_engine* e, const uint32_t* d_keys, size_t n, uint32_t* d_slot, uint32_t* meta_dev, uint32_t* d_count) {
  const uint32_t owned_only = (e->tile && e->ghosts_present) ? 1u : 0u;
  bool staged = n <= WRITE_STAGED_KEYS_MAX;
  const size_t lds = n * sizeof(uint32_t);
  if (staged && lds > 64u * 1024u &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(k_write_match<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)WRITE_LDS_BYTES) != hipSuccess) {
    (void)hipGetLastError();
    staged = false;  // (search in global memory instead)
  }
  if (staged) {
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || n_cu <= 0) n_cu = 256;
    // (one staging per workgroup: a few workgroups per CU stride over all slots)
    const uint32_t per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(4, WRITE_LDS_BYTES / std::max<size_t>(lds, 1)));
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>((e->n_slots + WRITE_STAGED_BLOCK - 1u) / WRITE_STAGED_BLOCK, (uint64_t)n_cu * per_cu));
    hipLaunchKernelGGL(k_write_match<true>, dim3(blocks), dim3(WRITE_STAGED_BLOCK), lds, e->stream, e->gdev, e->buf[e->cur],
                       e->n_slots, e->ctr.get(), e->tile ? 1u : 0u, owned_only, d_keys, (uint32_t)n, d_slot, meta_dev,
                       d_count);
  } else {
    hipLaunchKernelGGL(k_write_match<false>, dim3((e->n_slots + WRITE_MATCH_BLOCK - 1u) / WRITE_MATCH_BLOCK),
                       dim3(WRITE_MATCH_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], e->n_slots, e->ctr.get(),
                       e->tile ? 1u : 0u, owned_only, d_keys, (uint32_t)n, d_slot, meta_dev, d_count);
  }
}

// The queued steps first (stream order), then upload, K_match and the one read back.  Changes nothing on the device
// but the call's scratch.
int write_match(cs_engine* e, WritePlan* p) {
  if (e->poisoned) {
    e->error = e->poison_error;
    return 1;
  }
  if (int rc = cs_synchronize(e)) return rc;  // (a fire-and-forget step that failed: its Err is the write's)
  const size_t n = p->keys.size();
  p->matched = 0;
  p->meta_of.assign((p->fields & CS_WRITE_NEXT_WAYPOINT) ? n : 0, 0xFFFFFFFFu);
  if (!n || !e->n_slots) return 0;
  if (int rc = write_scratch(e, p)) return rc;
  const bool want_meta = (p->fields & CS_WRITE_NEXT_WAYPOINT) != 0;
  {  // the batch in one upload: keys, then records (the scratch lays them out the same way)
    const size_t b_keys = reinterpret_cast<unsigned char*>(p->d_recs) - reinterpret_cast<unsigned char*>(p->d_keys);
    std::vector<unsigned char> host(b_keys + n * sizeof(WriteRec));
    std::memcpy(host.data(), p->keys.data(), n * sizeof(uint32_t));
    std::memcpy(host.data() + b_keys, p->recs.data(), n * sizeof(WriteRec));
    HIP_OK_E(e, hipMemcpyAsync(p->d_keys, host.data(), host.size(), hipMemcpyHostToDevice, e->stream));
    HIP_OK_E(e, hipMemsetAsync(p->d_slot, 0xFF, n * sizeof(uint32_t), e->stream));
    HIP_OK_E(e, hipMemsetAsync(p->d_words, 0, sizeof(uint32_t), e->stream));
    if (want_meta) HIP_OK_E(e, hipMemsetAsync(p->d_words + 1, 0xFF, n * sizeof(uint32_t), e->stream));
    HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (the host staging dies here)
  }
  write_launch_match(e, p->d_keys, n, p->d_slot, want_meta ? p->d_words + 1 : nullptr, p->d_words);
  HIP_OK_E(e, hipGetLastError());
  std::vector<uint32_t> words(want_meta ? n + 1 : 1);
  HIP_OK_E(e, hipMemcpyAsync(words.data(), p->d_words, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  p->matched = words[0];
  if (want_meta) std::copy(words.begin() + 1, words.end(), p->meta_of.begin());
  return 0;
}

// next_waypoint of every record this engine matched: below its source-sink's number of waypoints while the sink is
// registered, else 0 (the reference never reads it then; the meta word's waypoint bits are as wide as the sinks need)
int write_check_waypoints(cs_engine* e, const WritePlan& p) {
  if (!(p.fields & CS_WRITE_NEXT_WAYPOINT)) return 0;
  for (size_t r = 0; r < p.meta_of.size(); ++r) {
    if (p.meta_of[r] == 0xFFFFFFFFu) continue;  // held elsewhere
    const uint32_t g = meta_group(e->gdev, p.meta_of[r]);
    const int32_t sink = g < e->groups.size() ? e->groups[g].sink : -1;
    const bool live_sink = sink >= 0 && (size_t)sink < e->sinks.size() && e->sinks[(size_t)sink].alive;
    const uint64_t limit = live_sink ? e->sinks[(size_t)sink].waypoints.size() / 2 : 1u;
    if (p.wp[r] >= limit) {
      e->error = "write_agents: next_waypoint out of range for this agent";
      return 3;
    }
  }
  return 0;
}

// K_apply and the flags that make the next step start from the written state.  `movers_out`: what left for other tiles.
int write_apply(cs_engine* e, WritePlan* p, std::vector<HaloRecord>* movers_out) {
  const uint32_t n = (uint32_t)p->keys.size();
  if (!n) return 0;
  if (p->any_mover && p->matched) HIP_OK_E(e, hipMemsetAsync(p->d_nmov, 0, sizeof(uint32_t), e->stream));
  if (p->matched)
    hipLaunchKernelGGL(k_write_apply, dim3((n + 255u) / 256u), dim3(256), 0, e->stream, e->gdev, e->view(e->cur), e->n_slots,
                       p->d_recs, p->d_slot, n, p->fields, p->any_mover ? p->d_movers : nullptr, p->d_nmov);
  HIP_OK_E(e, hipGetLastError());
  uint32_t n_mov = 0;
  if (p->any_mover && p->matched) {
    HIP_OK_E(e, hipMemcpyAsync(&n_mov, p->d_nmov, sizeof n_mov, hipMemcpyDeviceToHost, e->stream));
    HIP_OK_E(e, hipStreamSynchronize(e->stream));
    n_mov = std::min(n_mov, n);
    if (n_mov && movers_out) {
      const size_t at = movers_out->size();
      movers_out->resize(at + n_mov);
      HIP_OK_E(e, hipMemcpy(movers_out->data() + at, p->d_movers, n_mov * sizeof(HaloRecord), hipMemcpyDeviceToHost));
    }
  } else {
    HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (the call's scratch is reused by the next write)
  }
  if (p->matched) {
    e->sorted = false;
    e->hist_valid = false;
    e->occ_valid = false;
    // the kept band windows were cut for the cells of the step before: a written cell voids them (the next step cuts
    // its own in the scatter's launch, as after any change of what they were cut for)
    if (p->fields & CS_WRITE_POSITION) e->windows_valid = false;
    e->n_alive_host -= n_mov;
  }
  e->halo_invalidate();
  return 0;
}

}  // namespace

extern "C" {

int cs_write_agents(cs_engine* e, const cs_agent_view* in, size_t n, uint32_t fields) {
  if (!e) return 3;
  hipSetDevice(e->device);
  WritePlan p;
  if (int rc = write_prepare(e, in, n, fields, false, &p)) return rc;
  if (int rc = write_match(e, &p)) return rc;
  if (p.matched != n) {
    e->error = "unknown agent id";  // (as cs_remove_agent: a removed id, or an agent the index refused)
    return 2;
  }
  if (int rc = write_check_waypoints(e, p)) return rc;
  return write_apply(e, &p, nullptr);
}

// Collective.  Every tile matches the batch against the agents it holds; the counts and the per-record errors are
// summed over the tiles (and the ranks) before anything is applied; movers are gathered like cs_mesh_recut's exports
// and imported by every tile, each keeping what it owns.
int cs_mesh_write_agents(cs_mesh* m, const cs_agent_view* in, size_t n, uint32_t fields) {
  if (!m) return 3;
  if (m->dead()) return m->poison_rc;
  if (int rc = write_check_mask(&m->error, fields)) return rc;
  if (int rc = cs_mesh_synchronize(m)) return rc;  // queued steps first; a failure of one of them is the write's
  hipSetDevice(m->device);
  std::vector<WritePlan> plans(m->tiles.size());
  // host checks: the same batch gives the same answer on every rank (the grid and the ids are the same everywhere)
  for (size_t k = 0; k < m->tiles.size(); ++k)
    if (int rc = write_prepare(m->tiles[k], in, n, fields, true, &plans[k])) return m->fail(m->tiles[k], rc);
  // the match on every local tile; what it found is summed over the ranks before anybody applies anything
  struct Found {
    uint64_t matched;
    int32_t err;  // 0, 3 = a next_waypoint out of range, 90 = a HIP error
    int32_t pad;
  } mine{0, 0, 0};
  std::string local_error;
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    cs_engine* e = m->tiles[k];
    int rc = write_match(e, &plans[k]);
    if (!rc) rc = write_check_waypoints(e, plans[k]);
    if (rc && !mine.err) {
      mine.err = rc == 3 ? 3 : 90;
      local_error = e->error;
    }
    mine.matched += plans[k].matched;
  }
  Found all_found = mine;
  if (m->distributed) {
    std::vector<Found> all((size_t)m->n_ranks);
    if (int rc = mesh_allgather(m, &mine, sizeof mine, all.data())) return m->poison(rc, m->error);
    all_found = Found{0, 0, 0};
    for (const Found& f : all) {
      all_found.matched += f.matched;
      if (!all_found.err) all_found.err = f.err;
    }
  }
  if (all_found.err == 90) return m->poison(90, local_error.empty() ? "a tile of this mesh failed while writing agents" : local_error);
  if (all_found.err) {
    m->error = "write_agents: next_waypoint out of range for this agent";
    return 3;
  }
  if (all_found.matched != n) {
    m->error = "unknown agent id";
    return 2;
  }
  // apply: in place where the tile owns the new cell, else the record leaves the tile
  std::vector<HaloRecord> movers;
  for (size_t k = 0; k < m->tiles.size(); ++k)
    if (int rc = write_apply(m->tiles[k], &plans[k], &movers))
      return m->poison(rc, std::string("cs_mesh_write_agents failed half way: ") + cs_last_error(m->tiles[k]));
  // (decided alike on every rank: the gather below is collective)
  const bool may_move = (fields & CS_WRITE_POSITION) && m->n_tiles() > 1u && n > 0;
  if (may_move) {
    std::sort(movers.begin(), movers.end(), [](const HaloRecord& a, const HaloRecord& b) { return a.id < b.id; });
    if (m->distributed) {
      std::vector<std::vector<unsigned char>> parts;
      if (int rc = mesh_host_gatherv(m, movers.data(), movers.size() * sizeof(HaloRecord), parts))
        return m->poison(rc, m->error);
      movers.clear();
      for (const auto& part : parts) {
        const size_t at = movers.size();
        movers.resize(at + part.size() / sizeof(HaloRecord));
        if (!part.empty()) std::memcpy(movers.data() + at, part.data(), part.size());
      }
    }
    for (cs_engine* e : m->tiles) {
      e->hist_valid = false;  // (the import ranks its arrivals against a fresh count)
      if (!movers.empty())
        if (int rc = cs_tile_import(e, movers.data(), movers.size()))
          return m->poison(rc, std::string("cs_mesh_write_agents failed half way: ") + cs_last_error(e));
    }
  }
  for (cs_engine* e : m->tiles) e->halo_invalidate();  // (an exchange made ahead, CS_CFG_TILE_OVERLAP, is void)
  return 0;
}

}  // extern "C"
