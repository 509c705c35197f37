// cs_select.hip.inc — selecting, counting and removing agents between steps by region, owner and state
// (include/crowdstep_state.h).  Part of the single translation unit crowdstep_hip.hip (included there, after
// cs_set_targets.hip.inc; it shares the scratch of the by-id calls and the radix passes of cs_kernels_ids.hip.inc).
//
// The reference's host iterates its `agents` map with a condition (`sim.agents.values().filter(..)`) to get the ids its
// other calls start from.  Here the condition is a cs_selection, an AND of terms, judged on the device from the columns
// a slot holds (DESIGN.md section 2, "Selecting agents between steps"):
//   tables    (sink, hlp, lp) per planner group, 12 B each, from the HOST groups (a removed sink keeps its handle there),
//             uploaded when a group was added since the last selection; nothing a call uploads grows with the groups
//   K_select  k_select, one lane per slot: the f64 position cs_read_agents reports (the expression of
//             cs_engine::to_global), the terms in f64 without contraction, wave64 ballots summed per workgroup and one
//             atomic per workgroup for the place of its device ids in the scratch list; the count and the largest
//             selected id beside it
//   sort      one read back of (count, largest id); the radix passes of the renumbering (k_ids_hist / k_ids_scan /
//             k_ids_scatter) over `count` keys and the bits of the largest id: ascending device id is ascending external
//             id (the renumbering keeps order), so the host maps min(count, cap) ids and does nothing else per id
//   K_count   k_select_count (k_count is the sort's cell histogram), the many-selections form: a lane loads SEL_ITEMS
//             agents once and keeps them in registers, the workgroup stages the selections in LDS SEL_CHUNK at a time,
//             the tally is ballot + popcount into LDS counters and one global atomic per workgroup and non-empty
//             selection
// Nothing here changes a flag of the engine; the step kernels are not touched.

#define SEL_BLOCK 256u         // k_select_count
#define SEL_SELECT_BLOCK 1024u  // k_select: one place in the list per workgroup
#define SEL_ITEMS 4u    // agents a lane of k_select_count keeps in registers per staging of the selections
#define SEL_CHUNK 64u   // selections staged in LDS at a time (104 B each: 6.5 KiB)

// one agent as the terms see it
struct SelAgent {
  double x, y, vx, vy;
  uint32_t wp;
  SelGroupDev g;
};

// The terms, exactly as include/crowdstep_state.h writes them: f64, each product and sum rounded once (the library is
// built without contraction), a NaN fails the comparison it takes part in.  Host and device: the agents the index never
// took are judged by the host with the same function.
__host__ __device__ inline bool sel_pred(const cs_selection& s, double x, double y, double vx, double vy, uint64_t wp,
                                         uint32_t sink, uint32_t hlp, uint32_t lp) {
  const uint32_t t = s.terms;
  bool ok = true;
  if (t & CS_SEL_RECT) ok = ok && (s.x0 <= x && x < s.x1 && s.y0 <= y && y < s.y1);
  if (t & CS_SEL_CIRCLE) {
    const double dx = x - s.cx, dy = y - s.cy;
    ok = ok && (dx * dx + dy * dy < s.r * s.r);
  }
  if (t & CS_SEL_SOURCE_SINK) ok = ok && sink == s.source_sink;
  if (t & CS_SEL_HLP) ok = ok && hlp == s.hlp;
  if (t & CS_SEL_LP) ok = ok && lp == s.lp;
  if (t & CS_SEL_WAYPOINT) ok = ok && (s.wp_lo <= wp && wp <= s.wp_hi);
  if (t & CS_SEL_SPEED) {
    const double v2 = vx * vx + vy * vy;
    ok = ok && (s.speed_lo * s.speed_lo <= v2 && v2 < s.speed_hi * s.speed_hi);
  }
  return ok;
}

// Slot i as a selection sees it; false: beyond the slots in use, dead, a ghost (`owned_only`, the rule of k_write_match)
// or of no known group.  The position is the expression of cs_engine::to_global, so the f64 value cs_read_agents reports.
__device__ __forceinline__ bool sel_load(const GridDev& g, const AgentArrays& a, uint32_t i, uint32_t limit,
                                         uint32_t owned_only, const SelGroupDev* __restrict__ groups, uint32_t n_groups,
                                         double grid_off_x, double grid_off_y, double cell_size, bool want_vel,
                                         SelAgent* out) {
  const uint32_t c = i < limit ? a.cell[i] : CS_INVALID_CELL;
  if (c == CS_INVALID_CELL) return false;
  const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
  if (owned_only && (cx < g.own_x0 || cx >= g.own_x1 || cy < g.own_y0 || cy >= g.own_y1)) return false;
  const uint32_t meta = a.meta[i];
  const uint32_t grp = meta_group(g, meta);
  if (grp >= n_groups) return false;
  out->g = groups[grp];
  out->wp = meta_waypoint(g, meta);
  const float2 off = a.off[i];
  out->x = grid_off_x + ((double)((uint64_t)g.org_x + cx) * cell_size + (double)off.x);
  out->y = grid_off_y + ((double)((uint64_t)g.org_y + cy) * cell_size + (double)off.y);
  out->vx = 0.0;
  out->vy = 0.0;
  if (want_vel) {
    const float2 vel = a.vel[i];
    out->vx = (double)vel.x;
    out->vy = (double)vel.y;
  }
  return true;
}

// K_select.  hdr[0]: the number selected, hdr[1]: the largest selected device id (both start at 0).  `out` has room for
// `cap` ids (the host gives it one per slot).  The waves of a workgroup add their ballots up in LDS and the workgroup
// takes its place in the list with ONE atomic (and one for the largest id): with everybody selected, an atomic per wave
// on the same word was most of the kernel's time (0.36 ms of it at a million agents).
__global__ void __launch_bounds__(SEL_SELECT_BLOCK)
    k_select(GridDev g, AgentArrays a, uint32_t n_ub, const Counters* __restrict__ ctr, uint32_t tile, uint32_t owned_only,
             const SelGroupDev* __restrict__ groups, uint32_t n_groups, double grid_off_x, double grid_off_y,
             double cell_size, cs_selection s, uint32_t* __restrict__ out, uint32_t cap, uint32_t* __restrict__ hdr) {
  __shared__ uint32_t s_at[SEL_SELECT_BLOCK / 64u];   // per wave: its count, then where its ids go
  __shared__ uint32_t s_top[SEL_SELECT_BLOCK / 64u];  // per wave: its largest selected id
  const uint32_t limit = tile ? min(n_ub, ctr->n_pending) : n_ub;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  SelAgent ag;
  bool hit = sel_load(g, a, i, limit, owned_only, groups, n_groups, grid_off_x, grid_off_y, cell_size,
                      (s.terms & CS_SEL_SPEED) != 0u, &ag);
  hit = hit && sel_pred(s, ag.x, ag.y, ag.vx, ag.vy, ag.wp, ag.g.sink, ag.g.hlp, ag.g.lp);
  const uint32_t id = hit ? a.id[i] : 0u;
  const unsigned long long m = __ballot(hit);
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  uint32_t top = id;
  for (int d = 32; d >= 1; d >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, d, 64));
  if (lane == 0u) {
    s_at[wave] = (uint32_t)__popcll(m);
    s_top[wave] = top;
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t total = 0, largest = 0;
    for (uint32_t w = 0; w < n_waves; ++w) {
      const uint32_t c = s_at[w];
      s_at[w] = total;
      total += c;
      largest = max(largest, s_top[w]);
    }
    if (total) {
      const uint32_t base = atomicAdd(&hdr[0], total);
      for (uint32_t w = 0; w < n_waves; ++w) s_at[w] += base;
      atomicMax(&hdr[1], largest);
    }
  }
  __syncthreads();
  if (!hit) return;
  const uint32_t at = s_at[wave] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (at < cap) out[at] = id;
}

// K_count.  counts[k] (start at 0) += the agents selections[k] selects, n_sel <= CS_SELECT_MAX.  The workgroups stride
// over the slots SEL_BLOCK * SEL_ITEMS at a time; the bounds of both loops are the same for every lane of a workgroup,
// so the barriers and the ballots see whole workgroups and whole waves.
__global__ void __launch_bounds__(SEL_BLOCK)
    k_select_count(GridDev g, AgentArrays a, uint32_t n_ub, const Counters* __restrict__ ctr, uint32_t tile,
                   uint32_t owned_only, const SelGroupDev* __restrict__ groups, uint32_t n_groups, double grid_off_x,
                   double grid_off_y, double cell_size, const cs_selection* __restrict__ sels, uint32_t n_sel,
                   uint32_t want_vel, uint32_t* __restrict__ counts) {
  __shared__ cs_selection s_sel[SEL_CHUNK];
  __shared__ uint32_t s_cnt[CS_SELECT_MAX];
  static_assert(sizeof(cs_selection) % sizeof(uint64_t) == 0, "the staging copies 8-byte words");
  n_sel = min(n_sel, CS_SELECT_MAX);
  for (uint32_t j = threadIdx.x; j < n_sel; j += SEL_BLOCK) s_cnt[j] = 0u;
  const uint32_t limit = tile ? min(n_ub, ctr->n_pending) : n_ub;
  const uint32_t lane = __lane_id();
  const uint64_t stride = (uint64_t)gridDim.x * SEL_BLOCK * SEL_ITEMS;
  for (uint64_t base = (uint64_t)blockIdx.x * SEL_BLOCK * SEL_ITEMS; base < limit; base += stride) {
    SelAgent ag[SEL_ITEMS];
    bool live[SEL_ITEMS];
#pragma unroll
    for (uint32_t k = 0; k < SEL_ITEMS; ++k) {
      const uint64_t i = base + k * SEL_BLOCK + threadIdx.x;
      live[k] = sel_load(g, a, i < limit ? (uint32_t)i : limit, limit, owned_only, groups, n_groups, grid_off_x, grid_off_y,
                         cell_size, want_vel != 0u, &ag[k]);
    }
    for (uint32_t c0 = 0; c0 < n_sel; c0 += SEL_CHUNK) {
      const uint32_t nc = min(SEL_CHUNK, n_sel - c0);
      __syncthreads();  // (the chunk before is read; the first time: the counters are zero)
      {
        const uint64_t* src = reinterpret_cast<const uint64_t*>(sels + c0);
        uint64_t* dst = reinterpret_cast<uint64_t*>(s_sel);
        const uint32_t words = nc * (uint32_t)(sizeof(cs_selection) / sizeof(uint64_t));
        for (uint32_t w = threadIdx.x; w < words; w += SEL_BLOCK) dst[w] = src[w];
      }
      __syncthreads();
      for (uint32_t j = 0; j < nc; ++j) {
        const cs_selection& s = s_sel[j];  // (the same for the whole wave: LDS broadcasts)
        uint32_t n = 0;
#pragma unroll
        for (uint32_t k = 0; k < SEL_ITEMS; ++k)
          n += (uint32_t)__popcll(__ballot(
              live[k] && sel_pred(s, ag[k].x, ag[k].y, ag[k].vx, ag[k].vy, ag[k].wp, ag[k].g.sink, ag[k].g.hlp, ag[k].g.lp)));
        if (n && lane == 0u) atomicAdd(&s_cnt[c0 + j], n);
      }
    }
  }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < n_sel; j += SEL_BLOCK) {
    const uint32_t v = s_cnt[j];
    if (v) atomicAdd(&counts[j], v);
  }
}

namespace {

constexpr uint32_t kSelTermsAll =
    CS_SEL_RECT | CS_SEL_CIRCLE | CS_SEL_SOURCE_SINK | CS_SEL_HLP | CS_SEL_LP | CS_SEL_WAYPOINT | CS_SEL_SPEED;

// unknown term bits, a NaN in a field a set term reads, r < 0 (3)
int sel_check(std::string* error, const cs_selection* s, const char* what) {
  if (!s) {
    *error = std::string(what) + ": null selection";
    return 3;
  }
  if (s->terms & ~kSelTermsAll) {
    *error = std::string(what) + ": unknown selection term bits";
    return 3;
  }
  bool nan = false;
  if (s->terms & CS_SEL_RECT) nan = nan || s->x0 != s->x0 || s->y0 != s->y0 || s->x1 != s->x1 || s->y1 != s->y1;
  if (s->terms & CS_SEL_CIRCLE) nan = nan || s->cx != s->cx || s->cy != s->cy || s->r != s->r;
  if (s->terms & CS_SEL_SPEED) nan = nan || s->speed_lo != s->speed_lo || s->speed_hi != s->speed_hi;
  if (nan) {
    *error = std::string(what) + ": a NaN in a field of the selection";
    return 3;
  }
  if ((s->terms & CS_SEL_CIRCLE) && s->r < 0.0) {
    *error = std::string(what) + ": a negative radius";
    return 3;
  }
  return 0;
}

// the agents the index never took, as cs_read_agents lists them: at their created position, at rest, waypoint 0, spawned
// by no sink
bool sel_limbo(const cs_engine* e, const cs_selection& s, const cs_engine::LimboAgent& l) {
  const HostGroup& g = e->groups[l.group];
  return sel_pred(s, l.x, l.y, 0.0, 0.0, 0u, g.sink >= 0 ? (uint32_t)g.sink : UINT32_MAX, g.hlp, g.lp);
}
bool sel_limbo(const cs_selection& s, const cs_mesh::Limbo& l) {
  return sel_pred(s, l.view.x, l.view.y, l.view.vx, l.view.vy, l.view.next_waypoint, UINT32_MAX, l.hlp, l.lp);
}

// The queued steps first (a failure of one of them is the call's), then the selections' group table when a group was
// added since.  Touches no flag the step reads.
int sel_begin(cs_engine* e) {
  if (e->poisoned) {
    e->error = e->poison_error;
    return 1;
  }
  if (int rc = cs_synchronize(e)) return rc;
  if (!e->sel_groups_dirty) return 0;
  const size_t n = e->groups.size();
  std::vector<SelGroupDev> host(n);
  for (size_t i = 0; i < n; ++i) {
    const HostGroup& g = e->groups[i];  // (NOT the GroupDev copy: that one forgets a removed sink)
    host[i] = SelGroupDev{g.sink >= 0 ? (uint32_t)g.sink : UINT32_MAX, g.hlp, g.lp};
  }
  if (n > e->sel_groups_dev.count()) {
    HIP_OK_E(e, hipStreamSynchronize(e->stream));
    HIP_OK_E(e, e->sel_groups_dev.alloc(std::max<size_t>(1024, 2 * n)));
  }
  if (n) {
    HIP_OK_E(e, hipMemcpyAsync(e->sel_groups_dev.get(), host.data(), n * sizeof(SelGroupDev), hipMemcpyHostToDevice, e->stream));
    HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (the host staging dies here)
  }
  e->sel_groups_dirty = false;
  return 0;
}

size_t sel_up(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }

// K_select, the sort and one download on one engine (after sel_begin): *count = the agents of its (owned) slots that
// `s` selects, ids = the first min(*count, want) of them as DEVICE ids, ascending.  One memset, one kernel, one read back
// of two words, three launches per 4 bits of the largest selected id, one download: nothing depends on the slots or on
// the size of the answer.
int sel_run(cs_engine* e, const cs_selection& s, size_t want, std::vector<uint32_t>* ids, size_t* count) {
  ids->clear();
  *count = 0;
  const uint32_t n = e->n_slots;
  if (!n) return 0;
  const size_t tiles_max = ((size_t)n + IDS_TILE - 1u) / IDS_TILE;
  const size_t b_hdr = 256u, b_keys = sel_up((size_t)n * sizeof(uint32_t));
  const size_t b_hist = sel_up(IDS_RADIX * tiles_max * sizeof(uint32_t));
  if (int rc = write_scratch_reserve(e, b_hdr + 2u * b_keys + b_hist)) return rc;
  unsigned char* sc = static_cast<unsigned char*>(e->write_scratch.get());
  uint32_t* hdr = reinterpret_cast<uint32_t*>(sc);
  uint32_t* keys = reinterpret_cast<uint32_t*>(sc + b_hdr);
  uint32_t* other = reinterpret_cast<uint32_t*>(sc + b_hdr + b_keys);
  uint32_t* hist = reinterpret_cast<uint32_t*>(sc + b_hdr + 2u * b_keys);
  HIP_OK_E(e, hipMemsetAsync(hdr, 0, 2u * sizeof(uint32_t), e->stream));
  hipLaunchKernelGGL(k_select, dim3((n + SEL_SELECT_BLOCK - 1u) / SEL_SELECT_BLOCK), dim3(SEL_SELECT_BLOCK), 0, e->stream,
                     e->gdev, e->buf[e->cur], n, e->ctr.get(), e->tile ? 1u : 0u, (e->tile && e->ghosts_present) ? 1u : 0u,
                     e->sel_groups_dev.get(), (uint32_t)e->groups.size(), e->grid.offset_x, e->grid.offset_y, e->grid.cell_size, s,
                     keys, n, hdr);
  HIP_OK_E(e, hipGetLastError());
  uint32_t back[2] = {0u, 0u};
  HIP_OK_E(e, hipMemcpyAsync(back, hdr, sizeof back, hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  const uint32_t found = back[0];
  if (found > n) {
    e->error = "select_agents: more agents selected than slots";
    return 90;
  }
  *count = found;
  const size_t take = std::min<size_t>(found, want);
  if (!take) return 0;
  if (found > 1u) {  // (the passes are sized by the answer: its count and the bits of its largest id)
    const uint32_t tiles = (found + IDS_TILE - 1u) / IDS_TILE;
    const uint32_t bits = back[1] ? 32u - (uint32_t)__builtin_clz(back[1]) : 1u;
    for (uint32_t shift = 0; shift < bits; shift += 4u) {
      hipLaunchKernelGGL(k_ids_hist, dim3(tiles), dim3(IDS_BLOCK), 0, e->stream, keys, found, shift, hist, tiles);
      hipLaunchKernelGGL(k_ids_scan, dim3(1), dim3(IDS_BLOCK), 0, e->stream, hist, IDS_RADIX * tiles);
      hipLaunchKernelGGL(k_ids_scatter, dim3(tiles), dim3(IDS_BLOCK), 0, e->stream, keys, other, found, shift, hist, tiles);
      std::swap(keys, other);
    }
    HIP_OK_E(e, hipGetLastError());
  }
  ids->resize(take);
  HIP_OK_E(e, hipMemcpyAsync(ids->data(), keys, take * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  return 0;
}

// The selected agents of one engine as external ids, ascending, the agents the index never took merged in (`limbo`:
// not for a tile of a mesh, whose mesh keeps that list): *count = all of them, ids = the first min(*count, want).
int sel_ids(cs_engine* e, const cs_selection& s, size_t want, bool limbo, std::vector<uint64_t>* ids, size_t* count) {
  std::vector<uint32_t> dev;
  if (int rc = sel_run(e, s, want, &dev, count)) return rc;
  ids->resize(dev.size());
  for (size_t k = 0; k < dev.size(); ++k) (*ids)[k] = e->ext_id(dev[k]);
  if (limbo && !e->limbo.empty()) {
    std::vector<uint64_t> extra;
    for (const cs_engine::LimboAgent& l : e->limbo)
      if (sel_limbo(e, s, l)) extra.push_back(l.id);
    if (!extra.empty()) {
      std::sort(extra.begin(), extra.end());
      std::vector<uint64_t> all(ids->size() + extra.size());
      std::merge(ids->begin(), ids->end(), extra.begin(), extra.end(), all.begin());
      *count += extra.size();
      all.resize(std::min(all.size(), std::min(*count, want)));
      ids->swap(all);
    }
  }
  return 0;
}

// K_count on one engine (after sel_begin): counts[k] += the agents of its (owned) slots that sels[k] selects.  One
// upload, one memset, one kernel, one download.
int sel_count(cs_engine* e, const cs_selection* sels, size_t n_sel, uint64_t* counts) {
  const uint32_t n = e->n_slots;
  if (!n || !n_sel) return 0;
  const size_t b_sels = sel_up(n_sel * sizeof(cs_selection)), b_cnt = sel_up(n_sel * sizeof(uint32_t));
  if (int rc = write_scratch_reserve(e, b_sels + b_cnt)) return rc;
  unsigned char* sc = static_cast<unsigned char*>(e->write_scratch.get());
  cs_selection* d_sels = reinterpret_cast<cs_selection*>(sc);
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(sc + b_sels);
  uint32_t want_vel = 0u;
  for (size_t k = 0; k < n_sel; ++k)
    if (sels[k].terms & CS_SEL_SPEED) want_vel = 1u;
  HIP_OK_E(e, hipMemcpyAsync(d_sels, sels, n_sel * sizeof(cs_selection), hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipMemsetAsync(d_cnt, 0, n_sel * sizeof(uint32_t), e->stream));
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || n_cu <= 0) n_cu = 256;
  const uint64_t per_block = (uint64_t)SEL_BLOCK * SEL_ITEMS;
  const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1u) / per_block, (uint64_t)n_cu * 4u));
  hipLaunchKernelGGL(k_select_count, dim3(blocks), dim3(SEL_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], n, e->ctr.get(),
                     e->tile ? 1u : 0u, (e->tile && e->ghosts_present) ? 1u : 0u, e->sel_groups_dev.get(), (uint32_t)e->groups.size(),
                     e->grid.offset_x, e->grid.offset_y, e->grid.cell_size, d_sels, (uint32_t)n_sel, want_vel, d_cnt);
  HIP_OK_E(e, hipGetLastError());
  std::vector<uint32_t> back(n_sel);
  HIP_OK_E(e, hipMemcpyAsync(back.data(), d_cnt, n_sel * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  for (size_t k = 0; k < n_sel; ++k) counts[k] += back[k];
  return 0;
}

int sel_check_many(std::string* error, const cs_selection* sels, size_t n, const uint64_t* out) {
  if (n && (!sels || !out)) {
    *error = "count_agents: null array";
    return 3;
  }
  if (n > CS_SELECT_MAX) {
    *error = "count_agents: more than CS_SELECT_MAX (1024) selections in one call";
    return 3;
  }
  for (size_t k = 0; k < n; ++k)
    if (int rc = sel_check(error, &sels[k], "count_agents")) return rc;
  return 0;
}

// the selected ids of the whole mesh on every rank: every tile's sorted list merged, then (distributed) one gather of
// variable size.  *count = all of them, ids = the first min(*count, want).
int sel_mesh_ids(cs_mesh* m, const cs_selection& s, size_t want, std::vector<uint64_t>* ids, size_t* count) {
  if (int rc = cs_mesh_synchronize(m)) return rc;  // queued steps first; a failure of one of them is the call's
  hipSetDevice(m->device);
  int err = 0;
  std::string why;
  std::vector<uint64_t> all;
  std::vector<size_t> ends;
  uint64_t total = 0;
  for (cs_engine* e : m->tiles) {
    std::vector<uint64_t> part;
    size_t c = 0;
    if (!err) err = sel_begin(e);
    if (!err) err = sel_ids(e, s, want, false, &part, &c);
    if (err && why.empty()) why = cs_last_error(e);
    total += c;
    all.insert(all.end(), part.begin(), part.end());
    ends.push_back(all.size());
  }
  mesh_merge_runs(all, ends);
  if (m->distributed) {
    // what this rank's tiles selected: (failed?, count, the first ids)
    std::vector<uint64_t> mine;
    mine.push_back(err ? 1u : 0u);
    mine.push_back(total);
    if (!err) mine.insert(mine.end(), all.begin(), all.begin() + (long)std::min(all.size(), want));
    std::vector<std::vector<unsigned char>> parts;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), parts)) return m->poison(rc, m->error);
    all.clear();
    ends.clear();
    total = 0;
    for (const auto& part : parts) {
      const size_t words = part.size() / sizeof(uint64_t);
      std::vector<uint64_t> w(words);
      if (words) std::memcpy(w.data(), part.data(), words * sizeof(uint64_t));
      if (words < 2u || w[0]) {
        if (!err) {
          err = 90;
          why = "a tile of another rank failed while selecting agents";
        }
        continue;
      }
      total += w[1];
      all.insert(all.end(), w.begin() + 2, w.end());
      ends.push_back(all.size());
    }
    mesh_merge_runs(all, ends);
  }
  if (err) {
    m->error = why;
    return err;
  }
  // the mesh's own list of the agents the index never took (the same on every rank)
  std::vector<uint64_t> extra;
  for (const cs_mesh::Limbo& l : m->limbo)
    if (sel_limbo(s, l)) extra.push_back(l.view.id);
  if (!extra.empty()) {
    std::sort(extra.begin(), extra.end());
    std::vector<uint64_t> merged(all.size() + extra.size());
    std::merge(all.begin(), all.end(), extra.begin(), extra.end(), merged.begin());
    all.swap(merged);
    total += extra.size();
  }
  all.resize(std::min<size_t>(all.size(), std::min<uint64_t>(total, want)));
  ids->swap(all);
  *count = (size_t)total;
  return 0;
}

void sel_copy_out(const std::vector<uint64_t>& ids, uint64_t* out_ids, size_t cap) {
  if (!out_ids) return;
  const size_t k = std::min(ids.size(), cap);
  if (k) std::memcpy(out_ids, ids.data(), k * sizeof(uint64_t));
}

}  // namespace

extern "C" {

size_t cs_select_agents(cs_engine* e, const cs_selection* sel, uint64_t* out_ids, size_t cap) {
  if (!e) return SIZE_MAX;
  hipSetDevice(e->device);
  if (sel_check(&e->error, sel, "select_agents")) return SIZE_MAX;
  if (sel_begin(e)) return SIZE_MAX;
  std::vector<uint64_t> ids;
  size_t count = 0;
  if (sel_ids(e, *sel, out_ids ? cap : 0u, true, &ids, &count)) return SIZE_MAX;
  sel_copy_out(ids, out_ids, cap);
  return count;
}

int cs_count_agents(cs_engine* e, const cs_selection* selections, size_t n, uint64_t* out_counts) {
  if (!e) return 3;
  hipSetDevice(e->device);
  if (int rc = sel_check_many(&e->error, selections, n, out_counts)) return rc;
  if (int rc = sel_begin(e)) return rc;
  std::vector<uint64_t> counts(n, 0);
  if (int rc = sel_count(e, selections, n, counts.data())) return rc;
  for (const cs_engine::LimboAgent& l : e->limbo)
    for (size_t k = 0; k < n; ++k)
      if (sel_limbo(e, selections[k], l)) counts[k] += 1u;
  for (size_t k = 0; k < n; ++k) out_counts[k] = counts[k];
  return 0;
}

size_t cs_remove_selected(cs_engine* e, const cs_selection* sel, uint64_t* out_ids, size_t cap) {
  if (!e) return SIZE_MAX;
  hipSetDevice(e->device);
  if (sel_check(&e->error, sel, "remove_selected")) return SIZE_MAX;
  if (sel_begin(e)) return SIZE_MAX;
  std::vector<uint64_t> ids;
  size_t count = 0;
  if (sel_ids(e, *sel, SIZE_MAX, true, &ids, &count)) return SIZE_MAX;
  if (cs_remove_agents(e, ids.data(), ids.size())) return SIZE_MAX;
  sel_copy_out(ids, out_ids, cap);
  return ids.size();
}

size_t cs_mesh_select_agents(cs_mesh* m, const cs_selection* sel, uint64_t* out_ids, size_t cap) {
  if (!m) return SIZE_MAX;
  if (m->dead()) return SIZE_MAX;
  if (sel_check(&m->error, sel, "select_agents")) return SIZE_MAX;
  std::vector<uint64_t> ids;
  size_t count = 0;
  if (sel_mesh_ids(m, *sel, out_ids ? cap : 0u, &ids, &count)) return SIZE_MAX;
  sel_copy_out(ids, out_ids, cap);
  return count;
}

// Collective.  Every tile counts among the agents it owns; the sums of the ranks travel in one gather of n + 1 words.
int cs_mesh_count_agents(cs_mesh* m, const cs_selection* selections, size_t n, uint64_t* out_counts) {
  if (!m) return 3;
  if (m->dead()) return m->poison_rc;
  if (int rc = sel_check_many(&m->error, selections, n, out_counts)) return rc;
  if (int rc = cs_mesh_synchronize(m)) return rc;
  hipSetDevice(m->device);
  std::vector<uint64_t> mine(n + 1u, 0);  // [failed?, counts]
  std::string why;
  for (cs_engine* e : m->tiles) {
    int rc = mine[0] ? 0 : sel_begin(e);
    if (!rc && !mine[0]) rc = sel_count(e, selections, n, mine.data() + 1);
    if (rc) {
      mine[0] = 1u;
      why = cs_last_error(e);
    }
  }
  std::vector<uint64_t> sum(mine);
  if (m->distributed) {
    std::vector<uint64_t> all((n + 1u) * (size_t)m->n_ranks);
    if (int rc = mesh_allgather(m, mine.data(), mine.size() * sizeof(uint64_t), all.data())) return m->poison(rc, m->error);
    std::fill(sum.begin(), sum.end(), 0u);
    for (size_t r = 0; r < (size_t)m->n_ranks; ++r)
      for (size_t k = 0; k <= n; ++k) sum[k] += all[r * (n + 1u) + k];
  }
  if (sum[0]) {
    m->error = why.empty() ? "a tile of another rank failed while counting agents" : why;
    return 90;
  }
  for (const cs_mesh::Limbo& l : m->limbo)
    for (size_t k = 0; k < n; ++k)
      if (sel_limbo(selections[k], l)) sum[k + 1u] += 1u;
  for (size_t k = 0; k < n; ++k) out_counts[k] = sum[k + 1u];
  return 0;
}

// Collective: the selection on every rank, then cs_mesh_remove_agents of what it gave (agreement before any slot dies,
// events on the owning tile).
size_t cs_mesh_remove_selected(cs_mesh* m, const cs_selection* sel, uint64_t* out_ids, size_t cap) {
  if (!m) return SIZE_MAX;
  if (m->dead()) return SIZE_MAX;
  if (sel_check(&m->error, sel, "remove_selected")) return SIZE_MAX;
  std::vector<uint64_t> ids;
  size_t count = 0;
  if (sel_mesh_ids(m, *sel, SIZE_MAX, &ids, &count)) return SIZE_MAX;
  if (cs_mesh_remove_agents(m, ids.data(), ids.size())) return SIZE_MAX;
  sel_copy_out(ids, out_ids, cap);
  return ids.size();
}

}  // extern "C"
