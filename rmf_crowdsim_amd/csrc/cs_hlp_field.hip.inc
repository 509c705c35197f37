// cs_hlp_field.hip.inc — the flow-field high-level planner: a raster of preferred velocities that lives on the device and is
// sampled there every step (include/crowdstep_state.h, cs_register_hlp_field).  Part of the single translation unit
// crowdstep_hip.hip (included there, after cs_field.hip.inc, whose raster layout and binning expression it shares).
//
// The step kernels already read the answers of host planners from pref[slot] (hlp_velocity, case CS_HLP_CALLBACK).  A
// field planner's groups are such groups on the device, and one small kernel fills their slots of pref where the host
// path (cs_engine::eval_callback_hlps) downloads the state, calls the host, uploads and waits (DESIGN.md section 2,
// "Flow-field planner"):
//   K_hlp_field   k_hlp_field, one thread per slot of the sorted state: cell (dead slots skipped) -> meta -> group -> the
//                 group's planner -> the table of fields (one HlpFieldDev per planner handle; vxy == null: no field, the
//                 slot is NOT written) -> the f64 position cs_read_agents reports, the expression of cs_engine::to_global
//                 -> hlp_field_sample -> pref[slot].  A streaming pass: 16 B read and 8 B written per agent, and a gather
//                 of one to four 8-byte samples that is coherent because the slots are in cell order.
// The rule is compiled like the binning of cs_field.hip.inc: the library is built without contraction and without
// fast-math, so every line below is the IEEE operation it spells, on the host (cs_engine never calls it; the mirrors restate
// it) and on the device alike.  The step kernels are not touched.

#define HLP_FIELD_BLOCK 256u

__host__ __device__ inline bool hlp_field_is_nan(float v) { return v != v; }

// NEAREST of bin (ix, iy): the sample itself, or None = (0, 0) where a component is NaN
__host__ __device__ inline float2 hlp_field_nearest(const cs_field_desc& d, const float2* __restrict__ vxy, uint32_t ix,
                                                    uint32_t iy) {
  const float2 s = vxy[(size_t)iy * d.nx + ix];
  if (hlp_field_is_nan(s.x) || hlp_field_is_nan(s.y)) return make_float2(0.0f, 0.0f);
  return s;
}

// one axis of BILINEAR: the two bins whose centres lie on either side of f, and the weight of the upper one
__host__ __device__ inline void hlp_field_axis(double f, uint32_t n, uint32_t* i0, uint32_t* i1, double* t) {
  const double a = f - 0.5;
  if (a < 0.0) {
    *i0 = *i1 = 0u;
    *t = 0.0;
    return;
  }
  *i0 = (uint32_t)a;
  *t = a - (double)*i0;
  *i1 = *i0 + 1u < n ? *i0 + 1u : n - 1u;
}

// The rule of include/crowdstep_state.h for one agent at (x, y).
__host__ __device__ inline float2 hlp_field_sample(const cs_field_desc& d, uint32_t sampling, const float2* __restrict__ vxy,
                                                   double x, double y) {
  const double fx = (x - d.x0) / d.cell_w, fy = (y - d.y0) / d.cell_h;
  if (!(0.0 <= fx && fx < (double)d.nx && 0.0 <= fy && fy < (double)d.ny)) return make_float2(0.0f, 0.0f);
  const uint32_t ix = (uint32_t)fx, iy = (uint32_t)fy;
  if (sampling != CS_HLP_FIELD_BILINEAR) return hlp_field_nearest(d, vxy, ix, iy);
  uint32_t i0, i1, j0, j1;
  double tx, ty;
  hlp_field_axis(fx, d.nx, &i0, &i1, &tx);
  hlp_field_axis(fy, d.ny, &j0, &j1, &ty);
  const float2 s00 = vxy[(size_t)j0 * d.nx + i0], s10 = vxy[(size_t)j0 * d.nx + i1];
  const float2 s01 = vxy[(size_t)j1 * d.nx + i0], s11 = vxy[(size_t)j1 * d.nx + i1];
  if (hlp_field_is_nan(s00.x) || hlp_field_is_nan(s00.y) || hlp_field_is_nan(s10.x) || hlp_field_is_nan(s10.y) ||
      hlp_field_is_nan(s01.x) || hlp_field_is_nan(s01.y) || hlp_field_is_nan(s11.x) || hlp_field_is_nan(s11.y))
    return hlp_field_nearest(d, vxy, ix, iy);
  const double ax = (double)s00.x + ((double)s10.x - (double)s00.x) * tx;
  const double bx = (double)s01.x + ((double)s11.x - (double)s01.x) * tx;
  const double ay = (double)s00.y + ((double)s10.y - (double)s00.y) * tx;
  const double by = (double)s01.y + ((double)s11.y - (double)s01.y) * tx;
  return make_float2((float)(ax + (bx - ax) * ty), (float)(ay + (by - ay) * ty));
}

// K_hlp_field.  n: the host's slot count of the sorted arrays (a tile's is an upper bound: the scan's n_alive ends the
// live slots, as for the step kernels).  Every index is checked before it is used.
__global__ void __launch_bounds__(HLP_FIELD_BLOCK)
    k_hlp_field(GridDev g, const uint32_t* __restrict__ cell, const float2* __restrict__ off, const uint32_t* __restrict__ meta,
                uint32_t n, const Counters* __restrict__ ctr, const GroupDev* __restrict__ groups, uint32_t n_groups,
                const HlpFieldDev* __restrict__ fields, uint32_t n_fields, double grid_off_x, double grid_off_y,
                double cell_size, float2* __restrict__ pref) {
  const uint32_t i = blockIdx.x * HLP_FIELD_BLOCK + threadIdx.x;
  if (i >= n || i >= ctr->n_alive) return;
  const uint32_t c = cell[i];
  if (c == CS_INVALID_CELL) return;
  const uint32_t grp = meta_group(g, meta[i]);
  if (grp >= n_groups) return;
  const uint32_t hlp = groups[grp].hlp;
  if (hlp >= n_fields) return;
  const HlpFieldDev f = fields[hlp];
  if (!f.vxy) return;
  const uint32_t gx = c / g.nx, gy = c - gx * g.nx;
  const float2 o = off[i];
  // (the expression of cs_engine::to_global: the f64 position a host planner is handed)
  const double x = grid_off_x + ((double)(g.org_x + gx) * cell_size + (double)o.x);
  const double y = grid_off_y + ((double)(g.org_y + gy) * cell_size + (double)o.y);
  pref[i] = hlp_field_sample(f.d, f.sampling, f.vxy, x, y);
}

namespace {

// every refusal of a raster cs_agent_field makes (field_check), a null pointer and an unknown sampling
bool hlp_field_check(std::string* error, const cs_field_desc* d, uint32_t sampling, const float* vxy) {
  auto refuse = [&](const char* why) {
    *error = std::string("hlp_field: ") + why;
    return false;
  };
  if (!d) return refuse("null raster description");
  if (!vxy) return refuse("null samples");
  if (!std::isfinite(d->x0) || !std::isfinite(d->y0) || !std::isfinite(d->cell_w) || !std::isfinite(d->cell_h))
    return refuse("a non-finite origin or bin size");
  if (!(d->cell_w > 0.0) || !(d->cell_h > 0.0)) return refuse("a bin size that is not above zero");
  if (!d->nx || !d->ny) return refuse("a raster without bins");
  if ((uint64_t)d->nx * (uint64_t)d->ny > (uint64_t)CS_FIELD_MAX_CELLS) return refuse("more than CS_FIELD_MAX_CELLS (4194304) bins");
  if (sampling != CS_HLP_FIELD_NEAREST && sampling != CS_HLP_FIELD_BILINEAR) return refuse("unknown sampling");
  return true;
}

}  // namespace

// The field planners' turn in cs_engine::step: after the re-sort (and after the upload of the host planners' answers,
// which writes the whole of pref), before the step kernels and before a host LocalPlanner reads `recommended`.  On the
// engine's stream; nothing is waited for unless a field was registered since the last step (the table is uploaded then).
static int hlp_field_eval(cs_engine* e) {
  if (e->hlp_fields_dirty) {
    std::vector<HlpFieldDev> tab(e->hlps.size());
    std::memset(tab.data(), 0, tab.size() * sizeof(HlpFieldDev));
    for (const auto& kv : e->hlp_fields) {
      if (kv.first >= tab.size()) continue;
      tab[kv.first].d = kv.second.d;
      tab[kv.first].vxy = kv.second.data.get();
      tab[kv.first].sampling = kv.second.sampling;
    }
    HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (queued steps read the table that is replaced)
    if (tab.size() > e->hlp_field_tab.count()) HIP_OK_E(e, e->hlp_field_tab.alloc(2 * tab.size() + 8));
    HIP_OK_E(e, hipMemcpy(e->hlp_field_tab.get(), tab.data(), tab.size() * sizeof(HlpFieldDev), hipMemcpyHostToDevice));
    e->hlp_field_tab_n = (uint32_t)tab.size();  // (a planner registered later is no field, or sets the flag again)
    e->hlp_fields_dirty = false;
  }
  const uint32_t n = e->n_slots;
  // a CS_HLP_CALLBACK planner without a velocity function answers None: its slots of pref read zero as long as nobody
  // writes pref at all, which this kernel now does (slots change hands with every re-sort)
  if (e->any_silent_callback && !e->any_velocity_callback && n)
    HIP_OK_E(e, hipMemsetAsync(e->pref.get(), 0, (size_t)n * sizeof(float2), e->stream));
  const AgentArrays& a = e->buf[e->cur];
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (e->hlp_field_timing && e->hlp_field_timed.size() < 4096u && hipEventCreate(&t0) == hipSuccess) {
    if (hipEventCreate(&t1) == hipSuccess) {
      HIP_OK_E(e, hipEventRecord(t0, e->stream));
    } else {
      hipEventDestroy(t0);
      t0 = nullptr;
    }
  }
  hipLaunchKernelGGL(k_hlp_field, dim3(std::max(1u, (n + HLP_FIELD_BLOCK - 1u) / HLP_FIELD_BLOCK)), dim3(HLP_FIELD_BLOCK), 0,
                     e->stream, e->gdev, a.cell, a.off, a.meta, n, e->ctr.get(), e->groups_dev.get(), (uint32_t)e->groups.size(),
                     e->hlp_field_tab.get(), e->hlp_field_tab_n, e->grid.offset_x, e->grid.offset_y, e->grid.cell_size, e->pref.get());
  if (t0) {
    e->hlp_field_timed.emplace_back(t0, t1);
    HIP_OK_E(e, hipEventRecord(t1, e->stream));
  }
  HIP_OK_E(e, hipGetLastError());
  e->n_hlp_field_launches += 1;
  return 0;
}

extern "C" {

uint32_t cs_register_hlp_field(cs_engine* e, const cs_field_desc* raster, uint32_t sampling, const float* vxy) {
  if (!e) return UINT32_MAX;
  if (!hlp_field_check(&e->error, raster, sampling, vxy)) return UINT32_MAX;
  hipSetDevice(e->device);
  HostHlpField f;
  f.d = *raster;
  f.sampling = sampling;
  const size_t bytes = (size_t)raster->nx * raster->ny * sizeof(float2);
  if (f.data.alloc(bytes / sizeof(float2)) != hipSuccess) {
    (void)hipGetLastError();
    e->error = "hlp_field: out of device memory for the samples";
    return UINT32_MAX;
  }
  // (a buffer nothing queued reads yet: the blocking copy waits for no step)
  if (hipMemcpy(f.data.get(), vxy, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    e->error = "hlp_field: HIP error while uploading the samples";
    return UINT32_MAX;
  }
  cs_hlp_desc d;
  std::memset(&d, 0, sizeof d);
  d.kind = CS_HLP_FIELD;
  e->hlps.push_back(d);
  const uint32_t handle = (uint32_t)e->hlps.size() - 1;
  e->hlp_fields[handle] = std::move(f);
  e->hlp_fields_dirty = true;
  return handle;
}

int cs_hlp_field_update(cs_engine* e, uint32_t hlp, const float* vxy) {
  if (!e) return 3;
  if (!vxy) {
    e->error = "hlp_field: null samples";
    return 3;
  }
  auto it = e->hlp_fields.find(hlp);
  if (it == e->hlp_fields.end()) {
    e->error = "hlp_field: the handle is not a field planner's";
    return 3;
  }
  hipSetDevice(e->device);
  HostHlpField& f = it->second;
  const size_t bytes = (size_t)f.d.nx * f.d.ny * sizeof(float2);
  if (!f.stage.get()) {
    HIP_OK_E(e, f.stage.alloc(bytes / sizeof(float2)));
    HIP_OK_E(e, hipEventCreateWithFlags(&f.staged, hipEventDisableTiming));
  }
  if (f.stage_busy) HIP_OK_E(e, hipEventSynchronize(f.staged));  // (the upload of the update before this one)
  f.stage_busy = false;
  std::memcpy(f.stage.get(), vxy, bytes);
  // behind the steps already queued on the engine's stream, which sample the old values; in front of the next one
  HIP_OK_E(e, hipMemcpyAsync(f.data.get(), f.stage.get(), bytes, hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipEventRecord(f.staged, e->stream));
  f.stage_busy = true;
  return 0;
}

// Every tile holds the whole field (it is indexed in world coordinates) under the same handle.  A refusal is decided
// before the first tile is touched, so it leaves nothing registered anywhere.
uint32_t cs_mesh_register_hlp_field(cs_mesh* m, const cs_field_desc* raster, uint32_t sampling, const float* vxy) {
  if (!m) return UINT32_MAX;
  if (!hlp_field_check(&m->error, raster, sampling, vxy)) return UINT32_MAX;
  uint32_t handle = UINT32_MAX;
  for (cs_engine* e : m->tiles) {
    const uint32_t h = cs_register_hlp_field(e, raster, sampling, vxy);
    if (h == UINT32_MAX || (handle != UINT32_MAX && h != handle)) {
      m->error = h == UINT32_MAX ? cs_last_error(e) : "the tiles of a mesh disagree on a planner handle";
      return UINT32_MAX;
    }
    handle = h;
  }
  return handle;
}

int cs_mesh_hlp_field_update(cs_mesh* m, uint32_t hlp, const float* vxy) {
  if (!m) return 3;
  if (!vxy) {
    m->error = "hlp_field: null samples";
    return 3;
  }
  for (cs_engine* e : m->tiles)
    if (e->hlp_fields.find(hlp) == e->hlp_fields.end()) {
      m->error = "hlp_field: the handle is not a field planner's";
      return 3;
    }
  for (cs_engine* e : m->tiles)
    if (int rc = cs_hlp_field_update(e, hlp, vxy)) return m->fail(e, rc);
  return 0;
}

}  // extern "C"
