// cs_flow_solve.hip.inc — solving a flow field on the device: from goal bins, walls, a slowness raster and the crowd's
// density to the raster of preferred velocities a field planner samples (include/crowdstep_state.h, cs_flow_field_solve).
// Part of the single translation unit crowdstep_hip.hip (included there, after cs_hlp_field.hip.inc: it writes into the
// samples of a HostHlpField and reuses field_check, field_run and the selections of cs_field.hip.inc).
//
// The distances of the rule are the least fixed point of d[j] = min(d[j], d[i] + cost(j)) over the allowed steps j -> i.
// IEEE addition is monotone (a <= b implies a + c <= b + c), so every order of relaxations that runs to the fixed point
// ends at the same f64 bits as a sequential Dijkstra (DESIGN.md section 2, "Solving a flow field").  The order here:
//   K_flow_extra  k_flow_extra, one thread per agent the index never took: +1 on its bin of the counts field_run left
//   K_flow_init   k_flow_init, one thread per bin: s(bin), dist = 0 / +inf, the byte of allowed steps (bit k: step k of the
//                 header's order; the corner rule is evaluated here, once), and the tiles' flags (all active)
//   K_flow_relax  k_flow_relax, one workgroup per tile of FLOW_T x FLOW_T bins, an inactive tile leaves at once: the tile
//                 and a one-bin halo in LDS (34 x 34 f64, 9,248 B), Jacobi sweeps between barriers until no bin of the tile
//                 changes, the changed bins written back, the neighbouring tiles whose halo holds a changed bin flagged
//                 for the next round (two flag arrays, swapped per round), one add to the round's counter.  A halo value
//                 another workgroup replaces in the same round is read old or new: both are upper bounds of the fixed
//                 point, and the writer flags the reader, so the next round reads the new one.
//   host          rounds in batches of FLOW_BATCH launches, one counter per round, read after each batch; the first
//                 round that changed nothing ends the solve.  Every round holds at least one Jacobi sweep of every tile
//                 a sweep could change, and Bellman-Ford converges within one sweep per bin: at most nx * ny + 1 rounds.
//   K_flow_dir    k_flow_dir, one thread per bin: the argmin over the allowed steps in the fixed order, the table of the
//                 eight vectors, into the planner's samples or a scratch; `reached` by a wave reduction and one atomic.
// No grid-wide barrier, no workgroup waits for another.  No fast-math, no contraction (the library's flags): every line
// below is the IEEE operation it spells.  The step kernels are not touched.

#define FLOW_T 32u                       // a tile's side in bins
#define FLOW_LW (FLOW_T + 2u)            // ... and with its halo
#define FLOW_BLOCK 256u                  // threads of a relax workgroup: FLOW_PER bins each
#define FLOW_PER (FLOW_T * FLOW_T / FLOW_BLOCK)
#define FLOW_BATCH 4u                    // rounds between two reads of the counters
#define FLOW_DIR_BLOCK 256u

// step k of the header's order: dy = -1, 0, 1 outer, dx = -1, 0, 1 inner, (0, 0) skipped
__host__ __device__ inline int flow_dx(uint32_t k) { return (int)((k < 4u ? k : k + 1u) % 3u) - 1; }
__host__ __device__ inline int flow_dy(uint32_t k) { return (int)((k < 4u ? k : k + 1u) / 3u) - 1; }

// what the kernels are told of a solve
struct FlowLens {
  double w, h, d;  // len(+-1, 0), len(0, +-1), len of a diagonal
};
__host__ __device__ inline double flow_len(const FlowLens& l, uint32_t k) {
  const int dx = flow_dx(k), dy = flow_dy(k);
  return dx && dy ? l.d : dx ? l.w : l.h;
}
struct FlowVecs {
  float2 v[8];
};

__device__ inline double flow_inf() { return __longlong_as_double(0x7FF0000000000000ll); }

// K_flow_extra.  bins_of: the bin of each agent the index never took (already filtered and binned by the host).
__global__ void __launch_bounds__(FLOW_DIR_BLOCK)
    k_flow_extra(const uint32_t* __restrict__ bins_of, uint32_t n, uint32_t bins, uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * FLOW_DIR_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = bins_of[i];
  if (b < bins) atomicAdd(&cnt[b], 1u);
}

// K_flow_init.  blocked, slowness, cnt may be null (no walls, 1, no density: s = (double)slowness exactly).
__global__ void __launch_bounds__(FLOW_DIR_BLOCK)
    k_flow_init(uint32_t nx, uint32_t ny, const uint8_t* __restrict__ goals, const uint8_t* __restrict__ blocked,
                const float* __restrict__ slowness, const uint32_t* __restrict__ cnt, double density_weight,
                double* __restrict__ s, double* __restrict__ dist, uint8_t* __restrict__ mask, uint32_t n_tiles,
                uint32_t* __restrict__ act0, uint32_t* __restrict__ act1) {
  const uint32_t bin = blockIdx.x * FLOW_DIR_BLOCK + threadIdx.x;
  const uint32_t bins = nx * ny;
  if (bin < n_tiles) {
    act0[bin] = 1u;
    act1[bin] = 0u;
  }
  if (bin >= bins) return;
  const uint32_t iy = bin / nx, ix = bin - iy * nx;
  double sv = slowness ? (double)slowness[bin] : 1.0;
  if (cnt) sv = sv * (1.0 + density_weight * (double)cnt[bin]);
  s[bin] = sv;
  const bool wall = blocked && blocked[bin];
  dist[bin] = (!wall && goals[bin]) ? 0.0 : flow_inf();
  uint32_t m = 0u;
  if (!wall) {
    for (uint32_t k = 0; k < 8u; ++k) {
      const int dx = flow_dx(k), dy = flow_dy(k);
      const int64_t jx = (int64_t)ix + dx, jy = (int64_t)iy + dy;
      if (jx < 0 || jy < 0 || jx >= (int64_t)nx || jy >= (int64_t)ny) continue;
      bool ok = true;
      if (blocked) {
        ok = !blocked[(size_t)jy * nx + (size_t)jx];
        if (ok && dx && dy) ok = !blocked[(size_t)iy * nx + (size_t)jx] && !blocked[(size_t)jy * nx + ix];
      }
      if (ok) m |= 1u << k;
    }
  }
  mask[bin] = (uint8_t)m;
}

// K_flow_relax.  act_cur: the tiles of this round (a tile clears its own flag); act_next: those of the next round.
__global__ void __launch_bounds__(FLOW_BLOCK)
    k_flow_relax(uint32_t nx, uint32_t ny, uint32_t tiles_x, uint32_t tiles_y, const double* __restrict__ s,
                 const uint8_t* __restrict__ mask, double* dist, uint32_t* act_cur, uint32_t* act_next, uint32_t* changed,
                 FlowLens len) {
  __shared__ double L[FLOW_LW * FLOW_LW];
  __shared__ uint32_t l_act;
  const uint32_t tile = blockIdx.x;
  if (tile >= tiles_x * tiles_y) return;
  if (threadIdx.x == 0u) {
    l_act = act_cur[tile];
    act_cur[tile] = 0u;
  }
  __syncthreads();
  if (!l_act) return;  // (the same for the whole workgroup)
  const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int64_t bx = (int64_t)tx * FLOW_T - 1, by = (int64_t)ty * FLOW_T - 1;  // the halo's low corner
  for (uint32_t j = threadIdx.x; j < FLOW_LW * FLOW_LW; j += FLOW_BLOCK) {
    const uint32_t ly = j / FLOW_LW, lx = j - ly * FLOW_LW;
    const int64_t gx = bx + lx, gy = by + ly;
    double v = flow_inf();
    if (gx >= 0 && gy >= 0 && gx < (int64_t)nx && gy < (int64_t)ny)
      v = __hip_atomic_load(&dist[(size_t)gy * nx + (size_t)gx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    L[j] = v;
  }
  // this thread's bins: column threadIdx.x % FLOW_T, rows threadIdx.x / FLOW_T + k * (FLOW_BLOCK / FLOW_T)
  const uint32_t lx = threadIdx.x % FLOW_T, ly0 = threadIdx.x / FLOW_T;
  const uint32_t gx = tx * FLOW_T + lx;
  uint32_t m[FLOW_PER];
  double cw[FLOW_PER], ch[FLOW_PER], cd[FLOW_PER], first[FLOW_PER];
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < FLOW_PER; ++k) {
    const uint32_t ly = ly0 + k * (FLOW_BLOCK / FLOW_T), gy = ty * FLOW_T + ly;
    const bool in = gx < nx && gy < ny;
    const size_t bin = (size_t)gy * nx + gx;
    m[k] = in ? (uint32_t)mask[bin] : 0u;
    const double sv = in ? s[bin] : 0.0;
    cw[k] = len.w * sv;
    ch[k] = len.h * sv;
    cd[k] = len.d * sv;
    first[k] = L[(ly + 1u) * FLOW_LW + lx + 1u];
  }
  int again;
  do {
    double nv[FLOW_PER];
#pragma unroll
    for (uint32_t k = 0; k < FLOW_PER; ++k) {
      const uint32_t at = (ly0 + k * (FLOW_BLOCK / FLOW_T) + 1u) * FLOW_LW + lx + 1u;
      double best = L[at];
      const uint32_t mk = m[k];
      if (mk) {
        double c;
        if (mk & 1u)   { c = L[at - FLOW_LW - 1u] + cd[k]; if (c < best) best = c; }
        if (mk & 2u)   { c = L[at - FLOW_LW] + ch[k];      if (c < best) best = c; }
        if (mk & 4u)   { c = L[at - FLOW_LW + 1u] + cd[k]; if (c < best) best = c; }
        if (mk & 8u)   { c = L[at - 1u] + cw[k];           if (c < best) best = c; }
        if (mk & 16u)  { c = L[at + 1u] + cw[k];           if (c < best) best = c; }
        if (mk & 32u)  { c = L[at + FLOW_LW - 1u] + cd[k]; if (c < best) best = c; }
        if (mk & 64u)  { c = L[at + FLOW_LW] + ch[k];      if (c < best) best = c; }
        if (mk & 128u) { c = L[at + FLOW_LW + 1u] + cd[k]; if (c < best) best = c; }
      }
      nv[k] = best;
    }
    __syncthreads();  // (every read of this sweep is done)
    int ch_any = 0;
#pragma unroll
    for (uint32_t k = 0; k < FLOW_PER; ++k) {
      const uint32_t at = (ly0 + k * (FLOW_BLOCK / FLOW_T) + 1u) * FLOW_LW + lx + 1u;
      if (nv[k] < L[at]) {
        L[at] = nv[k];
        ch_any = 1;
      }
    }
    again = __syncthreads_or(ch_any);
  } while (again);
  int wrote = 0;
#pragma unroll
  for (uint32_t k = 0; k < FLOW_PER; ++k) {
    const uint32_t ly = ly0 + k * (FLOW_BLOCK / FLOW_T), gy = ty * FLOW_T + ly;
    const double v = L[(ly + 1u) * FLOW_LW + lx + 1u];
    if (!(gx < nx && gy < ny) || !(v < first[k])) continue;
    __hip_atomic_store(&dist[(size_t)gy * nx + gx], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    wrote = 1;
    // the tiles whose halo holds this bin
    const int ex = lx == 0u ? -1 : lx == FLOW_T - 1u ? 1 : 0, ey = ly == 0u ? -1 : ly == FLOW_T - 1u ? 1 : 0;
    const bool okx = ex && (int64_t)tx + ex >= 0 && (int64_t)tx + ex < (int64_t)tiles_x;
    const bool oky = ey && (int64_t)ty + ey >= 0 && (int64_t)ty + ey < (int64_t)tiles_y;
    if (okx) act_next[ty * tiles_x + (uint32_t)((int)tx + ex)] = 1u;
    if (oky) act_next[(uint32_t)((int)ty + ey) * tiles_x + tx] = 1u;
    if (okx && oky) act_next[(uint32_t)((int)ty + ey) * tiles_x + (uint32_t)((int)tx + ex)] = 1u;
  }
  if (__syncthreads_or(wrote) && threadIdx.x == 0u) atomicAdd(changed, 1u);
}

// K_flow_dir.  vxy (may be null): the vectors; reached: the number of bins with a finite distance.
__global__ void __launch_bounds__(FLOW_DIR_BLOCK)
    k_flow_dir(uint32_t nx, uint32_t ny, const uint8_t* __restrict__ goals, const double* __restrict__ s,
               const uint8_t* __restrict__ mask, const double* __restrict__ dist, FlowLens len, FlowVecs vecs,
               float2* __restrict__ vxy, unsigned long long* __restrict__ reached) {
  const uint32_t bin = blockIdx.x * FLOW_DIR_BLOCK + threadIdx.x;
  const uint32_t bins = nx * ny;
  bool finite = false;
  if (bin < bins) {
    const uint32_t iy = bin / nx, ix = bin - iy * nx;
    const double d = dist[bin];
    finite = d < flow_inf();
    if (vxy) {
      const float nan = __int_as_float(0x7FC00000);
      float2 out = make_float2(nan, nan);
      const uint32_t m = mask[bin];  // (0 at a blocked bin, whose distance is +inf)
      if (finite && goals[bin]) {
        out = make_float2(0.0f, 0.0f);
      } else if (finite) {
        const double sv = s[bin];
        double best = flow_inf();
        uint32_t pick = 8u;
        for (uint32_t k = 0; k < 8u; ++k) {
          if (!(m >> k & 1u)) continue;
          const int64_t jx = (int64_t)ix + flow_dx(k), jy = (int64_t)iy + flow_dy(k);
          if (jx < 0 || jy < 0 || jx >= (int64_t)nx || jy >= (int64_t)ny) continue;
          const double c = dist[(size_t)jy * nx + (size_t)jx] + flow_len(len, k) * sv;
          if (c < best) {
            best = c;
            pick = k;
          }
        }
        if (pick < 8u) out = vecs.v[pick];
      }
      vxy[bin] = out;
    }
  }
  const unsigned long long got = __ballot(finite);
  if (__lane_id() == 0u && got) atomicAdd(reached, (unsigned long long)__popcll(got));
}

namespace {

// every refusal of the list in include/crowdstep_state.h that needs no engine (3), decided before anything is touched
int flow_check(std::string* error, const cs_flow_desc* f, const float* out_vxy, const double* out_dist, uint32_t hlp) {
  auto refuse = [&](const char* why) {
    *error = std::string("flow_field_solve: ") + why;
    return 3;
  };
  if (!f) return refuse("null description");
  if (!f->goals) return refuse("null goals");
  uint32_t dummy = 0;
  if (int rc = field_check(error, &f->raster, f->density_filter, &dummy, nullptr, nullptr)) {
    *error = "flow_field_solve: " + *error;
    return rc;
  }
  if (!std::isfinite(f->speed) || f->speed < 0.0) return refuse("a speed that is not finite and >= 0");
  if (!std::isfinite(f->density_weight) || f->density_weight < 0.0 || f->density_weight > 4294967296.0)
    return refuse("a density_weight outside [0, 2^32]");
  if (hlp == UINT32_MAX && !out_vxy && !out_dist) return refuse("nothing to write to: no planner and no output");
  if (f->slowness) {
    const size_t bins = (size_t)f->raster.nx * f->raster.ny;
    for (size_t i = 0; i < bins; ++i)
      if (!(f->slowness[i] >= 0.0f) || !std::isfinite(f->slowness[i])) return refuse("a slowness that is NaN, infinite or negative");
  }
  return 0;
}

// the planner a solve writes into: a field planner of this engine whose raster equals the solve's byte for byte
int flow_planner(cs_engine* e, const cs_field_desc& d, uint32_t hlp, HostHlpField** out) {
  *out = nullptr;
  if (hlp == UINT32_MAX) return 0;
  auto it = e->hlp_fields.find(hlp);
  if (it == e->hlp_fields.end()) {
    e->error = "flow_field_solve: the handle is not a field planner's";
    return 3;
  }
  if (std::memcmp(&it->second.d, &d, sizeof d) != 0) {
    e->error = "flow_field_solve: the planner's raster is not the solve's";
    return 3;
  }
  *out = &it->second;
  return 0;
}

int flow_scratch_reserve(cs_engine* e, size_t need) {
  const int rc = scratch_reserve(e, e->flow_scratch, need, "flow_field_solve: out of device memory for the solve");
  if (rc && !e->flow_scratch.get()) (void)hipGetLastError();  // (the failed allocation's)
  return rc;
}

// The solve on one engine, after the checks.  counts_dev: the counts on this engine's device (field_run's), or
// counts_host: counts to upload (a mesh's, gathered), or neither (no density).  extra: bins of the agents the index never
// took, added to counts_dev.  Everything is queued on the engine's stream; the host waits once per batch of rounds.
int flow_run(cs_engine* e, const cs_flow_desc& f, uint32_t* counts_dev, const uint32_t* counts_host,
             const std::vector<uint32_t>& extra, HostHlpField* planner, float* out_vxy, double* out_dist,
             cs_flow_stats* stats) {
  const cs_field_desc& d = f.raster;
  const uint32_t nx = d.nx, ny = d.ny;
  const size_t bins = (size_t)nx * ny;
  const uint32_t tiles_x = (nx + FLOW_T - 1u) / FLOW_T, tiles_y = (ny + FLOW_T - 1u) / FLOW_T, n_tiles = tiles_x * tiles_y;
  const bool want_vec = planner || out_vxy;
  const bool vec_scratch = out_vxy && !planner;
  // the scratch: [header 256 | dist | s | vxy? | slowness? | counts? | extra? | act0 | act1 | mask | goals | blocked?]
  const size_t b_hdr = 256u, b_f64 = sel_up(bins * sizeof(double)), b_vec = vec_scratch ? sel_up(bins * sizeof(float2)) : 0u;
  const size_t b_slow = f.slowness ? sel_up(bins * sizeof(float)) : 0u;
  const size_t b_cnt = counts_host ? sel_up(bins * sizeof(uint32_t)) : 0u;
  const size_t b_extra = sel_up(extra.size() * sizeof(uint32_t));
  const size_t b_act = sel_up((size_t)n_tiles * sizeof(uint32_t)), b_u8 = sel_up(bins);
  const size_t need = b_hdr + 2u * b_f64 + b_vec + b_slow + b_cnt + b_extra + 2u * b_act + (f.blocked ? 3u : 2u) * b_u8;
  if (int rc = flow_scratch_reserve(e, need)) return rc;
  unsigned char* p = static_cast<unsigned char*>(e->flow_scratch.get());
  uint32_t* hdr = reinterpret_cast<uint32_t*>(p);  // [0 .. FLOW_BATCH): the rounds' counters; byte 64: reached (u64)
  unsigned long long* reached_dev = reinterpret_cast<unsigned long long*>(p + 64u);
  p += b_hdr;
  double* dist = reinterpret_cast<double*>(p); p += b_f64;
  double* sv = reinterpret_cast<double*>(p); p += b_f64;
  float2* vec = vec_scratch ? reinterpret_cast<float2*>(p) : planner ? planner->data.get() : nullptr; p += b_vec;
  float* slow = f.slowness ? reinterpret_cast<float*>(p) : nullptr; p += b_slow;
  uint32_t* cnt = counts_host ? reinterpret_cast<uint32_t*>(p) : counts_dev; p += b_cnt;
  uint32_t* extra_dev = reinterpret_cast<uint32_t*>(p); p += b_extra;
  uint32_t* act[2];
  act[0] = reinterpret_cast<uint32_t*>(p); p += b_act;
  act[1] = reinterpret_cast<uint32_t*>(p); p += b_act;
  uint8_t* mask = p; p += b_u8;
  uint8_t* goals = p; p += b_u8;
  uint8_t* blocked = f.blocked ? p : nullptr;

  hipStream_t st = e->stream;
  HIP_OK_E(e, hipMemsetAsync(e->flow_scratch.get(), 0, b_hdr, st));
  HIP_OK_E(e, hipMemcpyAsync(goals, f.goals, bins, hipMemcpyHostToDevice, st));
  if (blocked) HIP_OK_E(e, hipMemcpyAsync(blocked, f.blocked, bins, hipMemcpyHostToDevice, st));
  if (slow) HIP_OK_E(e, hipMemcpyAsync(slow, f.slowness, bins * sizeof(float), hipMemcpyHostToDevice, st));
  if (counts_host) HIP_OK_E(e, hipMemcpyAsync(cnt, counts_host, bins * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (!extra.empty() && counts_dev) {
    HIP_OK_E(e, hipMemcpyAsync(extra_dev, extra.data(), extra.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_flow_extra, dim3((uint32_t)((extra.size() + FLOW_DIR_BLOCK - 1u) / FLOW_DIR_BLOCK)), dim3(FLOW_DIR_BLOCK),
                       0, st, extra_dev, (uint32_t)extra.size(), (uint32_t)bins, counts_dev);
  }
  const uint32_t bin_blocks = (uint32_t)((bins + FLOW_DIR_BLOCK - 1u) / FLOW_DIR_BLOCK);
  hipLaunchKernelGGL(k_flow_init, dim3(bin_blocks), dim3(FLOW_DIR_BLOCK), 0, st, nx, ny, goals, blocked, slow, cnt,
                     f.density_weight, sv, dist, mask, n_tiles, act[0], act[1]);
  HIP_OK_E(e, hipGetLastError());

  FlowLens len;
  len.w = d.cell_w;
  len.h = d.cell_h;
  len.d = std::sqrt(d.cell_w * d.cell_w + d.cell_h * d.cell_h);
  const uint64_t cap = (uint64_t)bins + 1u;
  uint64_t rounds = 0;
  bool done = false;
  while (!done) {
    if (rounds >= cap) {
      HIP_OK_E(e, hipStreamSynchronize(st));
      e->error = "flow_field_solve: no fixed point within nx * ny + 1 rounds";
      return 90;
    }
    const uint32_t batch = (uint32_t)std::min<uint64_t>(FLOW_BATCH, cap - rounds);
    HIP_OK_E(e, hipMemsetAsync(hdr, 0, FLOW_BATCH * sizeof(uint32_t), st));
    for (uint32_t r = 0; r < batch; ++r) {
      const uint64_t round = rounds + r;
      hipLaunchKernelGGL(k_flow_relax, dim3(n_tiles), dim3(FLOW_BLOCK), 0, st, nx, ny, tiles_x, tiles_y, sv, mask, dist,
                         act[round & 1u], act[(round + 1u) & 1u], hdr + r, len);
    }
    HIP_OK_E(e, hipGetLastError());
    uint32_t changed[FLOW_BATCH] = {0u, 0u, 0u, 0u};
    HIP_OK_E(e, hipMemcpyAsync(changed, hdr, sizeof changed, hipMemcpyDeviceToHost, st));
    HIP_OK_E(e, hipStreamSynchronize(st));
    for (uint32_t r = 0; r < batch && !done; ++r) {
      rounds += 1u;
      done = changed[r] == 0u;  // (the rounds after it found no active tile)
    }
  }

  FlowVecs vecs;
  for (uint32_t k = 0; k < 8u; ++k) {
    const double sx = (double)flow_dx(k) * d.cell_w, sy = (double)flow_dy(k) * d.cell_h, n = flow_len(len, k);
    vecs.v[k] = make_float2((float)((f.speed * sx) / n), (float)((f.speed * sy) / n));
  }
  if (want_vec || stats) {
    hipLaunchKernelGGL(k_flow_dir, dim3(bin_blocks), dim3(FLOW_DIR_BLOCK), 0, st, nx, ny, goals, sv, mask, dist, len, vecs,
                       want_vec ? vec : nullptr, reached_dev);
    HIP_OK_E(e, hipGetLastError());
  }
  unsigned long long reached = 0;
  if (out_vxy) HIP_OK_E(e, hipMemcpyAsync(out_vxy, vec, bins * sizeof(float2), hipMemcpyDeviceToHost, st));
  if (out_dist) HIP_OK_E(e, hipMemcpyAsync(out_dist, dist, bins * sizeof(double), hipMemcpyDeviceToHost, st));
  if (stats) HIP_OK_E(e, hipMemcpyAsync(&reached, reached_dev, sizeof reached, hipMemcpyDeviceToHost, st));
  if (out_vxy || out_dist || stats) HIP_OK_E(e, hipStreamSynchronize(st));
  if (stats) {
    stats->reached = reached;
    stats->rounds = (uint32_t)std::min<uint64_t>(rounds, UINT32_MAX);
    stats->reserved = 0u;
  }
  return 0;
}

}  // namespace

extern "C" {

int cs_flow_field_solve(cs_engine* e, const cs_flow_desc* desc, uint32_t hlp, float* out_vxy, double* out_dist,
                        cs_flow_stats* stats) {
  if (!e) return 3;
  if (int rc = flow_check(&e->error, desc, out_vxy, out_dist, hlp)) return rc;
  HostHlpField* planner = nullptr;
  if (int rc = flow_planner(e, desc->raster, hlp, &planner)) return rc;
  hipSetDevice(e->device);
  if (e->poisoned) {
    e->error = e->poison_error;
    return 1;
  }
  const bool density = desc->density_weight != 0.0;
  FieldDev dev;
  std::vector<uint32_t> extra;
  if (density) {
    if (int rc = sel_begin(e)) return rc;
    const cs_selection s = desc->density_filter ? *desc->density_filter : cs_selection{};
    if (int rc = field_run(e, desc->raster, s, false, false, &dev)) return rc;
    for (const cs_engine::LimboAgent& l : e->limbo) {
      uint32_t ix = 0, iy = 0;
      if (sel_limbo(e, s, l) && field_bin(desc->raster, l.x, l.y, &ix, &iy)) extra.push_back(iy * desc->raster.nx + ix);
    }
  }
  return flow_run(e, *desc, density ? dev.cnt : nullptr, nullptr, extra, planner, out_vxy, out_dist, stats);
}

// Collective with equal arguments.  The counts come by cs_mesh_agent_field (the same bytes on every rank); then every tile
// solves the same problem into its own copy of the planner's samples.  Outputs are the first local tile's.
int cs_mesh_flow_field_solve(cs_mesh* m, const cs_flow_desc* desc, uint32_t hlp, float* out_vxy, double* out_dist,
                             cs_flow_stats* stats) {
  if (!m) return 3;
  if (m->dead()) return m->poison_rc;
  if (int rc = flow_check(&m->error, desc, out_vxy, out_dist, hlp)) return rc;
  std::vector<HostHlpField*> planners;
  for (cs_engine* e : m->tiles) {
    HostHlpField* p = nullptr;
    if (int rc = flow_planner(e, desc->raster, hlp, &p)) return m->fail(e, rc);
    planners.push_back(p);
  }
  std::vector<uint32_t> counts;
  if (desc->density_weight != 0.0) {
    counts.assign((size_t)desc->raster.nx * desc->raster.ny, 0u);
    if (int rc = cs_mesh_agent_field(m, &desc->raster, desc->density_filter, counts.data(), nullptr, nullptr)) return rc;
  }
  if (m->tiles.empty() && (out_vxy || out_dist || stats)) {
    m->error = "flow_field_solve: this rank holds no tile to take the outputs from";
    return 3;
  }
  const std::vector<uint32_t> none;
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    cs_engine* e = m->tiles[k];
    hipSetDevice(e->device);
    const bool first = k == 0;
    if (int rc = flow_run(e, *desc, nullptr, counts.empty() ? nullptr : counts.data(), none, planners[k],
                          first ? out_vxy : nullptr, first ? out_dist : nullptr, first ? stats : nullptr))
      return m->fail(e, rc);
    if (hlp == UINT32_MAX) break;  // (nothing to write into on the other tiles)
  }
  return 0;
}

}  // extern "C"
