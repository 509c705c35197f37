// cs_field.hip.inc — rasterising the crowd between steps: per bin of a host-given raster the number of agents and the sum
// of their velocities (include/crowdstep_state.h, cs_agent_field).  Part of the single translation unit
// crowdstep_hip.hip (included there, after cs_select.hip.inc: it reuses sel_begin, sel_load, sel_pred and the group table).
//
// A raster costs O(agents), not O(agents x bins) as counting one rectangle per bin would (DESIGN.md section 2,
// "Rasterising the crowd between steps"):
//   K_field   k_field, one lane per slot and stride: the f64 position cs_read_agents reports (sel_load), the bin by
//             field_bin (one subtraction, one correctly rounded division per axis, the range test, then the truncation),
//             the filter by sel_pred.  Slots are in cell order after a step, so neighbouring lanes usually share a bin:
//             a lane compares its bin with the lane before it, the heads of the runs are balloted, the count of a run is
//             the distance to the next head, the sums are a segmented shuffle reduction that stops at the longest run
//             of the wave, and ONLY THE HEAD of a run issues atomics.  Nothing here relies on the order of the slots: an
//             unsorted crowd gives shorter runs, so more atomics, and the same raster.
//   <true>    the raster privatised in the workgroup's LDS (ds_add_u32 / ds_add_f64), flushed once per workgroup, the
//             non-empty bins only: for rasters of at most field_lds_limit() bytes (4 B a bin, 20 B with sums)
//   <false>   the heads add to the raster in global memory (global_atomic_add / global_atomic_add_f64: the scratch is
//             coarse-grained hipMalloc memory, where the hardware f64 add is valid; no compare-and-swap loop)
//   bbox      for a mesh: the bounding box of the bins a tile touched (wave reduction, four atomics per wave), so that
//             only that part of the raster leaves the device and the rank
// The raster lives in cs_engine::field_scratch, grown on demand, zeroed on the stream before the kernel.  Nothing here
// changes a flag of the engine; the step kernels are not touched.

#define FIELD_BLOCK 256u
#define FIELD_NONE 0xFFFFFFFFu          // the bin of a lane that contributes nothing
#define FIELD_LDS_MAX_BYTES 65536u      // the most LDS a workgroup of k_field<true> may ask for

// The bin of a point, exactly as include/crowdstep_state.h writes it: fx = (x - x0) / cell_w in f64 (the library is built
// without contraction and without fast-math: one IEEE subtraction, one IEEE division, no reciprocal), inside iff
// 0 <= fx < nx (a NaN or an infinity fails), and only then ix = (uint32_t)fx.  Host and device: the agents the index
// never took are binned by the host with the same function.
__host__ __device__ inline bool field_bin(const cs_field_desc& d, double x, double y, uint32_t* ix, uint32_t* iy) {
  const double fx = (x - d.x0) / d.cell_w, fy = (y - d.y0) / d.cell_h;
  if (!(0.0 <= fx && fx < (double)d.nx && 0.0 <= fy && fy < (double)d.ny)) return false;
  *ix = (uint32_t)fx;
  *iy = (uint32_t)fy;
  return true;
}

// K_field.  cnt / svx / svy: the raster's channels (nx * ny each, zero at the start; svx and svy only with want_sums).
// box (may be null): min ix, min iy (start at UINT32_MAX), max ix, max iy (start at 0) of the bins touched.
// LDS: the dynamic shared memory holds [svx | svy] (with want_sums) and cnt for the whole raster.
// The bounds of the loop are the same for every lane of a workgroup, so the ballots and shuffles see whole waves.
template <bool LDS>
__global__ void __launch_bounds__(FIELD_BLOCK)
    k_field(GridDev g, AgentArrays a, uint32_t n_ub, const Counters* __restrict__ ctr, uint32_t tile, uint32_t owned_only,
            const SelGroupDev* __restrict__ groups, uint32_t n_groups, double grid_off_x, double grid_off_y,
            double cell_size, cs_field_desc d, cs_selection s, uint32_t want_sums, uint32_t load_vel,
            uint32_t* __restrict__ cnt, double* __restrict__ svx, double* __restrict__ svy, uint32_t* __restrict__ box) {
  extern __shared__ double field_lds[];
  const uint32_t bins = d.nx * d.ny;
  double* l_vx = field_lds;
  double* l_vy = field_lds + (want_sums ? bins : 0u);
  uint32_t* l_cnt = reinterpret_cast<uint32_t*>(field_lds + (want_sums ? 2u * bins : 0u));
  if (LDS) {
    for (uint32_t j = threadIdx.x; j < bins; j += FIELD_BLOCK) {
      l_cnt[j] = 0u;
      if (want_sums) {
        l_vx[j] = 0.0;
        l_vy[j] = 0.0;
      }
    }
    __syncthreads();
  }
  const uint32_t limit = tile ? min(n_ub, ctr->n_pending) : n_ub;
  const uint32_t lane = __lane_id();
  uint32_t bx0 = UINT32_MAX, by0 = UINT32_MAX, bx1 = 0u, by1 = 0u;
  const uint64_t stride = (uint64_t)gridDim.x * FIELD_BLOCK;
  for (uint64_t base = (uint64_t)blockIdx.x * FIELD_BLOCK; base < limit; base += stride) {
    const uint64_t i = base + threadIdx.x;
    SelAgent ag;
    bool hit = sel_load(g, a, i < limit ? (uint32_t)i : limit, limit, owned_only, groups, n_groups, grid_off_x, grid_off_y,
                        cell_size, load_vel != 0u, &ag);
    hit = hit && sel_pred(s, ag.x, ag.y, ag.vx, ag.vy, ag.wp, ag.g.sink, ag.g.hlp, ag.g.lp);
    uint32_t ix = 0u, iy = 0u;
    hit = hit && field_bin(d, ag.x, ag.y, &ix, &iy);
    const uint32_t bin = hit ? iy * d.nx + ix : FIELD_NONE;
    if (hit) {
      bx0 = min(bx0, ix); bx1 = max(bx1, ix);
      by0 = min(by0, iy); by1 = max(by1, iy);
    }
    // the runs of equal bins in this wave: heads, and for every lane the lane after the end of its run
    const uint32_t before = (uint32_t)__shfl_up((int)bin, 1, 64);
    const unsigned long long heads = __ballot(lane == 0u || bin != before);
    const unsigned long long above = lane == 63u ? 0ull : heads >> (lane + 1u);
    const uint32_t end = above ? lane + (uint32_t)__ffsll(above) : 64u;
    double vx = ag.vx, vy = ag.vy;
    if (want_sums) {
      // `longer`: the lanes that begin dist non-heads in a row, so non-zero while some run is longer than dist
      unsigned long long longer = ~heads;
      for (uint32_t dist = 1u; dist < 64u && longer; dist <<= 1) {
        const double ox = __shfl_down(vx, dist, 64), oy = __shfl_down(vy, dist, 64);
        if (lane + dist < end) {
          vx += ox;
          vy += oy;
        }
        longer &= longer >> dist;
      }
    }
    if (bin != FIELD_NONE && (heads >> lane & 1ull)) {
      const uint32_t n = end - lane;
      if (LDS) {
        atomicAdd(&l_cnt[bin], n);
        if (want_sums) {
          atomicAdd(&l_vx[bin], vx);
          atomicAdd(&l_vy[bin], vy);
        }
      } else {
        atomicAdd(&cnt[bin], n);
        if (want_sums) {
          atomicAdd(&svx[bin], vx);
          atomicAdd(&svy[bin], vy);
        }
      }
    }
  }
  if (box) {
    for (int dist = 32; dist >= 1; dist >>= 1) {
      bx0 = min(bx0, (uint32_t)__shfl_xor((int)bx0, dist, 64));
      by0 = min(by0, (uint32_t)__shfl_xor((int)by0, dist, 64));
      bx1 = max(bx1, (uint32_t)__shfl_xor((int)bx1, dist, 64));
      by1 = max(by1, (uint32_t)__shfl_xor((int)by1, dist, 64));
    }
    if (lane == 0u && bx0 != UINT32_MAX) {
      atomicMin(&box[0], bx0);
      atomicMin(&box[1], by0);
      atomicMax(&box[2], bx1);
      atomicMax(&box[3], by1);
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < bins; j += FIELD_BLOCK) {
      const uint32_t n = l_cnt[j];
      if (!n) continue;
      atomicAdd(&cnt[j], n);
      if (want_sums) {
        atomicAdd(&svx[j], l_vx[j]);
        atomicAdd(&svy[j], l_vy[j]);
      }
    }
  }
}

namespace {

// every refusal of the list in include/crowdstep_state.h (3), decided before anything is touched
int field_check(std::string* error, const cs_field_desc* d, const cs_selection* filter, const uint32_t* out_count,
                const double* out_sum_vx, const double* out_sum_vy) {
  auto refuse = [&](const char* why) {
    *error = std::string("agent_field: ") + why;
    return 3;
  };
  if (!d) return refuse("null raster description");
  if (!std::isfinite(d->x0) || !std::isfinite(d->y0) || !std::isfinite(d->cell_w) || !std::isfinite(d->cell_h))
    return refuse("a non-finite origin or bin size");
  if (!(d->cell_w > 0.0) || !(d->cell_h > 0.0)) return refuse("a bin size that is not above zero");
  if (!d->nx || !d->ny) return refuse("a raster without bins");
  if ((uint64_t)d->nx * (uint64_t)d->ny > (uint64_t)CS_FIELD_MAX_CELLS) return refuse("more than CS_FIELD_MAX_CELLS (4194304) bins");
  if (!out_count && !out_sum_vx && !out_sum_vy) return refuse("no output given");
  if ((out_sum_vx == nullptr) != (out_sum_vy == nullptr)) return refuse("one velocity output without the other");
  if (filter) return sel_check(error, filter, "agent_field");
  return 0;
}

// the raster of the last field_run of an engine, in its scratch
struct FieldDev {
  uint32_t* cnt = nullptr;
  double* svx = nullptr;
  double* svy = nullptr;
  uint32_t* box = nullptr;
};

// Rasters up to this many bytes are privatised in LDS.  Set from the table of tools/field_bench.py (DESIGN.md section
// 8): where both forms exist the LDS form was never the slower one, so the limit is what a workgroup may ask for.
// CS_FIELD_LDS_BYTES (development and tests: time and check both forms on the same raster) lowers it; 0: never.
size_t field_lds_limit() {
  size_t limit = FIELD_LDS_MAX_BYTES;
  if (const char* v = std::getenv("CS_FIELD_LDS_BYTES")) limit = std::min<size_t>(limit, (size_t)std::strtoull(v, nullptr, 10));
  return limit;
}

int field_scratch_reserve(cs_engine* e, size_t need) {
  return scratch_reserve(e, e->field_scratch, need, "agent_field: out of device memory for the raster");
}

// K_field on one engine (after sel_begin): the raster of its (owned) slots in its scratch, zeroed and filled on the
// stream; nothing is waited for.  One memset and one kernel (and a 16-byte upload for the box).
int field_run(cs_engine* e, const cs_field_desc& d, const cs_selection& s, bool want_sums, bool want_box, FieldDev* out) {
  const size_t bins = (size_t)d.nx * d.ny;
  const size_t b_cnt = sel_up(bins * sizeof(uint32_t)), b_sum = want_sums ? sel_up(bins * sizeof(double)) : 0u;
  if (int rc = field_scratch_reserve(e, 256u + b_cnt + 2u * b_sum)) return rc;
  unsigned char* sc = static_cast<unsigned char*>(e->field_scratch.get());
  out->box = reinterpret_cast<uint32_t*>(sc);
  out->cnt = reinterpret_cast<uint32_t*>(sc + 256u);
  out->svx = want_sums ? reinterpret_cast<double*>(sc + 256u + b_cnt) : nullptr;
  out->svy = want_sums ? reinterpret_cast<double*>(sc + 256u + b_cnt + b_sum) : nullptr;
  HIP_OK_E(e, hipMemsetAsync(sc, 0, 256u + b_cnt + 2u * b_sum, e->stream));  // (all-zero bits: 0 and +0.0)
  if (want_box) HIP_OK_E(e, hipMemsetAsync(out->box, 0xFF, 2u * sizeof(uint32_t), e->stream));
  const uint32_t n = e->n_slots;
  if (!n) return 0;
  const size_t lds = bins * (sizeof(uint32_t) + (want_sums ? 2u * sizeof(double) : 0u));
  const bool in_lds = lds <= field_lds_limit();
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || n_cu <= 0) n_cu = 256;
  const uint64_t per_cu = in_lds ? (lds > 16384u ? 2u : 4u) : 8u;  // (a workgroup zeroes and flushes what it privatises)
  const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n + FIELD_BLOCK - 1u) / FIELD_BLOCK, (uint64_t)n_cu * per_cu));
  const uint32_t load_vel = (want_sums || (s.terms & CS_SEL_SPEED)) ? 1u : 0u;
  auto kernel = in_lds ? k_field<true> : k_field<false>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(FIELD_BLOCK), in_lds ? lds : 0u, e->stream, e->gdev, e->buf[e->cur], n,
                     e->ctr.get(), e->tile ? 1u : 0u, (e->tile && e->ghosts_present) ? 1u : 0u, e->sel_groups_dev.get(),
                     (uint32_t)e->groups.size(), e->grid.offset_x, e->grid.offset_y, e->grid.cell_size, d, s,
                     want_sums ? 1u : 0u, load_vel, out->cnt, out->svx, out->svy, want_box ? out->box : nullptr);
  HIP_OK_E(e, hipGetLastError());
  return 0;
}

// one agent the index never took into host rasters (cnt / svx / svy may be null)
void field_add_host(const cs_field_desc& d, double x, double y, double vx, double vy, uint32_t* cnt, double* svx, double* svy) {
  uint32_t ix = 0, iy = 0;
  if (!field_bin(d, x, y, &ix, &iy)) return;
  const size_t bin = (size_t)iy * d.nx + ix;
  if (cnt) cnt[bin] += 1u;
  if (svx) {
    svx[bin] += vx;
    svy[bin] += vy;
  }
}

// A rank's contribution to cs_mesh_agent_field, 8-byte words: [failed?], then per local tile [ix0, iy0, w, h] (w == 0:
// the tile touched no bin) and the w x h part of its raster, row by row: the counts as u32, two to a word, then (with
// sums) the f64 sums of vx and of vy.  Its size depends on the raster and the tiles, not on the crowd.
size_t field_words_u32(size_t n) { return (n + 1u) / 2u; }  // words that hold n u32

}  // namespace

extern "C" {

int cs_agent_field(cs_engine* e, const cs_field_desc* desc, const cs_selection* filter, uint32_t* out_count,
                   double* out_sum_vx, double* out_sum_vy) {
  if (!e) return 3;
  hipSetDevice(e->device);
  if (int rc = field_check(&e->error, desc, filter, out_count, out_sum_vx, out_sum_vy)) return rc;
  if (int rc = sel_begin(e)) return rc;
  const cs_selection s = filter ? *filter : cs_selection{};
  const bool want_sums = out_sum_vx != nullptr;
  const size_t bins = (size_t)desc->nx * desc->ny;
  FieldDev dev;
  if (int rc = field_run(e, *desc, s, want_sums, false, &dev)) return rc;
  // one copy per channel asked for, straight into the caller's arrays
  if (out_count) HIP_OK_E(e, hipMemcpyAsync(out_count, dev.cnt, bins * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  if (want_sums) {
    HIP_OK_E(e, hipMemcpyAsync(out_sum_vx, dev.svx, bins * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK_E(e, hipMemcpyAsync(out_sum_vy, dev.svy, bins * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  }
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  for (const cs_engine::LimboAgent& l : e->limbo)  // (as cs_read_agents lists them: where they were created, at rest)
    if (sel_limbo(e, s, l)) field_add_host(*desc, l.x, l.y, 0.0, 0.0, out_count, out_sum_vx, out_sum_vy);
  return 0;
}

// Collective.  Every tile rasterises what it owns and reports the bounding box of the bins it touched; only that part
// of its raster leaves the device.  One gather of variable size carries [failed?, per tile: box, sub-rasters]; every
// rank adds the parts in (rank, local tile) order, then the mesh's own list of the agents the index never took.
int cs_mesh_agent_field(cs_mesh* m, const cs_field_desc* desc, const cs_selection* filter, uint32_t* out_count,
                        double* out_sum_vx, double* out_sum_vy) {
  if (!m) return 3;
  if (m->dead()) return m->poison_rc;
  if (int rc = field_check(&m->error, desc, filter, out_count, out_sum_vx, out_sum_vy)) return rc;
  if (int rc = cs_mesh_synchronize(m)) return rc;
  hipSetDevice(m->device);
  const cs_field_desc d = *desc;
  const cs_selection s = filter ? *filter : cs_selection{};
  const bool want_sums = out_sum_vx != nullptr;
  const size_t bins = (size_t)d.nx * d.ny;
  std::vector<uint64_t> mine(1, 0u);
  std::string why;
  for (cs_engine* e : m->tiles) {
    if (mine[0]) break;
    FieldDev dev;
    uint32_t box[4] = {UINT32_MAX, UINT32_MAX, 0u, 0u};
    int rc = sel_begin(e);
    if (!rc) rc = field_run(e, d, s, want_sums, true, &dev);
    if (!rc && (hipMemcpyAsync(box, dev.box, sizeof box, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
                hipStreamSynchronize(e->stream) != hipSuccess)) {
      e->error = "agent_field: HIP error while reading a tile's raster";
      rc = 90;
    }
    const bool empty = box[0] == UINT32_MAX;
    if (!rc && !empty && (box[2] >= d.nx || box[3] >= d.ny || box[0] > box[2] || box[1] > box[3])) {
      e->error = "agent_field: a tile's bounding box lies outside the raster";
      rc = 90;
    }
    const size_t w = empty ? 0u : (size_t)box[2] - box[0] + 1u, h = empty ? 0u : (size_t)box[3] - box[1] + 1u;
    const size_t at = mine.size(), w_cnt = field_words_u32(w * h), w_sum = want_sums ? w * h : 0u;
    if (!rc) {
      mine.resize(at + 4u + w_cnt + 2u * w_sum, 0u);
      mine[at] = empty ? 0u : box[0];
      mine[at + 1u] = empty ? 0u : box[1];
      mine[at + 2u] = w;
      mine[at + 3u] = h;
    }
    if (!rc && !empty) {
      const size_t first = (size_t)box[1] * d.nx + box[0];
      hipError_t err = hipMemcpy2DAsync(&mine[at + 4u], w * sizeof(uint32_t), dev.cnt + first, (size_t)d.nx * sizeof(uint32_t),
                                        w * sizeof(uint32_t), h, hipMemcpyDeviceToHost, e->stream);
      if (err == hipSuccess && want_sums)
        err = hipMemcpy2DAsync(&mine[at + 4u + w_cnt], w * sizeof(double), dev.svx + first, (size_t)d.nx * sizeof(double),
                               w * sizeof(double), h, hipMemcpyDeviceToHost, e->stream);
      if (err == hipSuccess && want_sums)
        err = hipMemcpy2DAsync(&mine[at + 4u + w_cnt + w_sum], w * sizeof(double), dev.svy + first,
                               (size_t)d.nx * sizeof(double), w * sizeof(double), h, hipMemcpyDeviceToHost, e->stream);
      if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
      if (err != hipSuccess) {
        e->error = "agent_field: HIP error while reading a tile's raster";
        rc = 90;
      }
    }
    if (rc) {
      mine.assign(1, 1u);
      why = cs_last_error(e);
    }
  }
  m->field_gather_bytes = mine.size() * sizeof(uint64_t);
  std::vector<std::vector<unsigned char>> parts;
  if (m->distributed) {
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), parts)) return m->poison(rc, m->error);
  } else {
    parts.emplace_back(reinterpret_cast<const unsigned char*>(mine.data()),
                       reinterpret_cast<const unsigned char*>(mine.data()) + mine.size() * sizeof(uint64_t));
  }
  // every rank adds the same parts in the same order: (rank, local tile), so the sums are the same bits everywhere
  std::vector<uint32_t> cnt(out_count ? bins : 0u, 0u);
  std::vector<double> svx(want_sums ? bins : 0u, 0.0), svy(want_sums ? bins : 0u, 0.0);
  bool failed = false, malformed = false;
  for (const auto& part : parts) {
    const size_t words = part.size() / sizeof(uint64_t);
    std::vector<uint64_t> wds(words);
    if (words) std::memcpy(wds.data(), part.data(), words * sizeof(uint64_t));
    if (!words || wds[0]) {
      failed = true;
      continue;
    }
    size_t at = 1u;
    while (at < words && !malformed) {
      if (at + 4u > words) { malformed = true; break; }
      const uint64_t ix0 = wds[at], iy0 = wds[at + 1u], w = wds[at + 2u], h = wds[at + 3u];
      at += 4u;
      if (!w || !h) continue;
      if (ix0 + w > d.nx || iy0 + h > d.ny) { malformed = true; break; }
      const size_t w_cnt = field_words_u32((size_t)(w * h)), w_sum = want_sums ? (size_t)(w * h) : 0u;
      if (at + w_cnt + 2u * w_sum > words) { malformed = true; break; }
      const uint32_t* p_cnt = reinterpret_cast<const uint32_t*>(&wds[at]);
      const double* p_vx = reinterpret_cast<const double*>(&wds[at + w_cnt]);
      const double* p_vy = reinterpret_cast<const double*>(&wds[at + w_cnt + w_sum]);
      for (size_t r = 0; r < h; ++r)
        for (size_t c = 0; c < w; ++c) {
          const size_t bin = (size_t)(iy0 + r) * d.nx + (size_t)(ix0 + c), k = r * (size_t)w + c;
          if (!p_cnt[k]) continue;  // (a bin the tile did not touch: its sums are +0.0)
          if (out_count) cnt[bin] += p_cnt[k];
          if (want_sums) {
            svx[bin] += p_vx[k];
            svy[bin] += p_vy[k];
          }
        }
      at += w_cnt + 2u * w_sum;
    }
  }
  if (failed || malformed) {
    m->error = !why.empty() ? why
               : malformed  ? "agent_field: a malformed contribution of a rank"
                            : "a tile of another rank failed while rasterising agents";
    return 90;
  }
  for (const cs_mesh::Limbo& l : m->limbo)
    if (sel_limbo(s, l))
      field_add_host(d, l.view.x, l.view.y, l.view.vx, l.view.vy, out_count ? cnt.data() : nullptr,
                     want_sums ? svx.data() : nullptr, want_sums ? svy.data() : nullptr);
  if (out_count) std::memcpy(out_count, cnt.data(), bins * sizeof(uint32_t));
  if (want_sums) {
    std::memcpy(out_sum_vx, svx.data(), bins * sizeof(double));
    std::memcpy(out_sum_vy, svy.data(), bins * sizeof(double));
  }
  return 0;
}

uint64_t cs_mesh_field_gather_bytes(const cs_mesh* m) { return m ? m->field_gather_bytes : 0u; }

}  // extern "C"
