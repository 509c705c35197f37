// cs_rays.hip.inc — rays against the crowd between steps: for each ray the first agent whose disc of `radius` it enters and
// the parameter where it does (include/crowdstep_state.h, "Rays against the crowd between steps").  Part of the single
// translation unit crowdstep_hip.hip (included there, after cs_encounters.hip.inc; it uses pairs_args, pairs_in_grid,
// near_roles and PairsScratch of cs_near.hip.inc, sel_begin / sel_check / sel_up of cs_select.hip.inc and
// mesh_host_gatherv of cs_mesh.hip.inc, and changes none of them).
//
//   K_rays   k_cast_rays, one 64-lane wave per ray, four rays per workgroup.  Everything the walk decides is computed
//            from the ray alone, so it is the same in all the lanes of a wave: the wave walks the grid rows the ray meets,
//            in the order it meets them; in row xr the cells that matter are ONE interval of columns, hence one run of slots
//            of the CELL-SORTED arrays, taken RAYS_CHUNK columns at a time in the order the ray meets them; the lanes
//            stride the slots of a chunk.  A lane rebuilds a candidate's position with near_walk's expression (the
//            position cs_read_agents reports), applies the rule (ray_rule) and keeps its best (t, id); t >= +0.0, so its
//            bit pattern orders as an unsigned integer.  The participant test and the selection (near_roles) are
//            evaluated only for a candidate that would become the lane's best.  After every chunk the wave takes the
//            minimum of the lanes' t (shuffles); at the end lane 0 writes the lexicographic minimum of (t, id).
//   host     one upload of the rays (the `ignore` ids mapped to device ids), one kernel, one download of the hits.
//   mesh     every tile casts ALL rays against the agents it owns (the walk is clipped to the owned cells, the ray stays in
//            world coordinates); the rows are merged by the lexicographic minimum of (t, id); one gather.
//
// WHY THE WALK IS CONSERVATIVE.  Write cs for the cell size, R for the radius and grow = R + cs.  A hit of the rule on
// participant q at parameter t means, in exact arithmetic, that the point E = o + u * t lies within R of q (on the circle,
// or E = o inside the disc at t = 0) with 0 <= t < t_max.  A participant's offset lies in [0, cs] of the cell it is indexed
// under up to one rounding (see cs_near.hip.inc), so E lies in that cell's rectangle grown by R.  The rule's rounding moves
// what it decides by far less than a cell: rx and ry carry half an ulp of the larger of the two coordinates they subtract,
// cr and b one more relative 2^-52 of |r| |u|, so the perpendicular and the along-ray distance are off by at most about
// 2^-51 (|o| + |x_q|) metres; for coordinates within 2^32 cells (the walk's own limit, below) that is 2^-19 of a cell.
// The walk grows every rectangle by grow, a WHOLE cell more than R, and computes its clips with single f64 operations on
// values of the same size, so their rounding (again relative 2^-52) is below the spare cell by the same margin.  Hence:
//   * the ray is clipped, in f64 and before any integer is formed, to [ta, tb]: the part of [0, t_max] inside the (owned)
//     grid's rectangle grown by grow.  An axis with u == 0 divides nothing: the origin is inside the slab or the ray
//     visits nothing.  Every hit has ta <= t <= tb.
//   * row xr is visited when its slab [xr * cs - grow, (xr + 1) * cs + grow] meets the x range of the clipped segment,
//     for the part [s0, s1] of [ta, tb] the ray spends in that slab; its columns are those whose slab (grown likewise)
//     meets the y range of that part.  Row and column numbers are clamped to the (owned) grid as f64 values and only
//     then converted.
//   * EARLY EXIT.  Every hit in row xr has t >= s0(xr), the parameter at which the ray enters that row's grown slab, and
//     s0 does not decrease along the order of the rows; every hit in a chunk of columns has t >= the parameter at which
//     the ray enters the chunk's grown slab, which does not decrease along the order of the chunks.  The wave stops a
//     row's chunks, or the rows, when its best t is STRICTLY below that bound: a candidate with an equal t (and maybe a
//     smaller id) is still visited.
//   * an origin or a radius beyond 2^32 cells of the local grid's corner (where the roundings above are no longer small
//     against a cell, and where +inf would meet 0 in a product) takes no clip at all: the wave visits every (owned) cell,
//     without early exit.
//
// Scratch: the rays (48 bytes each) and the hits (16 bytes each) through PairsScratch: kept while at most
// PAIRS_SCRATCH_KEEP, else allocated for the call and freed before it returns.

#define RAYS_CHUNK 16u           // columns of a row taken between two looks at the wave's best t
#define RAYS_NOBODY 0xFFFFFFFFu  // no device id
#define RAYS_FAR_CELLS 4294967296.0  // 2^32

static_assert(sizeof(cs_ray) == 48 && sizeof(cs_ray_hit) == 16, "rays and hits travel as they are declared");

// The rule for one ray and the candidate at (xq, yq): one f64 operation per line of the header, rounded once each.
__device__ __forceinline__ bool ray_rule(double ox, double oy, double ux, double uy, double uu, double R2, double t_max,
                                         double xq, double yq, double* t_out) {
  const double rx = xq - ox, ry = yq - oy;
  const double d2 = rx * rx + ry * ry;
  double t = 0.0;
  if (!(d2 < R2)) {
    const double b = rx * ux + ry * uy;
    if (!(b > 0.0)) return false;
    const double cr = rx * uy - ry * ux;
    const double h2 = R2 * uu - cr * cr;
    if (!(h2 > 0.0)) return false;
    t = (b - __dsqrt_rn(h2)) / uu;
    if (t < 0.0) t = 0.0;
  }
  *t_out = t;
  return t < t_max;
}

// [ta, tb] cut to the parameters at which q + u * t lies in [lo, hi]; false: none left.  u == 0 divides nothing.
__device__ __forceinline__ bool ray_slab(double q, double u, double lo, double hi, double* ta, double* tb) {
  if (u == 0.0) return lo <= q && q <= hi;
  const double t1 = (lo - q) / u, t2 = (hi - q) / u;
  *ta = fmax(*ta, fmin(t1, t2));
  *tb = fmin(*tb, fmax(t1, t2));
  return *ta <= *tb;
}

__device__ __forceinline__ unsigned long long rays_wave_min(unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ uint32_t rays_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// K_rays.  rays[k].ignore holds a DEVICE id (or CS_NO_HIT); out[k].id is a device id (or CS_NO_HIT).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_cast_rays(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                const SelGroupDev* __restrict__ groups, PairsArgs P, double grow, const cs_ray* __restrict__ rays,
                uint32_t n_rays, cs_ray_hit* __restrict__ out) {
  const uint32_t k = rays_uniform(blockIdx.x * PAIRS_WAVES + (threadIdx.x >> 6));
  if (k >= n_rays) return;  // (the whole wave)
  const uint32_t lane = __lane_id();
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);  // the sorted arrays hold the live agents in front
  const cs_ray r = rays[k];
  const double cs = P.cell_size, R2 = P.dist2;
  const double uu = r.ux * r.ux + r.uy * r.uy;
  const uint32_t ign = r.ignore < (uint64_t)RAYS_NOBODY ? (uint32_t)r.ignore : RAYS_NOBODY;
  // the (owned) grid: rows are x, g.ny of them; columns are y, g.nx of them
  const uint32_t lo_x = P.owned_only ? g.own_x0 : 0u, hi_x = P.owned_only ? g.own_x1 : g.ny;
  const uint32_t lo_y = P.owned_only ? g.own_y0 : 0u, hi_y = P.owned_only ? g.own_y1 : g.nx;
  unsigned long long best_t = 0x7FF0000000000000ull;  // the bits of +inf
  uint32_t best_id = RAYS_NOBODY;
  double wbest = __longlong_as_double((long long)best_t);  // the wave's best t so far
  bool any = lo_x < hi_x && lo_y < hi_y && limit != 0u;
  // the ray in metres from the low corner of local cell (0, 0)
  const double qx = r.ox - (P.off_x + (double)g.org_x * cs), qy = r.oy - (P.off_y + (double)g.org_y * cs);
  const double far = RAYS_FAR_CELLS * cs;
  const bool full = !(fabs(qx) < far && fabs(qy) < far && grow < far);
  double ta = 0.0, tb = r.t_max;
  double rlo = (double)lo_x, rhi = (double)hi_x - 1.0;
  if (any && !full) {
    any = ray_slab(qx, r.ux, (double)lo_x * cs - grow, (double)hi_x * cs + grow, &ta, &tb) &&
          ray_slab(qy, r.uy, (double)lo_y * cs - grow, (double)hi_y * cs + grow, &ta, &tb);
    if (any) {  // (tb is finite here: one of ux, uy is not zero and its slab is bounded)
      const double xa = qx + r.ux * ta, xb = qx + r.ux * tb;
      rlo = fmax(floor((fmin(xa, xb) - grow) / cs) - 1.0, rlo);
      rhi = fmin(floor((fmax(xa, xb) + grow) / cs), rhi);
      any = rlo <= rhi;
    }
  }
  if (any) {
    const uint32_t r0 = rays_uniform((uint32_t)rlo), r1 = rays_uniform((uint32_t)rhi);  // (clamped to [lo_x, hi_x) above)
    const bool up = !(r.ux < 0.0);
    for (uint32_t i = 0; i <= r1 - r0; ++i) {
      const uint32_t xr = up ? r0 + i : r1 - i;
      double s0 = 0.0, s1 = 0.0;
      double clo = (double)lo_y, chi = (double)hi_y - 1.0;
      if (!full) {
        s0 = ta;
        s1 = tb;
        if (r.ux != 0.0) {
          const double t1 = (((double)xr * cs - grow) - qx) / r.ux, t2 = ((((double)xr + 1.0) * cs + grow) - qx) / r.ux;
          s0 = fmax(ta, fmin(t1, t2));
          s1 = fmin(tb, fmax(t1, t2));
        }
        if (!(s0 <= s1)) continue;
        if (wbest < s0) break;  // every row from here on is entered later than the best hit
        const double ya = qy + r.uy * s0, yb = qy + r.uy * s1;
        clo = fmax(floor((fmin(ya, yb) - grow) / cs) - 1.0, clo);
        chi = fmin(floor((fmax(ya, yb) + grow) / cs), chi);
        if (!(clo <= chi)) continue;
      }
      const uint32_t c0 = rays_uniform((uint32_t)clo), c1 = rays_uniform((uint32_t)chi);  // (clamped to [lo_y, hi_y))
      const uint32_t rowbase = xr * g.nx;  // (below ncells, which fits 32 bits)
      const double bx = (double)((uint64_t)g.org_x + (uint64_t)xr) * cs;
      const bool yup = !(r.uy < 0.0);
      const unsigned long long ncols = (unsigned long long)(c1 - c0) + 1ull;
      for (unsigned long long done = 0; done < ncols; done += RAYS_CHUNK) {
        const uint32_t len = (uint32_t)min((unsigned long long)RAYS_CHUNK, ncols - done);
        const uint32_t a0 = yup ? c0 + (uint32_t)done : c1 - (uint32_t)done - (len - 1u);
        const uint32_t a1 = a0 + (len - 1u);
        if (!full) {
          double lb = s0;
          if (r.uy > 0.0) lb = fmax(lb, (((double)a0 * cs - grow) - qy) / r.uy);
          if (r.uy < 0.0) lb = fmax(lb, ((((double)a1 + 1.0) * cs + grow) - qy) / r.uy);
          if (wbest < lb) break;  // every chunk of this row from here on is entered later than the best hit
        }
        const uint32_t b = cell_start[rowbase + a0];
        const uint32_t e = min(cell_start[rowbase + a1 + 1u], limit);  // (index <= ncells: the table has ncells + 1)
        for (uint32_t j = b + lane; j < e; j += 64u) {
          const uint32_t idj = a.id[j];
          if (idj == ign) continue;
          const uint32_t cyj = a.cell[j] - rowbase;
          if (cyj > a1) continue;  // (a slot that is not of this row's run: cannot happen in sorted arrays)
          const float2 off = a.off[j];
          const double xq = P.off_x + (bx + (double)off.x);
          const double yq = P.off_y + ((double)((uint64_t)g.org_y + cyj) * cs + (double)off.y);
          double t;
          if (!ray_rule(r.ox, r.oy, r.ux, r.uy, uu, R2, r.t_max, xq, yq, &t)) continue;
          const unsigned long long tbits = (unsigned long long)__double_as_longlong(t);
          if (!(tbits < best_t || (tbits == best_t && idj < best_id))) continue;
          if (!pairs_in_grid(P, xq, yq)) continue;
          if (!(near_roles(g, a, j, groups, P, xq, yq, 3u) & 1u)) continue;  // (role A: the targets)
          best_t = tbits;
          best_id = idj;
        }
        wbest = __longlong_as_double((long long)rays_wave_min(best_t));
      }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {  // the lexicographic minimum of (t, id) over the wave
    const uint32_t lo = __shfl_xor((uint32_t)best_t, d, 64), hi = __shfl_xor((uint32_t)(best_t >> 32), d, 64);
    const uint32_t oid = __shfl_xor(best_id, d, 64);
    const unsigned long long ot = ((unsigned long long)hi << 32) | lo;
    if (ot < best_t || (ot == best_t && oid < best_id)) {
      best_t = ot;
      best_id = oid;
    }
  }
  if (lane == 0u) {
    cs_ray_hit h;
    h.id = best_id == RAYS_NOBODY ? CS_NO_HIT : (uint64_t)best_id;
    h.t = __longlong_as_double((long long)best_t);
    out[k] = h;
  }
}

namespace {

const cs_ray_hit kRayMiss = {CS_NO_HIT, std::numeric_limits<double>::infinity()};

// the refusals of the header (3); the text names the first bad ray
int rays_check(std::string* error, const cs_ray* rays, size_t n, double radius, const cs_selection* targets) {
  if (n > CS_RAYS_MAX) {
    *error = "cast_rays: more rays than CS_RAYS_MAX = 1048576 in one call";
    return 3;
  }
  if (n && !rays) {
    *error = "cast_rays: null rays";
    return 3;
  }
  if (!(radius >= 0.0)) {
    *error = "cast_rays: the radius is NaN or negative";
    return 3;
  }
  if (targets)
    if (int rc = sel_check(error, targets, "cast_rays")) return rc;
  for (size_t k = 0; k < n; ++k) {
    const cs_ray& r = rays[k];
    const char* what = nullptr;
    if (!(std::isfinite(r.ox) && std::isfinite(r.oy))) {
      what = "its origin is not finite";
    } else if (!(std::isfinite(r.ux) && std::isfinite(r.uy))) {
      what = "its direction is not finite";
    } else {
      const double uu = r.ux * r.ux + r.uy * r.uy;
      if (!(uu >= 0x1p-100 && uu <= 0x1p100)) what = "the squared length of its direction is outside [2^-100, 2^100]";
      else if (!(r.t_max >= 0.0)) what = "its t_max is NaN or negative";
    }
    if (what) {
      *error = "cast_rays: ray " + std::to_string(k) + ": " + what;
      return 3;
    }
  }
  return 0;
}

// All n rays (n > 0) against the agents one engine holds (after sel_begin), into rows[0 .. n) as DEVICE ids.  One upload,
// one kernel, one download, one synchronise.
int rays_run(cs_engine* e, const cs_ray* rays, size_t n, double radius, const cs_selection* targets,
             std::vector<cs_ray_hit>* rows) {
  rows->assign(n, kRayMiss);
  if (int rc = e->refresh_counts()) return rc;
  if (int rc = e->ensure_index()) return rc;
  if (!e->n_slots) return 0;
  const PairsArgs P = pairs_args(e, radius, targets, nullptr);
  std::vector<cs_ray> mine(rays, rays + n);
  for (cs_ray& r : mine) {  // the way the by-id calls map ids: an id no live agent can hold is nobody's
    uint64_t dev = 0;
    const bool known = r.ignore != CS_NO_HIT && e->dev_id(r.ignore, &dev) && dev < e->id_limit && dev < 0xFFFFFFFFull;
    r.ignore = known ? dev : CS_NO_HIT;
  }
  PairsScratch sc(e);
  const size_t b_rays = sel_up(n * sizeof(cs_ray));
  unsigned char* p = static_cast<unsigned char*>(sc.get(b_rays + n * sizeof(cs_ray_hit)));
  if (!p) return 90;
  cs_ray* d_rays = reinterpret_cast<cs_ray*>(p);
  cs_ray_hit* d_hits = reinterpret_cast<cs_ray_hit*>(p + b_rays);
  HIP_OK_E(e, hipMemcpyAsync(d_rays, mine.data(), n * sizeof(cs_ray), hipMemcpyHostToDevice, e->stream));
  const uint32_t blocks = ((uint32_t)n + PAIRS_WAVES - 1u) / PAIRS_WAVES;
  hipLaunchKernelGGL(k_cast_rays, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], e->n_slots,
                     e->cell_start.get(), e->sel_groups_dev.get(), P, radius + e->grid.cell_size, d_rays, (uint32_t)n, d_hits);
  HIP_OK_E(e, hipGetLastError());
  HIP_OK_E(e, hipMemcpyAsync(rows->data(), d_hits, n * sizeof(cs_ray_hit), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (the host staging of the rays dies here)
  return 0;
}

// row k of `into` = the lexicographic minimum of (t, id) of it and row k of `from` (t >= +0.0 or +inf: never a NaN)
void rays_merge(std::vector<cs_ray_hit>* into, const cs_ray_hit* from) {
  for (size_t k = 0; k < into->size(); ++k) {
    cs_ray_hit& h = (*into)[k];
    if (from[k].t < h.t || (from[k].t == h.t && from[k].id < h.id)) h = from[k];
  }
}

// device ids -> external ids into the caller's rows (may be null); the number of rays that hit something
size_t rays_copy_out(const cs_engine* ids_of, const std::vector<cs_ray_hit>& rows, cs_ray_hit* out) {
  size_t hits = 0;
  for (size_t k = 0; k < rows.size(); ++k) {
    const bool hit = rows[k].id != CS_NO_HIT;
    hits += hit ? 1u : 0u;
    if (!out) continue;
    out[k].id = hit ? ids_of->ext_id(rows[k].id) : CS_NO_HIT;
    out[k].t = rows[k].t;
  }
  return hits;
}

}  // namespace

extern "C" {

size_t cs_cast_rays(cs_engine* e, const cs_ray* rays, size_t n, double radius, const cs_selection* targets,
                    cs_ray_hit* out) {
  if (!e) return SIZE_MAX;
  hipSetDevice(e->device);
  if (rays_check(&e->error, rays, n, radius, targets)) return SIZE_MAX;
  if (sel_begin(e)) return SIZE_MAX;
  if (!n) return 0;
  std::vector<cs_ray_hit> rows;
  if (rays_run(e, rays, n, radius, targets, &rows)) return SIZE_MAX;
  return rays_copy_out(e, rows, out);
}

// Collective: ONE gather of variable size (two collectives), whatever the crowd and the answer: a rank sends its failure
// word and, unless it failed, the n rows that are the minimum over its tiles.  n == 0 makes none: every rank passes the
// same n.  No halo exchange, no band: a tile's walk is clipped to the cells it owns and every agent is owned by one tile.
size_t cs_mesh_cast_rays(cs_mesh* m, const cs_ray* rays, size_t n, double radius, const cs_selection* targets,
                         cs_ray_hit* out) {
  if (!m) return SIZE_MAX;
  if (m->dead()) return SIZE_MAX;
  if (rays_check(&m->error, rays, n, radius, targets)) return SIZE_MAX;
  if (cs_mesh_synchronize(m)) return SIZE_MAX;
  hipSetDevice(m->device);
  if (!n) return 0;
  int err = 0;
  std::string why;
  std::vector<cs_ray_hit> best(n, kRayMiss), part;
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    cs_engine* e = m->tiles[k];
    if (!err) err = sel_begin(e);
    if (!err) err = rays_run(e, rays, n, radius, targets, &part);
    if (err && why.empty()) why = cs_last_error(e);
    if (!err) rays_merge(&best, part.data());
  }
  if (m->distributed) {
    static_assert(sizeof(cs_ray_hit) == 2u * sizeof(uint64_t), "hits travel as two 8-byte words");
    std::vector<uint64_t> mine(1u + (err ? 0u : 2u * n), err ? 1u : 0u);
    if (!err) std::memcpy(&mine[1], best.data(), n * sizeof(cs_ray_hit));
    std::vector<std::vector<unsigned char>> parts;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), parts)) {
      m->poison(rc, m->error);
      return SIZE_MAX;
    }
    std::vector<cs_ray_hit> theirs(n);
    for (const auto& p : parts) {
      uint64_t failed = 1u;
      if (p.size() >= sizeof failed) std::memcpy(&failed, p.data(), sizeof failed);
      if (failed || p.size() != sizeof(uint64_t) + n * sizeof(cs_ray_hit)) {
        if (!err) {
          err = 90;
          why = "a tile of another rank failed while casting rays";
        }
        continue;
      }
      std::memcpy(theirs.data(), p.data() + sizeof(uint64_t), n * sizeof(cs_ray_hit));
      rays_merge(&best, theirs.data());
    }
  }
  if (err) {
    m->error = why;
    return SIZE_MAX;
  }
  if (m->tiles.empty()) {
    if (out) std::fill(out, out + n, kRayMiss);
    return 0;
  }
  return rays_copy_out(m->tiles[0], best, out);
}

}  // extern "C"
