// cs_legs.hip.inc — timed path legs against the moving crowd between steps: for each leg the first agent that comes within
// `distance` of a probe moving at constant velocity, if every agent keeps the velocity it has now, and the time after the
// leg's start at which it does (include/crowdstep_state.h, "Paths against the moving crowd between steps").  Part of the
// single translation unit crowdstep_hip.hip (included there, after cs_rays.hip.inc; it uses ray_slab, rays_uniform,
// RAYS_CHUNK, RAYS_NOBODY and RAYS_FAR_CELLS of that file, pairs_args, pairs_in_grid, near_roles and PairsScratch of
// cs_near.hip.inc, sel_begin / sel_check / sel_up of cs_select.hip.inc and mesh_host_gatherv of cs_mesh.hip.inc, and
// changes none of them).
//
//   K_legs   k_leg_conflicts, one 64-lane wave per leg, four legs per workgroup.  Everything the walk decides is computed
//            from the leg alone, so it is the same in all the lanes of a wave: the wave walks the grid rows that meet the
//            segment the probe sweeps, grown by the leg's own reach; in row xr the cells that matter are ONE interval of
//            columns, hence one run of slots of the CELL-SORTED arrays, taken RAYS_CHUNK columns at a time; the lanes stride
//            the slots of a chunk.  A lane rebuilds a candidate's position with near_walk's expression (the position
//            cs_read_agents reports), widens its f32 velocity, applies the speed test and the rule (leg_rule) and keeps its
//            best (s, id); s >= +0.0, so its bit pattern orders as an unsigned integer.  The participant test and the
//            selection (near_roles) are evaluated only for a candidate that would become the lane's best.  At the end
//            lane 0 writes the lexicographic minimum of (s, id) over the wave.
//   host     one upload of the legs (the `ignore` ids mapped to device ids), one kernel, one download of the hits.
//   mesh     every tile runs ALL legs against the agents it owns (the walk is clipped to the owned cells, the leg stays in
//            world coordinates); the rows are merged by the lexicographic minimum of (s, id); one gather.
//
// WHY A BOUNDED SEARCH IS SOUND.  A conflict of the rule on participant q at s means, in exact arithmetic, that at time
// t0 + s, with 0 <= s < T = t1 - t0, the probe at E = (x0, y0) + v * s and the agent at x_q + v_q * (t0 + s) are within
// `distance` of one another (on the circle, or inside it at s = 0).  q is considered only if |v_q| < speed_max, and
// t0 + s < t1, so the agent has moved less than speed_max * t1 from where it stands NOW: its present position, the one the
// cell index knows, lies within  G = distance + speed_max * t1  of the point E of the swept segment (x0, y0) + v * [0, T].
// Agents that are faster are left out by the rule itself, not by the walk.
//
// WHY THE WALK IS CONSERVATIVE.  Write cs for the cell size and grow = G + cs, from THIS leg's t1.  A participant's offset
// lies in [0, cs] of the cell it is indexed under up to one rounding (see cs_near.hip.inc), so E lies in that cell's
// rectangle grown by G.  The rule's rounding moves what it decides by far less than a cell: px and py carry half an ulp
// of |x_q| + |v_q| t0 each (|v_q| t0 < speed_max * t1 <= grow, below 2^32 cells), rx and ry half an ulp of the larger of
// the two coordinates they subtract, a, cr and ww one more relative 2^-52, so the distance the rule measures is off by at
// most about 2^-50 (|x0| + |x_q| + grow) metres; for coordinates and a reach within 2^32 cells (the walk's own limit,
// below) that is 2^-18 of a cell.  The walk grows every rectangle by grow, a WHOLE cell more than G, and computes its clips
// with single f64 operations on values of the same size, so their rounding (again relative 2^-52) is below the spare cell
// by the same margin.  Hence:
//   * the leg is clipped, in f64 and before any integer is formed, to [sa, sb]: the part of [0, T] the probe spends inside
//     the (owned) grid's rectangle grown by grow.  An axis with v == 0 divides nothing: the start is inside the slab or
//     the leg visits nothing; a waiting leg takes that branch on both axes and keeps [0, T].  Every conflict has its E at
//     a parameter in [sa, sb].
//   * row xr is visited when its slab [xr * cs - grow, (xr + 1) * cs + grow] meets the x range of the clipped segment, for
//     the part [s0, s1] of [sa, sb] the probe spends in that slab; its columns are those whose slab (grown likewise) meets
//     the y range of that part.  Row and column numbers are clamped to the (owned) grid as f64 values and only then
//     converted.
//   * NO EARLY EXIT.  The cell a candidate stands in now says where the probe is when they meet only up to G, and nothing
//     about when: an agent far along the segment may walk towards the probe and arrive before a near one.  Every row and
//     every chunk of the capsule is visited.
//   * a start, or a reach, at or beyond 2^32 cells of the local grid's corner (where the roundings above are no longer
//     small against a cell, and where +inf would meet 0 in a product: speed_max = +inf, distance = +inf) takes no clip at
//     all: the wave visits every (owned) cell.  A NaN reach (+inf * 0 at t1 == 0) does the same.
//
// Scratch: the legs (56 bytes each) and the hits (16 bytes each) through PairsScratch: kept while at most
// PAIRS_SCRATCH_KEEP, else allocated for the call and freed before it returns.

static_assert(sizeof(cs_leg) == 56 && sizeof(cs_leg_hit) == 16, "legs and hits travel as they are declared");

// The rule for one leg and the candidate at (xq, yq) with velocity (vxq, vyq): one f64 operation per operation of the
// header, rounded once each.  S2 = speed_max * speed_max, D2 = distance * distance, T = t1 - t0.
__device__ __forceinline__ bool leg_rule(const cs_leg& l, double S2, double D2, double T, double xq, double yq, double vxq,
                                         double vyq, double* s_out) {
  const double ss = vxq * vxq + vyq * vyq;
  if (!(ss < S2)) return false;
  const double px = xq + vxq * l.t0, py = yq + vyq * l.t0;
  const double rx = px - l.x0, ry = py - l.y0;
  const double d2 = rx * rx + ry * ry;
  double s = 0.0;
  if (!(d2 < D2)) {
    const double wx = vxq - l.vx, wy = vyq - l.vy;
    const double a = rx * wx + ry * wy;
    if (!(a < 0.0)) return false;
    const double ww = wx * wx + wy * wy;
    const double cr = rx * wy - ry * wx;
    const double h2 = D2 * ww - cr * cr;
    if (!(h2 > 0.0)) return false;
    s = (-a - __dsqrt_rn(h2)) / ww;
    if (s < 0.0) s = 0.0;
  }
  *s_out = s;
  return s < T;
}

// K_legs.  legs[k].ignore holds a DEVICE id (or CS_NO_HIT); out[k].id is a device id (or CS_NO_HIT).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_leg_conflicts(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                    const SelGroupDev* __restrict__ groups, PairsArgs P, double distance, double speed_max,
                    const cs_leg* __restrict__ legs, uint32_t n_legs, cs_leg_hit* __restrict__ out) {
  const uint32_t k = rays_uniform(blockIdx.x * PAIRS_WAVES + (threadIdx.x >> 6));
  if (k >= n_legs) return;  // (the whole wave)
  const uint32_t lane = __lane_id();
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);  // the sorted arrays hold the live agents in front
  const cs_leg l = legs[k];
  const double cs = P.cell_size, D2 = P.dist2, S2 = speed_max * speed_max, T = l.t1 - l.t0;
  const double grow = (distance + speed_max * l.t1) + cs;  // this leg's reach and the spare cell
  const uint32_t ign = l.ignore < (uint64_t)RAYS_NOBODY ? (uint32_t)l.ignore : RAYS_NOBODY;
  // the (owned) grid: rows are x, g.ny of them; columns are y, g.nx of them
  const uint32_t lo_x = P.owned_only ? g.own_x0 : 0u, hi_x = P.owned_only ? g.own_x1 : g.ny;
  const uint32_t lo_y = P.owned_only ? g.own_y0 : 0u, hi_y = P.owned_only ? g.own_y1 : g.nx;
  unsigned long long best_s = 0x7FF0000000000000ull;  // the bits of +inf
  uint32_t best_id = RAYS_NOBODY;
  bool any = lo_x < hi_x && lo_y < hi_y && limit != 0u && T > 0.0 && D2 > 0.0;  // (s >= 0 is never below T == 0)
  // the start of the leg in metres from the low corner of local cell (0, 0)
  const double qx = l.x0 - (P.off_x + (double)g.org_x * cs), qy = l.y0 - (P.off_y + (double)g.org_y * cs);
  const double far = RAYS_FAR_CELLS * cs;
  const bool full = !(fabs(qx) < far && fabs(qy) < far && grow < far);
  double sa = 0.0, sb = T;
  double rlo = (double)lo_x, rhi = (double)hi_x - 1.0;
  if (any && !full) {
    any = ray_slab(qx, l.vx, (double)lo_x * cs - grow, (double)hi_x * cs + grow, &sa, &sb) &&
          ray_slab(qy, l.vy, (double)lo_y * cs - grow, (double)hi_y * cs + grow, &sa, &sb);
    if (any) {  // (sb <= T is finite)
      const double xa = qx + l.vx * sa, xb = qx + l.vx * sb;
      rlo = fmax(floor((fmin(xa, xb) - grow) / cs) - 1.0, rlo);
      rhi = fmin(floor((fmax(xa, xb) + grow) / cs), rhi);
      any = rlo <= rhi;
    }
  }
  if (any) {
    const uint32_t r0 = rays_uniform((uint32_t)rlo), r1 = rays_uniform((uint32_t)rhi);  // (clamped to [lo_x, hi_x) above)
    for (uint32_t xr = r0;; ++xr) {
      double clo = (double)lo_y, chi = (double)hi_y - 1.0;
      bool row = true;
      if (!full) {
        double s0 = sa, s1 = sb;
        if (l.vx != 0.0) {
          const double t1 = (((double)xr * cs - grow) - qx) / l.vx, t2 = ((((double)xr + 1.0) * cs + grow) - qx) / l.vx;
          s0 = fmax(sa, fmin(t1, t2));
          s1 = fmin(sb, fmax(t1, t2));
        }
        row = s0 <= s1;
        if (row) {
          const double ya = qy + l.vy * s0, yb = qy + l.vy * s1;
          clo = fmax(floor((fmin(ya, yb) - grow) / cs) - 1.0, clo);
          chi = fmin(floor((fmax(ya, yb) + grow) / cs), chi);
          row = clo <= chi;
        }
      }
      if (row) {
        const uint32_t c0 = rays_uniform((uint32_t)clo), c1 = rays_uniform((uint32_t)chi);  // (clamped to [lo_y, hi_y))
        const uint32_t rowbase = xr * g.nx;  // (below ncells, which fits 32 bits)
        const double bx = (double)((uint64_t)g.org_x + (uint64_t)xr) * cs;
        const unsigned long long ncols = (unsigned long long)(c1 - c0) + 1ull;
        for (unsigned long long done = 0; done < ncols; done += RAYS_CHUNK) {
          const uint32_t len = (uint32_t)min((unsigned long long)RAYS_CHUNK, ncols - done);
          const uint32_t a0 = c0 + (uint32_t)done, a1 = a0 + (len - 1u);
          const uint32_t b = cell_start[rowbase + a0];
          const uint32_t e = min(cell_start[rowbase + a1 + 1u], limit);  // (index <= ncells: the table has ncells + 1)
          for (uint32_t j = b + lane; j < e; j += 64u) {
            const uint32_t idj = a.id[j];
            if (idj == ign) continue;
            const uint32_t cyj = a.cell[j] - rowbase;
            if (cyj > a1) continue;  // (a slot that is not of this row's run: cannot happen in sorted arrays)
            const float2 off = a.off[j], vel = a.vel[j];
            const double xq = P.off_x + (bx + (double)off.x);
            const double yq = P.off_y + ((double)((uint64_t)g.org_y + cyj) * cs + (double)off.y);
            double s;
            if (!leg_rule(l, S2, D2, T, xq, yq, (double)vel.x, (double)vel.y, &s)) continue;
            const unsigned long long sbits = (unsigned long long)__double_as_longlong(s);
            if (!(sbits < best_s || (sbits == best_s && idj < best_id))) continue;
            if (!pairs_in_grid(P, xq, yq)) continue;
            if (!(near_roles(g, a, j, groups, P, xq, yq, 3u) & 1u)) continue;  // (role A: the targets)
            best_s = sbits;
            best_id = idj;
          }
        }
      }
      if (xr == r1) break;  // (r1 may be the last row a uint32_t can name)
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {  // the lexicographic minimum of (s, id) over the wave
    const uint32_t lo = __shfl_xor((uint32_t)best_s, d, 64), hi = __shfl_xor((uint32_t)(best_s >> 32), d, 64);
    const uint32_t oid = __shfl_xor(best_id, d, 64);
    const unsigned long long os = ((unsigned long long)hi << 32) | lo;
    if (os < best_s || (os == best_s && oid < best_id)) {
      best_s = os;
      best_id = oid;
    }
  }
  if (lane == 0u) {
    cs_leg_hit h;
    h.id = best_id == RAYS_NOBODY ? CS_NO_HIT : (uint64_t)best_id;
    h.s = __longlong_as_double((long long)best_s);
    out[k] = h;
  }
}

namespace {

const cs_leg_hit kLegMiss = {CS_NO_HIT, std::numeric_limits<double>::infinity()};

// the refusals of the header (3), under the name of the call; the text names the first bad leg
int legs_check(std::string* error, const std::string& call, const cs_leg* legs, size_t n, double distance, double speed_max,
               const cs_selection* targets) {
  if (n > CS_LEGS_MAX) {
    *error = call + ": more legs than CS_LEGS_MAX = 1048576 in one call";
    return 3;
  }
  if (n && !legs) {
    *error = call + ": null legs";
    return 3;
  }
  if (!(distance >= 0.0)) {
    *error = call + ": the distance is NaN or negative";
    return 3;
  }
  if (!(speed_max >= 0.0)) {
    *error = call + ": speed_max is NaN or negative";
    return 3;
  }
  if (targets)
    if (int rc = sel_check(error, targets, call.c_str())) return rc;
  for (size_t k = 0; k < n; ++k) {
    const cs_leg& l = legs[k];
    const char* what = nullptr;
    if (!(std::isfinite(l.x0) && std::isfinite(l.y0))) what = "its start is not finite";
    else if (!(std::isfinite(l.vx) && std::isfinite(l.vy))) what = "its velocity is not finite";
    else if (!(std::isfinite(l.t0) && std::isfinite(l.t1))) what = "its times are not finite";
    else if (l.t0 < 0.0) what = "its t0 is negative";
    else if (l.t1 < l.t0) what = "its t1 is before its t0";
    if (what) {
      *error = call + ": leg " + std::to_string(k) + ": " + what;
      return 3;
    }
  }
  return 0;
}

// the legs with their `ignore` ids mapped to DEVICE ids, the way the by-id calls map ids: an id no live agent can hold is
// nobody's
std::vector<cs_leg> legs_with_device_ids(const cs_engine* e, const cs_leg* legs, size_t n) {
  std::vector<cs_leg> mine(legs, legs + n);
  for (cs_leg& l : mine) {
    uint64_t dev = 0;
    const bool known = l.ignore != CS_NO_HIT && e->dev_id(l.ignore, &dev) && dev < e->id_limit && dev < 0xFFFFFFFFull;
    l.ignore = known ? dev : CS_NO_HIT;
  }
  return mine;
}

// All n legs (n > 0) against the agents one engine holds (after sel_begin), into rows[0 .. n) as DEVICE ids.  One upload,
// one kernel, one download, one synchronise.
int legs_run(cs_engine* e, const cs_leg* legs, size_t n, double distance, double speed_max, const cs_selection* targets,
             std::vector<cs_leg_hit>* rows) {
  rows->assign(n, kLegMiss);
  if (int rc = e->refresh_counts()) return rc;
  if (int rc = e->ensure_index()) return rc;
  if (!e->n_slots) return 0;
  const PairsArgs P = pairs_args(e, distance, targets, nullptr);
  const std::vector<cs_leg> mine = legs_with_device_ids(e, legs, n);
  PairsScratch sc(e);
  const size_t b_legs = sel_up(n * sizeof(cs_leg));
  unsigned char* p = static_cast<unsigned char*>(sc.get(b_legs + n * sizeof(cs_leg_hit)));
  if (!p) return 90;
  cs_leg* d_legs = reinterpret_cast<cs_leg*>(p);
  cs_leg_hit* d_hits = reinterpret_cast<cs_leg_hit*>(p + b_legs);
  HIP_OK_E(e, hipMemcpyAsync(d_legs, mine.data(), n * sizeof(cs_leg), hipMemcpyHostToDevice, e->stream));
  const uint32_t blocks = ((uint32_t)n + PAIRS_WAVES - 1u) / PAIRS_WAVES;
  hipLaunchKernelGGL(k_leg_conflicts, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], e->n_slots,
                     e->cell_start.get(), e->sel_groups_dev.get(), P, distance, speed_max, d_legs, (uint32_t)n, d_hits);
  HIP_OK_E(e, hipGetLastError());
  HIP_OK_E(e, hipMemcpyAsync(rows->data(), d_hits, n * sizeof(cs_leg_hit), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (the host staging of the legs dies here)
  return 0;
}

// row k of `into` = the lexicographic minimum of (s, id) of it and row k of `from` (s >= +0.0 or +inf: never a NaN)
void legs_merge(std::vector<cs_leg_hit>* into, const cs_leg_hit* from) {
  for (size_t k = 0; k < into->size(); ++k) {
    cs_leg_hit& h = (*into)[k];
    if (from[k].s < h.s || (from[k].s == h.s && from[k].id < h.id)) h = from[k];
  }
}

// device ids -> external ids into the caller's rows (may be null); the number of legs with a conflict
size_t legs_copy_out(const cs_engine* ids_of, const std::vector<cs_leg_hit>& rows, cs_leg_hit* out) {
  size_t hits = 0;
  for (size_t k = 0; k < rows.size(); ++k) {
    const bool hit = rows[k].id != CS_NO_HIT;
    hits += hit ? 1u : 0u;
    if (!out) continue;
    out[k].id = hit ? ids_of->ext_id(rows[k].id) : CS_NO_HIT;
    out[k].s = rows[k].s;
  }
  return hits;
}

}  // namespace

extern "C" {

size_t cs_leg_conflicts(cs_engine* e, const cs_leg* legs, size_t n, double distance, double speed_max,
                        const cs_selection* targets, cs_leg_hit* out) {
  if (!e) return SIZE_MAX;
  hipSetDevice(e->device);
  if (legs_check(&e->error, "leg_conflicts", legs, n, distance, speed_max, targets)) return SIZE_MAX;
  if (sel_begin(e)) return SIZE_MAX;
  if (!n) return 0;
  std::vector<cs_leg_hit> rows;
  if (legs_run(e, legs, n, distance, speed_max, targets, &rows)) return SIZE_MAX;
  return legs_copy_out(e, rows, out);
}

// Collective: ONE gather of variable size (two collectives), whatever the crowd and the answer: a rank sends its failure
// word and, unless it failed, the n rows that are the minimum over its tiles.  n == 0 makes none: every rank passes the
// same n.  No halo exchange, no band: a tile's walk is clipped to the cells it owns and every agent is owned by one tile.
size_t cs_mesh_leg_conflicts(cs_mesh* m, const cs_leg* legs, size_t n, double distance, double speed_max,
                             const cs_selection* targets, cs_leg_hit* out) {
  if (!m) return SIZE_MAX;
  if (m->dead()) return SIZE_MAX;
  if (legs_check(&m->error, "leg_conflicts", legs, n, distance, speed_max, targets)) return SIZE_MAX;
  if (cs_mesh_synchronize(m)) return SIZE_MAX;
  hipSetDevice(m->device);
  if (!n) return 0;
  int err = 0;
  std::string why;
  std::vector<cs_leg_hit> best(n, kLegMiss), part;
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    cs_engine* e = m->tiles[k];
    if (!err) err = sel_begin(e);
    if (!err) err = legs_run(e, legs, n, distance, speed_max, targets, &part);
    if (err && why.empty()) why = cs_last_error(e);
    if (!err) legs_merge(&best, part.data());
  }
  if (m->distributed) {
    static_assert(sizeof(cs_leg_hit) == 2u * sizeof(uint64_t), "hits travel as two 8-byte words");
    std::vector<uint64_t> mine(1u + (err ? 0u : 2u * n), err ? 1u : 0u);
    if (!err) std::memcpy(&mine[1], best.data(), n * sizeof(cs_leg_hit));
    std::vector<std::vector<unsigned char>> parts;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), parts)) {
      m->poison(rc, m->error);
      return SIZE_MAX;
    }
    std::vector<cs_leg_hit> theirs(n);
    for (const auto& p : parts) {
      uint64_t failed = 1u;
      if (p.size() >= sizeof failed) std::memcpy(&failed, p.data(), sizeof failed);
      if (failed || p.size() != sizeof(uint64_t) + n * sizeof(cs_leg_hit)) {
        if (!err) {
          err = 90;
          why = "a tile of another rank failed while checking legs";
        }
        continue;
      }
      std::memcpy(theirs.data(), p.data() + sizeof(uint64_t), n * sizeof(cs_leg_hit));
      legs_merge(&best, theirs.data());
    }
  }
  if (err) {
    m->error = why;
    return SIZE_MAX;
  }
  if (m->tiles.empty()) {
    if (out) std::fill(out, out + n, kLegMiss);
    return 0;
  }
  return legs_copy_out(m->tiles[0], best, out);
}

}  // extern "C"
