// cs_leg_intervals.hip.inc — timed path legs against the moving crowd between steps, the complete list: for each leg EVERY
// agent that comes within `distance` of the probe, with the seconds after the leg's start at which it enters and at which
// it leaves again (include/crowdstep_state.h, "Every agent that enters a leg").  Part of the single translation unit
// crowdstep_hip.hip (included there, after cs_legs.hip.inc; it uses legs_check and legs_with_device_ids of that file,
// ray_slab, rays_uniform, RAYS_NOBODY and RAYS_FAR_CELLS of cs_rays.hip.inc, pairs_args, pairs_in_grid, near_roles,
// pairs_wave_sum, pairs_header, pairs_read_count, pairs_read_header, pairs_radix, pairs_bits and PairsScratch of
// cs_near.hip.inc, k_encounters_gather of cs_encounters.hip.inc, sel_begin / sel_up of cs_select.hip.inc and
// mesh_host_gatherv / mesh_merge_runs of cs_mesh.hip.inc, and changes none of them).
//
//   K_count  k_leg_intervals_count, one 64-lane wave per leg, four legs per workgroup, over the capsule of k_leg_conflicts
//            (legiv_walk; why it is sound and conservative for every conflict of a leg, not only the first, is written in
//            cs_legs.hip.inc: the bound G = distance + speed_max * t1 does not depend on which conflict is meant).  The
//            wave takes 64 slots of a row's run at a time; a lane rebuilds its candidate's position with near_walk's
//            expression, applies the rule (legiv_rule), and EVERY candidate the rule passes is tested as a participant
//            and against the selection: a row is a row whoever else is one.  The wave's sum goes into counts[leg] and,
//            with one atomic, into the 64-bit total.
//   K_emit   k_leg_intervals_emit, only when listing: the same walk.  The rows of leg k go to list places
//            offsets[k] .. offsets[k + 1], the exclusive sums of the counts (made on the host, which has the counts by
//            then); the rows of one 64-slot step take consecutive places by a ballot.  A row is (leg << 32 | device id,
//            its place, s_in, s_out).
//   sort     pairs_radix over the id half (the bits of the largest id listed) and the leg half (the bits of n - 1) of the
//            key with the place as the payload; k_encounters_gather (two f64 columns by the sorted places) then brings
//            s_in and s_out of the first `want` rows into sorted order.
//   mesh     every tile runs ALL legs against the agents it owns (the walk is clipped to the owned cells, the legs stay in
//            world coordinates).  Agents are disjoint across tiles, so counts add and the rows of all tiles, merged by
//            their key, are the single engine's.  One gather for the counts, one for the rows.
//
// Scratch through PairsScratch: for the count the legs (56 bytes each) and the counts (8 bytes each); for a listing the
// legs, the offsets and six 8-byte arrays of one entry per row, with the histogram of the sort.

static_assert(sizeof(cs_leg_interval) == 32, "intervals travel as they are declared");

// The rule for one leg and the candidate at (xq, yq) with velocity (vxq, vyq): one f64 operation per operation of the
// header, rounded once each; s_in is leg_rule's s, from the same operations.  S2 = speed_max * speed_max, D2 = distance *
// distance, T = t1 - t0.
__device__ __forceinline__ bool legiv_rule(const cs_leg& l, double S2, double D2, double T, double xq, double yq,
                                           double vxq, double vyq, double* s_in, double* s_out) {
  const double ss = vxq * vxq + vyq * vyq;
  if (!(ss < S2)) return false;
  const double px = xq + vxq * l.t0, py = yq + vyq * l.t0;
  const double rx = px - l.x0, ry = py - l.y0;
  const double d2 = rx * rx + ry * ry;
  const double wx = vxq - l.vx, wy = vyq - l.vy;
  const double a = rx * wx + ry * wy;
  const double ww = wx * wx + wy * wy;
  const double cr = rx * wy - ry * wx;
  const double h2 = D2 * ww - cr * cr;
  double s = 0.0;
  if (!(d2 < D2)) {
    if (!(a < 0.0)) return false;
    if (!(h2 > 0.0)) return false;
    s = (-a - __dsqrt_rn(h2)) / ww;
    if (s < 0.0) s = 0.0;
  }
  if (!(s < T)) return false;
  double e;
  if (!(h2 > 0.0)) {
    e = ww == 0.0 ? T : s;  // the same velocity, inside: it never leaves; else rounding only
  } else {
    e = (-a + __dsqrt_rn(h2)) / ww;
    if (!(e > s)) e = s;
    if (!(e < T)) e = T;
  }
  *s_in = s;
  *s_out = e;
  return true;
}

// The walk of the wave of leg l over its capsule (the clips of k_leg_conflicts, see there; a row's columns are taken as
// one run of slots).  Every lane of the wave calls v.row(is_row, id, s_in, s_out) once per 64 slots of a run, all lanes
// together: is_row says whether the lane's slot is a row of this leg.
template <class V>
__device__ __forceinline__ void legiv_walk(const GridDev& g, const AgentArrays& a, uint32_t limit,
                                           const uint32_t* __restrict__ cell_start, const SelGroupDev* __restrict__ groups,
                                           const PairsArgs& P, double distance, double speed_max, const cs_leg& l,
                                           uint32_t lane, V& v) {
  const double cs = P.cell_size, D2 = P.dist2, S2 = speed_max * speed_max, T = l.t1 - l.t0;
  const double grow = (distance + speed_max * l.t1) + cs;  // this leg's reach and the spare cell
  const uint32_t ign = l.ignore < (uint64_t)RAYS_NOBODY ? (uint32_t)l.ignore : RAYS_NOBODY;
  // the (owned) grid: rows are x, g.ny of them; columns are y, g.nx of them
  const uint32_t lo_x = P.owned_only ? g.own_x0 : 0u, hi_x = P.owned_only ? g.own_x1 : g.ny;
  const uint32_t lo_y = P.owned_only ? g.own_y0 : 0u, hi_y = P.owned_only ? g.own_y1 : g.nx;
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
  if (!any) return;
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
      const uint32_t b = rays_uniform(cell_start[rowbase + c0]);
      const uint32_t e = rays_uniform(min(cell_start[rowbase + c1 + 1u], limit));  // (index <= ncells: the table has ncells + 1)
      for (uint32_t j0 = b; j0 < e; j0 += 64u) {  // (e <= limit is far below 2^32 - 64)
        const uint32_t j = j0 + lane;
        bool is_row = false;
        uint32_t idj = RAYS_NOBODY;
        double s_in = 0.0, s_out = 0.0;
        if (j < e) {
          idj = a.id[j];
          const uint32_t cyj = a.cell[j] - rowbase;
          if (idj != ign && cyj <= c1) {  // (a slot that is not of this row's run cannot happen in sorted arrays)
            const float2 off = a.off[j], vel = a.vel[j];
            const double xq = P.off_x + (bx + (double)off.x);
            const double yq = P.off_y + ((double)((uint64_t)g.org_y + cyj) * cs + (double)off.y);
            is_row = legiv_rule(l, S2, D2, T, xq, yq, (double)vel.x, (double)vel.y, &s_in, &s_out) &&
                     pairs_in_grid(P, xq, yq) && (near_roles(g, a, j, groups, P, xq, yq, 3u) & 1u);  // (role A: the targets)
          }
        }
        v.row(is_row, idj, s_in, s_out);
      }
    }
    if (xr == r1) break;  // (r1 may be the last row a uint32_t can name)
  }
}

struct LegivCount {
  uint32_t n;
  __device__ __forceinline__ void row(bool is_row, uint32_t, double, double) { n += is_row ? 1u : 0u; }
};

// The rows of a 64-slot step take the places at, at + 1, ... in lane order; `at` is the same in every lane.  Nothing is
// written at or beyond `end`, the first place of the next leg.
struct LegivEmit {
  unsigned long long at, end, leg_bits;
  unsigned long long* __restrict__ keys;
  double* __restrict__ index;
  double* __restrict__ s_ins;
  double* __restrict__ s_outs;
  uint32_t lane, top;
  __device__ __forceinline__ void row(bool is_row, uint32_t id, double s_in, double s_out) {
    const unsigned long long m = __ballot(is_row);
    if (is_row) {
      const unsigned long long k = at + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
      if (k < end) {
        keys[k] = leg_bits | id;
        index[k] = __longlong_as_double((long long)k);
        s_ins[k] = s_in;
        s_outs[k] = s_out;
      }
      top = max(top, id);
    }
    at += (unsigned long long)__popcll(m);
  }
};

// K_count.  legs[k].ignore holds a DEVICE id (or CS_NO_HIT).  counts[k] = the rows of leg k; hdr[0] += them (starts at 0).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_leg_intervals_count(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                          const SelGroupDev* __restrict__ groups, PairsArgs P, double distance, double speed_max,
                          const cs_leg* __restrict__ legs, uint32_t n_legs, unsigned long long* __restrict__ counts,
                          unsigned long long* __restrict__ hdr) {
  const uint32_t k = rays_uniform(blockIdx.x * PAIRS_WAVES + (threadIdx.x >> 6));
  if (k >= n_legs) return;  // (the whole wave)
  const uint32_t lane = __lane_id();
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);  // the sorted arrays hold the live agents in front
  const cs_leg l = legs[k];
  LegivCount v{0u};
  legiv_walk(g, a, limit, cell_start, groups, P, distance, speed_max, l, lane, v);
  const unsigned long long w = pairs_wave_sum(v.n);
  if (lane == 0u) {
    counts[k] = w;
    if (w) atomicAdd(&hdr[0], w);
  }
}

// K_emit.  offsets[k]: the list place of the first row of leg k (n_legs + 1 entries).  hdr[1] += the rows written (starts
// at 0), the low word of hdr[2]: the largest id listed.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_leg_intervals_emit(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                         const SelGroupDev* __restrict__ groups, PairsArgs P, double distance, double speed_max,
                         const cs_leg* __restrict__ legs, uint32_t n_legs, const unsigned long long* __restrict__ offsets,
                         unsigned long long* __restrict__ hdr, unsigned long long* __restrict__ keys,
                         double* __restrict__ index, double* __restrict__ s_ins, double* __restrict__ s_outs) {
  const uint32_t k = rays_uniform(blockIdx.x * PAIRS_WAVES + (threadIdx.x >> 6));
  if (k >= n_legs) return;  // (the whole wave)
  const unsigned long long at = offsets[k], end = offsets[k + 1u];
  if (at >= end) return;  // (no rows: the same in all the lanes)
  const uint32_t lane = __lane_id();
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);
  const cs_leg l = legs[k];
  LegivEmit v{at, end, (unsigned long long)k << 32, keys, index, s_ins, s_outs, lane, 0u};
  legiv_walk(g, a, limit, cell_start, groups, P, distance, speed_max, l, lane, v);
  uint32_t top = v.top;
  for (int d = 32; d >= 1; d >>= 1) top = max(top, (uint32_t)__shfl_xor(top, d, 64));
  if (lane == 0u) {
    atomicAdd(&hdr[1], min(v.at, end) - at);
    if (top) atomicMax(reinterpret_cast<uint32_t*>(&hdr[2]), top);
  }
}

namespace {

// one listed interval on the host: the key (leg << 32 | DEVICE id) and the two times
struct LegivRec {
  uint64_t key;
  double s_in, s_out;
};
bool operator<(const LegivRec& l, const LegivRec& r) { return l.key < r.key; }

// what one engine counted: the legs as it uploads them, the rows of each leg and of all
struct LegivPart {
  std::vector<cs_leg> legs;
  std::vector<uint64_t> counts;
  uint64_t total = 0;
};

// All n legs (n > 0) against the agents one engine holds (after sel_begin), counted: part->total, and with want_counts
// part->counts.  One memset, one upload, one kernel, one read back (and one download of the counts): no row is made.
int legiv_count(cs_engine* e, const cs_leg* legs, size_t n, double distance, double speed_max, const cs_selection* targets,
                bool want_counts, LegivPart* part) {
  part->legs.clear();
  part->counts.assign(n, 0u);
  part->total = 0;
  if (int rc = e->refresh_counts()) return rc;
  if (int rc = e->ensure_index()) return rc;
  if (!e->n_slots) return 0;
  const PairsArgs P = pairs_args(e, distance, targets, nullptr);
  part->legs = legs_with_device_ids(e, legs, n);
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  PairsScratch sc(e);
  const size_t b_legs = sel_up(n * sizeof(cs_leg));
  unsigned char* p = static_cast<unsigned char*>(sc.get(b_legs + n * sizeof(uint64_t)));
  if (!p) return 90;
  cs_leg* d_legs = reinterpret_cast<cs_leg*>(p);
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(p + b_legs);
  HIP_OK_E(e, hipMemcpyAsync(d_legs, part->legs.data(), n * sizeof(cs_leg), hipMemcpyHostToDevice, e->stream));
  const uint32_t blocks = ((uint32_t)n + PAIRS_WAVES - 1u) / PAIRS_WAVES;
  hipLaunchKernelGGL(k_leg_intervals_count, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur],
                     e->n_slots, e->cell_start.get(), e->sel_groups_dev.get(), P, distance, speed_max, d_legs, (uint32_t)n, d_counts,
                     hdr);
  HIP_OK_E(e, hipGetLastError());
  if (want_counts)
    HIP_OK_E(e, hipMemcpyAsync(part->counts.data(), d_counts, n * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
  unsigned long long found = 0;
  if (int rc = pairs_read_count(e, hdr, &found)) return rc;  // (synchronised: the host staging may go)
  part->total = found;
  return 0;
}

// The first min(part.total, want) rows of what legiv_count counted (with its counts; part.total at most CS_PAIRS_MAX),
// ascending by (leg, id), as device ids.  One memset, one upload, one kernel, one read back, three launches per 4 bits of
// the largest id and of the largest leg, one gather, one download.
int legiv_list(cs_engine* e, const LegivPart& part, double distance, double speed_max, const cs_selection* targets,
               size_t want, std::vector<LegivRec>* out) {
  out->clear();
  const size_t n = part.legs.size();
  const uint64_t found = part.total;
  if (!want || !found || !n) return 0;
  std::vector<uint64_t> offsets(n + 1u, 0u);
  for (size_t k = 0; k < n; ++k) offsets[k + 1u] = offsets[k] + part.counts[k];
  if (offsets[n] != found) {
    e->error = "leg_intervals: the counts of the legs do not add up to the total";
    return 90;
  }
  const PairsArgs P = pairs_args(e, distance, targets, nullptr);
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  PairsScratch sc(e);
  const size_t b_legs = sel_up(n * sizeof(cs_leg)), b_off = sel_up((n + 1u) * sizeof(uint64_t));
  const size_t b = sel_up((size_t)found * sizeof(uint64_t));
  const size_t tiles = ((size_t)found + IDS_TILE - 1u) / IDS_TILE;
  const size_t b_hist = sel_up(IDS_RADIX * std::max<size_t>(tiles, 1u) * sizeof(uint32_t));
  unsigned char* p = static_cast<unsigned char*>(sc.get(b_legs + b_off + 6u * b + b_hist + 256u));
  if (!p) return 90;
  cs_leg* d_legs = reinterpret_cast<cs_leg*>(p);
  unsigned long long* d_off = reinterpret_cast<unsigned long long*>(p + b_legs);
  unsigned char* q = p + b_legs + b_off;
  unsigned long long *keys = reinterpret_cast<unsigned long long*>(q), *keys_other = reinterpret_cast<unsigned long long*>(q + b);
  double *index = reinterpret_cast<double*>(q + 2u * b), *index_other = reinterpret_cast<double*>(q + 3u * b);
  double *s_ins = reinterpret_cast<double*>(q + 4u * b), *s_outs = reinterpret_cast<double*>(q + 5u * b);
  uint32_t* hist = reinterpret_cast<uint32_t*>(q + 6u * b);
  HIP_OK_E(e, hipMemcpyAsync(d_legs, part.legs.data(), n * sizeof(cs_leg), hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(d_off, offsets.data(), (n + 1u) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
  const uint32_t blocks = ((uint32_t)n + PAIRS_WAVES - 1u) / PAIRS_WAVES;
  hipLaunchKernelGGL(k_leg_intervals_emit, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur],
                     e->n_slots, e->cell_start.get(), e->sel_groups_dev.get(), P, distance, speed_max, d_legs, (uint32_t)n, d_off, hdr,
                     keys, index, s_ins, s_outs);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long back[3];
  if (int rc = pairs_read_header(e, hdr, back)) return rc;  // (synchronised: the host staging may go)
  if (back[1] != found) {
    e->error = "leg_intervals: the listing found another number of intervals than the count";
    return 90;
  }
  const uint32_t rows = (uint32_t)found;  // (at most CS_PAIRS_MAX)
  if (rows > 1u) {  // the id in the low half, the leg in the high half
    if (int rc = pairs_radix(e, &keys, &keys_other, &index, &index_other, hist, rows, 0u, pairs_bits((uint32_t)back[2])))
      return rc;
    if (n > 1u)
      if (int rc = pairs_radix(e, &keys, &keys_other, &index, &index_other, hist, rows, 32u, pairs_bits((uint32_t)(n - 1u))))
        return rc;
  }
  const uint32_t take = (uint32_t)std::min<size_t>(want, rows);
  double* in_sorted = reinterpret_cast<double*>(keys_other);
  double* out_sorted = index_other;
  std::vector<uint64_t> k_host(take);
  std::vector<double> in_host(take), out_host(take);
  hipLaunchKernelGGL(k_encounters_gather, dim3((take + PAIRS_BLOCK - 1u) / PAIRS_BLOCK), dim3(PAIRS_BLOCK), 0, e->stream,
                     index, s_ins, s_outs, take, rows, in_sorted, out_sorted);
  HIP_OK_E(e, hipGetLastError());
  HIP_OK_E(e, hipMemcpyAsync(k_host.data(), keys, take * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(in_host.data(), in_sorted, take * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(out_host.data(), out_sorted, take * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  out->resize(take);
  for (size_t k = 0; k < take; ++k) (*out)[k] = LegivRec{k_host[k], in_host[k], out_host[k]};
  return 0;
}

int legiv_too_many(std::string* error) {
  *error = "leg_intervals: too many intervals to list (more than CS_PAIRS_MAX = 67108864); the count-only form has no limit";
  return 3;
}

// device ids -> external ids, into the caller's rows
void legiv_copy_out(const cs_engine* ids_of, const std::vector<LegivRec>& list, cs_leg_interval* out, size_t cap) {
  const size_t k = std::min(list.size(), cap);
  for (size_t i = 0; i < k; ++i) {
    out[i].leg = list[i].key >> 32;
    out[i].id = ids_of->ext_id(list[i].key & 0xFFFFFFFFull);
    out[i].s_in = list[i].s_in;
    out[i].s_out = list[i].s_out;
  }
}

}  // namespace

extern "C" {

size_t cs_leg_intervals(cs_engine* e, const cs_leg* legs, size_t n, double distance, double speed_max,
                        const cs_selection* targets, uint64_t* out_counts, cs_leg_interval* out, size_t cap) {
  if (!e) return SIZE_MAX;
  hipSetDevice(e->device);
  if (legs_check(&e->error, "leg_intervals", legs, n, distance, speed_max, targets)) return SIZE_MAX;
  if (sel_begin(e)) return SIZE_MAX;
  if (!n) return 0;
  const size_t want = out ? cap : 0u;
  LegivPart part;
  if (legiv_count(e, legs, n, distance, speed_max, targets, want || out_counts, &part)) return SIZE_MAX;
  if (want && part.total > CS_PAIRS_MAX) {
    legiv_too_many(&e->error);
    return SIZE_MAX;
  }
  std::vector<LegivRec> list;
  if (legiv_list(e, part, distance, speed_max, targets, want, &list)) return SIZE_MAX;
  if (out_counts) std::copy(part.counts.begin(), part.counts.end(), out_counts);
  if (want) legiv_copy_out(e, list, out, cap);
  return (size_t)part.total;
}

// Collective: one gather of variable size (two collectives) for the counts and, when listing, one more for the rows,
// whatever the crowd and the answer: a rank that failed, or a listing that is refused, sends its word alone.  n == 0
// makes none: every rank passes the same n.  No halo exchange, no band: a tile's walk is clipped to the cells it owns and
// every agent is owned by one tile.
size_t cs_mesh_leg_intervals(cs_mesh* m, const cs_leg* legs, size_t n, double distance, double speed_max,
                             const cs_selection* targets, uint64_t* out_counts, cs_leg_interval* out, size_t cap) {
  if (!m) return SIZE_MAX;
  if (m->dead()) return SIZE_MAX;
  if (legs_check(&m->error, "leg_intervals", legs, n, distance, speed_max, targets)) return SIZE_MAX;
  if (cs_mesh_synchronize(m)) return SIZE_MAX;
  hipSetDevice(m->device);
  if (!n) return 0;
  const size_t want = out ? cap : 0u;
  const char* const other_failed = "a tile of another rank failed while listing leg intervals";
  int err = 0;
  std::string why;
  // 1. every tile counts; the counts of all tiles of all ranks: [0 ok / 1 failed, n counts]
  std::vector<LegivPart> parts(m->tiles.size());
  std::vector<uint64_t> counts(n, 0u);
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    cs_engine* e = m->tiles[k];
    if (!err) err = sel_begin(e);
    if (!err) err = legiv_count(e, legs, n, distance, speed_max, targets, true, &parts[k]);
    if (err && why.empty()) why = cs_last_error(e);
    if (!err)
      for (size_t i = 0; i < n; ++i) counts[i] += parts[k].counts[i];
  }
  if (m->distributed) {
    std::vector<uint64_t> mine(1u + (err ? 0u : n), err ? 1u : 0u);
    if (!err) std::copy(counts.begin(), counts.end(), mine.begin() + 1);
    std::vector<std::vector<unsigned char>> got;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), got)) {
      m->poison(rc, m->error);
      return SIZE_MAX;
    }
    counts.assign(n, 0u);
    std::vector<uint64_t> w(1u + n);
    for (const auto& p : got) {
      if (p.size() != w.size() * sizeof(uint64_t)) {  // (a rank that failed sends its word alone)
        if (!err) {
          err = 90;
          why = other_failed;
        }
        continue;
      }
      std::memcpy(w.data(), p.data(), p.size());
      for (size_t i = 0; i < n; ++i) counts[i] += w[1u + i];
    }
  }
  uint64_t total = 0;
  for (uint64_t c : counts) total += c;
  const bool too_many = want && total > CS_PAIRS_MAX;
  // 2. when listing: the rows of every tile, merged; then those of every rank: [0 ok / 1 failed, keys, s_in, s_out]
  std::vector<LegivRec> all;
  if (want) {
    std::vector<size_t> ends;
    for (size_t k = 0; k < m->tiles.size() && !err && !too_many; ++k) {
      std::vector<LegivRec> part;
      err = legiv_list(m->tiles[k], parts[k], distance, speed_max, targets, want, &part);
      if (err) why = cs_last_error(m->tiles[k]);
      all.insert(all.end(), part.begin(), part.end());
      ends.push_back(all.size());
    }
    mesh_merge_runs(all, ends);
    if (all.size() > want) all.resize(want);
    if (m->distributed) {
      const size_t rows = (err || too_many) ? 0u : all.size();
      std::vector<uint64_t> mine(1u + 3u * rows, err ? 1u : 0u);
      for (size_t i = 0; i < rows; ++i) {
        mine[1u + i] = all[i].key;
        std::memcpy(&mine[1u + rows + i], &all[i].s_in, sizeof(double));
        std::memcpy(&mine[1u + 2u * rows + i], &all[i].s_out, sizeof(double));
      }
      std::vector<std::vector<unsigned char>> got;
      if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), got)) {
        m->poison(rc, m->error);
        return SIZE_MAX;
      }
      all.clear();
      ends.clear();
      for (const auto& p : got) {
        const size_t words = p.size() / sizeof(uint64_t);
        std::vector<uint64_t> w(words);
        if (words) std::memcpy(w.data(), p.data(), words * sizeof(uint64_t));
        if (!words || w[0] != 0u || (words - 1u) % 3u) {
          if (!err) {
            err = 90;
            why = other_failed;
          }
          continue;
        }
        const size_t rows_p = (words - 1u) / 3u;
        for (size_t i = 0; i < rows_p; ++i) {
          LegivRec r;
          r.key = w[1u + i];
          std::memcpy(&r.s_in, &w[1u + rows_p + i], sizeof(double));
          std::memcpy(&r.s_out, &w[1u + 2u * rows_p + i], sizeof(double));
          all.push_back(r);
        }
        ends.push_back(all.size());
      }
      mesh_merge_runs(all, ends);
      if (all.size() > want) all.resize(want);
    }
  }
  if (err) {
    m->error = why;
    return SIZE_MAX;
  }
  if (too_many) {
    legiv_too_many(&m->error);
    return SIZE_MAX;
  }
  if (out_counts) std::copy(counts.begin(), counts.end(), out_counts);
  if (want && !m->tiles.empty()) legiv_copy_out(m->tiles[0], all, out, cap);
  return (size_t)total;
}

}  // extern "C"
