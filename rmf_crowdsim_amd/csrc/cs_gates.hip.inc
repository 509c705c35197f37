// cs_gates.hip.inc — lines that are crossed: for each GATE (a segment A -> B with a time window) every agent that walks
// through it within the window if it keeps the velocity it has now, from which side, when and where along the segment
// (include/crowdstep_state.h, "Who crosses a line").  Part of the single translation unit crowdstep_hip.hip (included
// there, after cs_leg_intervals.hip.inc; it uses ray_slab, rays_uniform, RAYS_NOBODY and RAYS_FAR_CELLS of
// cs_rays.hip.inc, pairs_args, pairs_in_grid, near_roles, pairs_wave_sum, pairs_header, pairs_read_count,
// pairs_read_header, pairs_radix, pairs_bits and PairsScratch of cs_near.hip.inc, k_encounters_gather of
// cs_encounters.hip.inc, sel_begin / sel_check / sel_up of cs_select.hip.inc and mesh_host_gatherv / mesh_merge_runs of
// cs_mesh.hip.inc, and changes none of them: the walk below is legiv_walk's, restated for a probe without a distance and
// without an `ignore`, so that no existing device function is compiled from other text than before).
//
//   K_count  k_gate_count, one 64-lane wave per gate, four gates per workgroup.  Everything the walk decides is computed
//            from the gate alone, so it is the same in all the lanes of a wave.  The wave walks the rows of cells that
//            meet the segment grown by the gate's reach and the spare cell; in a row the cells that matter are one
//            interval of columns, hence one run of slots of the cell-sorted arrays, taken 64 slots at a time.  A lane
//            rebuilds its candidate's position with near_walk's expression (the position cs_read_agents reports), widens
//            its f32 velocity, applies the rule (gate_rule) and tests every candidate the rule passes as a participant
//            and against the filter.  The wave's two sums go into counts[2 * gate] (dir +1) and counts[2 * gate + 1]
//            (dir -1) and, with one atomic, into the 64-bit total.
//   K_emit   k_gate_emit, only when listing: the same walk.  The rows of gate k go to list places offsets[k] ..
//            offsets[k + 1], the exclusive sums of the counts of both directions (made on the host, which has the counts
//            by then); the rows of one 64-slot step take consecutive places by a ballot.  A row is (gate << 32 | device
//            id, its place, s, u).  s is +0.0 or positive, so its sign bit is free: it carries dir (set: dir -1) through
//            the sort and the mesh and is taken out again on the host.
//   sort     pairs_radix over the id half (the bits of the largest id listed) and the gate half (the bits of n - 1) of
//            the key with the place as the payload; k_encounters_gather (two f64 columns by the sorted places) then brings
//            s and u of the first `want` rows into sorted order.
//   mesh     every tile runs ALL gates against the agents it owns (the walk is clipped to the owned cells, the gates stay
//            in world coordinates).  Agents are disjoint across tiles, so counts add and the rows of all tiles, merged by
//            their key, are the single engine's.  One gather for the counts, one for the rows.
//
// One wave per gate, not the item cut of cs_zones.hip.inc: a gate's capsule holds its length times twice its reach of
// crowd (a 100 m lane with a reach of 6 m in a crowd of 2.5 agents per square metre: some 3,000 slots, 50 steps of a wave),
// where a zone may hold the whole crowd.  tools/gate_crossings_bench.py times door-sized and 100 m gates against the host
// path; should long gates with a large reach leave waves idle, the item cut is the known remedy (DESIGN.md section 8).
//
// WHY A BOUNDED SEARCH IS SOUND.  Write e = (ex, ey) for B - A as the rule rounds it; the rule knows the gate only as A
// and e.  A crossing of the rule on participant q means, in exact arithmetic, that at time t0 + s, with 0 <= s < T =
// t1 - t0, the agent, at x_q + v_q * (t0 + s), is at the point E = A + u * e of the segment, 0 <= u < 1.  q is considered
// only if |v_q| < speed_max, and t0 + s < t1, so it has moved less than speed_max * t1 from where it stands NOW: its
// present position, the one the cell index knows, lies within  G = speed_max * t1  of the point E of the segment
// A + e * [0, 1].  Agents that are faster are left out by the rule itself, not by the walk.
//
// WHY THE WALK IS CONSERVATIVE.  It is the capsule walk of cs_legs.hip.inc (see there) with the probe going from A to
// A + e over the parameter 0 .. 1 and distance = 0: grow = G + cs from THIS gate's t1, the segment clipped in f64 to the
// part [sa, sb] of [0, 1] inside the (owned) grid's rectangle grown by grow, row xr visited for the part of [sa, sb] the
// probe spends in the row's slab grown by grow, its columns those whose slab meets the y range of that part; rows and
// columns are clamped as f64 values and only then converted; no early exit.  A participant's offset lies in [0, cs] of
// its cell up to one rounding, so E lies in that cell's rectangle grown by G, and the walk grows by a WHOLE cell more.
// A start, an extent |ex|, |ey| or a reach at or beyond 2^32 cells (where roundings are no longer small against a cell,
// and where +inf would meet 0 in a product: speed_max = +inf) takes no clip at all: the wave visits every (owned) cell.
// A gate with A == B crosses nobody by the rule (cv == 0) and visits nothing.
//
// WHERE ROUNDING DECIDES.  px, py, rx, ry carry half an ulp of the coordinates they combine, c0 and cu one more relative
// 2^-52 of |e||r| and |r||v|, so s and u place the crossing off by about 2^-51 |r| / sin(angle between e and v_q) metres.
// With coordinates within 2^32 cells that is below the spare cell unless the walker moves parallel to the gate to within
// 2^-18 radians; and it is NOTHING wherever the products are exact (axis-aligned gates, small dyadic coordinates).  Only
// for a walker whose cv is itself rounding noise (parallel to an oblique gate to some fifty bits AND collinear with it
// likewise) can the rule name a crossing that no geometry backs, and such a candidate is listed when it stands within the
// reach and not when it stands beyond it.
//
// Scratch through PairsScratch: for the count the gates (48 bytes each) and the counts (16 bytes each); for a listing the
// gates, the offsets and six 8-byte arrays of one entry per row, with the histogram of the sort.

static_assert(sizeof(cs_gate) == 48 && sizeof(cs_gate_crossing) == 32, "gates and crossings travel as they are declared");

// The rule for one gate and the candidate at (xq, yq) with velocity (vxq, vyq): one f64 operation per operation of the
// header, rounded once each.  (ex, ey) = B - A, S2 = speed_max * speed_max, T = t1 - t0.  *neg: dir is -1.
__device__ __forceinline__ bool gate_rule(const cs_gate& gt, double ex, double ey, double S2, double T, double xq, double yq,
                                          double vxq, double vyq, double* s_out, double* u_out, bool* neg) {
  const double ss = vxq * vxq + vyq * vyq;
  if (!(ss < S2)) return false;
  const double px = xq + vxq * gt.t0, py = yq + vyq * gt.t0;
  const double rx = px - gt.ax, ry = py - gt.ay;
  const double c0 = ex * ry - ey * rx;
  const double cv = ex * vyq - ey * vxq;
  const double cu = rx * vyq - ry * vxq;
  if (!((cv > 0.0 && c0 <= 0.0) || (cv < 0.0 && c0 >= 0.0))) return false;
  double s = (-c0) / cv;
  if (!(s > 0.0)) s = 0.0;
  const double u = cu / cv;
  if (!(s < T && u >= 0.0 && u < 1.0)) return false;
  *s_out = s;
  *u_out = u;
  *neg = !(cv > 0.0);
  return true;
}

// The walk of the wave of gate gt over its capsule.  Every lane of the wave calls v.row(is_row, id, neg, s, u) once per
// 64 slots of a run, all lanes together: is_row says whether the lane's slot is a row of this gate.
template <class V>
__device__ __forceinline__ void gate_walk(const GridDev& g, const AgentArrays& a, uint32_t limit,
                                          const uint32_t* __restrict__ cell_start, const SelGroupDev* __restrict__ groups,
                                          const PairsArgs& P, double speed_max, const cs_gate& gt, uint32_t lane, V& v) {
  const double cs = P.cell_size, S2 = speed_max * speed_max, T = gt.t1 - gt.t0;
  const double ex = gt.bx - gt.ax, ey = gt.by - gt.ay;
  const double grow = speed_max * gt.t1 + cs;  // this gate's reach and the spare cell
  // the (owned) grid: rows are x, g.ny of them; columns are y, g.nx of them
  const uint32_t lo_x = P.owned_only ? g.own_x0 : 0u, hi_x = P.owned_only ? g.own_x1 : g.ny;
  const uint32_t lo_y = P.owned_only ? g.own_y0 : 0u, hi_y = P.owned_only ? g.own_y1 : g.nx;
  // (s >= 0 is never below T == 0; A == B has cv == 0 for everyone)
  bool any = lo_x < hi_x && lo_y < hi_y && limit != 0u && T > 0.0 && (ex != 0.0 || ey != 0.0);
  // A in metres from the low corner of local cell (0, 0)
  const double qx = gt.ax - (P.off_x + (double)g.org_x * cs), qy = gt.ay - (P.off_y + (double)g.org_y * cs);
  const double far = RAYS_FAR_CELLS * cs;
  const bool full = !(fabs(qx) < far && fabs(qy) < far && fabs(ex) < far && fabs(ey) < far && grow < far);
  double sa = 0.0, sb = 1.0;
  double rlo = (double)lo_x, rhi = (double)hi_x - 1.0;
  if (any && !full) {
    any = ray_slab(qx, ex, (double)lo_x * cs - grow, (double)hi_x * cs + grow, &sa, &sb) &&
          ray_slab(qy, ey, (double)lo_y * cs - grow, (double)hi_y * cs + grow, &sa, &sb);
    if (any) {
      const double xa = qx + ex * sa, xb = qx + ex * sb;
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
      if (ex != 0.0) {
        const double t1 = (((double)xr * cs - grow) - qx) / ex, t2 = ((((double)xr + 1.0) * cs + grow) - qx) / ex;
        s0 = fmax(sa, fmin(t1, t2));
        s1 = fmin(sb, fmax(t1, t2));
      }
      row = s0 <= s1;
      if (row) {
        const double ya = qy + ey * s0, yb = qy + ey * s1;
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
        bool is_row = false, neg = false;
        uint32_t idj = RAYS_NOBODY;
        double s = 0.0, u = 0.0;
        if (j < e) {
          idj = a.id[j];
          const uint32_t cyj = a.cell[j] - rowbase;
          if (cyj <= c1) {  // (a slot that is not of this row's run cannot happen in sorted arrays)
            const float2 off = a.off[j], vel = a.vel[j];
            const double xq = P.off_x + (bx + (double)off.x);
            const double yq = P.off_y + ((double)((uint64_t)g.org_y + cyj) * cs + (double)off.y);
            is_row = gate_rule(gt, ex, ey, S2, T, xq, yq, (double)vel.x, (double)vel.y, &s, &u, &neg) &&
                     pairs_in_grid(P, xq, yq) && (near_roles(g, a, j, groups, P, xq, yq, 3u) & 1u);  // (role A: the filter)
          }
        }
        v.row(is_row, idj, neg, s, u);
      }
    }
    if (xr == r1) break;  // (r1 may be the last row a uint32_t can name)
  }
}

struct GateCount {
  uint32_t pos, neg;
  __device__ __forceinline__ void row(bool is_row, uint32_t, bool is_neg, double, double) {
    pos += (is_row && !is_neg) ? 1u : 0u;
    neg += (is_row && is_neg) ? 1u : 0u;
  }
};

// The rows of a 64-slot step take the places at, at + 1, ... in lane order; `at` is the same in every lane.  Nothing is
// written at or beyond `end`, the first place of the next gate.
struct GateEmit {
  unsigned long long at, end, gate_bits;
  unsigned long long* __restrict__ keys;
  double* __restrict__ index;
  double* __restrict__ ss;
  double* __restrict__ us;
  uint32_t lane, top;
  __device__ __forceinline__ void row(bool is_row, uint32_t id, bool is_neg, double s, double u) {
    const unsigned long long m = __ballot(is_row);
    if (is_row) {
      const unsigned long long k = at + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
      if (k < end) {
        keys[k] = gate_bits | id;
        index[k] = __longlong_as_double((long long)k);
        // (s is +0.0 or positive: its sign bit carries dir)
        ss[k] = __longlong_as_double(__double_as_longlong(s) | (is_neg ? (long long)0x8000000000000000ull : 0ll));
        us[k] = u;
      }
      top = max(top, id);
    }
    at += (unsigned long long)__popcll(m);
  }
};

// K_count.  counts[2k], counts[2k + 1] = the rows of gate k with dir +1, -1; hdr[0] += them (starts at 0).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_gate_count(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                 const SelGroupDev* __restrict__ groups, PairsArgs P, double speed_max, const cs_gate* __restrict__ gates,
                 uint32_t n_gates, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ hdr) {
  const uint32_t k = rays_uniform(blockIdx.x * PAIRS_WAVES + (threadIdx.x >> 6));
  if (k >= n_gates) return;  // (the whole wave)
  const uint32_t lane = __lane_id();
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);  // the sorted arrays hold the live agents in front
  const cs_gate gt = gates[k];
  GateCount v{0u, 0u};
  gate_walk(g, a, limit, cell_start, groups, P, speed_max, gt, lane, v);
  const unsigned long long wp = pairs_wave_sum(v.pos), wn = pairs_wave_sum(v.neg);
  if (lane == 0u) {
    counts[2u * (size_t)k] = wp;
    counts[2u * (size_t)k + 1u] = wn;
    if (wp + wn) atomicAdd(&hdr[0], wp + wn);
  }
}

// K_emit.  offsets[k]: the list place of the first row of gate k (n_gates + 1 entries).  hdr[1] += the rows written
// (starts at 0), the low word of hdr[2]: the largest id listed.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_gate_emit(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                const SelGroupDev* __restrict__ groups, PairsArgs P, double speed_max, const cs_gate* __restrict__ gates,
                uint32_t n_gates, const unsigned long long* __restrict__ offsets, unsigned long long* __restrict__ hdr,
                unsigned long long* __restrict__ keys, double* __restrict__ index, double* __restrict__ ss,
                double* __restrict__ us) {
  const uint32_t k = rays_uniform(blockIdx.x * PAIRS_WAVES + (threadIdx.x >> 6));
  if (k >= n_gates) return;  // (the whole wave)
  const unsigned long long at = offsets[k], end = offsets[k + 1u];
  if (at >= end) return;  // (no rows: the same in all the lanes)
  const uint32_t lane = __lane_id();
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);
  const cs_gate gt = gates[k];
  GateEmit v{at, end, (unsigned long long)k << 32, keys, index, ss, us, lane, 0u};
  gate_walk(g, a, limit, cell_start, groups, P, speed_max, gt, lane, v);
  uint32_t top = v.top;
  for (int d = 32; d >= 1; d >>= 1) top = max(top, (uint32_t)__shfl_xor(top, d, 64));
  if (lane == 0u) {
    atomicAdd(&hdr[1], min(v.at, end) - at);
    if (top) atomicMax(reinterpret_cast<uint32_t*>(&hdr[2]), top);
  }
}

namespace {

// one listed crossing on the host: the key (gate << 32 | DEVICE id), s with dir in its sign bit (set: -1), and u
struct GateRec {
  uint64_t key;
  double s_dir, u;
};
bool operator<(const GateRec& l, const GateRec& r) { return l.key < r.key; }

// what one engine counted: the rows of each gate and direction (2n entries) and of all
struct GatePart {
  std::vector<uint64_t> counts;
  uint64_t total = 0;
};

// the refusals of the header (3); the text names the first bad gate
int gates_check(std::string* error, const cs_gate* gates, size_t n, double speed_max, const cs_selection* filter) {
  const std::string call = "gate_crossings";
  if (n > CS_GATES_MAX) {
    *error = call + ": more gates than CS_GATES_MAX = 1048576 in one call";
    return 3;
  }
  if (n && !gates) {
    *error = call + ": null gates";
    return 3;
  }
  if (!(speed_max >= 0.0)) {
    *error = call + ": speed_max is NaN or negative";
    return 3;
  }
  if (filter)
    if (int rc = sel_check(error, filter, call.c_str())) return rc;
  for (size_t k = 0; k < n; ++k) {
    const cs_gate& gt = gates[k];
    const char* what = nullptr;
    if (!(std::isfinite(gt.ax) && std::isfinite(gt.ay) && std::isfinite(gt.bx) && std::isfinite(gt.by)))
      what = "its ends are not finite";
    else if (!(std::isfinite(gt.t0) && std::isfinite(gt.t1))) what = "its times are not finite";
    else if (gt.t0 < 0.0) what = "its t0 is negative";
    else if (gt.t1 < gt.t0) what = "its t1 is before its t0";
    if (what) {
      *error = call + ": gate " + std::to_string(k) + ": " + what;
      return 3;
    }
  }
  return 0;
}

// All n gates (n > 0) against the agents one engine holds (after sel_begin), counted: part->total, and with want_counts
// part->counts.  One memset, one upload, one kernel, one read back (and one download of the counts): no row is made.
int gates_count(cs_engine* e, const cs_gate* gates, size_t n, double speed_max, const cs_selection* filter,
                bool want_counts, GatePart* part) {
  part->counts.assign(2u * n, 0u);
  part->total = 0;
  if (int rc = e->refresh_counts()) return rc;
  if (int rc = e->ensure_index()) return rc;
  if (!e->n_slots) return 0;
  const PairsArgs P = pairs_args(e, 0.0, filter, nullptr);
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  PairsScratch sc(e);
  const size_t b_gates = sel_up(n * sizeof(cs_gate));
  unsigned char* p = static_cast<unsigned char*>(sc.get(b_gates + 2u * n * sizeof(uint64_t)));
  if (!p) return 90;
  cs_gate* d_gates = reinterpret_cast<cs_gate*>(p);
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(p + b_gates);
  HIP_OK_E(e, hipMemcpyAsync(d_gates, gates, n * sizeof(cs_gate), hipMemcpyHostToDevice, e->stream));
  const uint32_t blocks = ((uint32_t)n + PAIRS_WAVES - 1u) / PAIRS_WAVES;
  hipLaunchKernelGGL(k_gate_count, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], e->n_slots,
                     e->cell_start.get(), e->sel_groups_dev.get(), P, speed_max, d_gates, (uint32_t)n, d_counts, hdr);
  HIP_OK_E(e, hipGetLastError());
  if (want_counts)
    HIP_OK_E(e, hipMemcpyAsync(part->counts.data(), d_counts, 2u * n * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
  unsigned long long found = 0;
  if (int rc = pairs_read_count(e, hdr, &found)) return rc;  // (synchronised: the caller's gates were read)
  part->total = found;
  return 0;
}

// The first min(part.total, want) rows of what gates_count counted (with its counts; part.total at most CS_PAIRS_MAX),
// ascending by (gate, id), as device ids.  One memset, two uploads, one kernel, one read back, three launches per 4 bits
// of the largest id and of the largest gate, one gather, one download.
int gates_list(cs_engine* e, const GatePart& part, const cs_gate* gates, size_t n, double speed_max,
               const cs_selection* filter, size_t want, std::vector<GateRec>* out) {
  out->clear();
  const uint64_t found = part.total;
  if (!want || !found || !n) return 0;
  std::vector<uint64_t> offsets(n + 1u, 0u);
  for (size_t k = 0; k < n; ++k) offsets[k + 1u] = offsets[k] + part.counts[2u * k] + part.counts[2u * k + 1u];
  if (offsets[n] != found) {
    e->error = "gate_crossings: the counts of the gates do not add up to the total";
    return 90;
  }
  const PairsArgs P = pairs_args(e, 0.0, filter, nullptr);
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  PairsScratch sc(e);
  const size_t b_gates = sel_up(n * sizeof(cs_gate)), b_off = sel_up((n + 1u) * sizeof(uint64_t));
  const size_t b = sel_up((size_t)found * sizeof(uint64_t));
  const size_t tiles = ((size_t)found + IDS_TILE - 1u) / IDS_TILE;
  const size_t b_hist = sel_up(IDS_RADIX * std::max<size_t>(tiles, 1u) * sizeof(uint32_t));
  unsigned char* p = static_cast<unsigned char*>(sc.get(b_gates + b_off + 6u * b + b_hist + 256u));
  if (!p) return 90;
  cs_gate* d_gates = reinterpret_cast<cs_gate*>(p);
  unsigned long long* d_off = reinterpret_cast<unsigned long long*>(p + b_gates);
  unsigned char* q = p + b_gates + b_off;
  unsigned long long *keys = reinterpret_cast<unsigned long long*>(q), *keys_other = reinterpret_cast<unsigned long long*>(q + b);
  double *index = reinterpret_cast<double*>(q + 2u * b), *index_other = reinterpret_cast<double*>(q + 3u * b);
  double *ss = reinterpret_cast<double*>(q + 4u * b), *us = reinterpret_cast<double*>(q + 5u * b);
  uint32_t* hist = reinterpret_cast<uint32_t*>(q + 6u * b);
  HIP_OK_E(e, hipMemcpyAsync(d_gates, gates, n * sizeof(cs_gate), hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(d_off, offsets.data(), (n + 1u) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
  const uint32_t blocks = ((uint32_t)n + PAIRS_WAVES - 1u) / PAIRS_WAVES;
  hipLaunchKernelGGL(k_gate_emit, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], e->n_slots,
                     e->cell_start.get(), e->sel_groups_dev.get(), P, speed_max, d_gates, (uint32_t)n, d_off, hdr, keys, index, ss, us);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long back[3];
  if (int rc = pairs_read_header(e, hdr, back)) return rc;  // (synchronised: the host staging may go)
  if (back[1] != found) {
    e->error = "gate_crossings: the listing found another number of crossings than the count";
    return 90;
  }
  const uint32_t rows = (uint32_t)found;  // (at most CS_PAIRS_MAX)
  if (rows > 1u) {  // the id in the low half, the gate in the high half
    if (int rc = pairs_radix(e, &keys, &keys_other, &index, &index_other, hist, rows, 0u, pairs_bits((uint32_t)back[2])))
      return rc;
    if (n > 1u)
      if (int rc = pairs_radix(e, &keys, &keys_other, &index, &index_other, hist, rows, 32u, pairs_bits((uint32_t)(n - 1u))))
        return rc;
  }
  const uint32_t take = (uint32_t)std::min<size_t>(want, rows);
  double* s_sorted = reinterpret_cast<double*>(keys_other);
  double* u_sorted = index_other;
  std::vector<uint64_t> k_host(take);
  std::vector<double> s_host(take), u_host(take);
  hipLaunchKernelGGL(k_encounters_gather, dim3((take + PAIRS_BLOCK - 1u) / PAIRS_BLOCK), dim3(PAIRS_BLOCK), 0, e->stream,
                     index, ss, us, take, rows, s_sorted, u_sorted);
  HIP_OK_E(e, hipGetLastError());
  HIP_OK_E(e, hipMemcpyAsync(k_host.data(), keys, take * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(s_host.data(), s_sorted, take * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(u_host.data(), u_sorted, take * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  out->resize(take);
  for (size_t k = 0; k < take; ++k) (*out)[k] = GateRec{k_host[k], s_host[k], u_host[k]};
  return 0;
}

int gates_too_many(std::string* error) {
  *error = "gate_crossings: too many crossings to list (more than CS_PAIRS_MAX = 67108864); the count-only form has no limit";
  return 3;
}

// device ids -> external ids and the sign bit of s -> dir, into the caller's rows
void gates_copy_out(const cs_engine* ids_of, const std::vector<GateRec>& list, cs_gate_crossing* out, size_t cap) {
  const size_t k = std::min(list.size(), cap);
  for (size_t i = 0; i < k; ++i) {
    out[i].gate = (uint32_t)(list[i].key >> 32);
    out[i].dir = std::signbit(list[i].s_dir) ? -1 : 1;
    out[i].id = ids_of->ext_id(list[i].key & 0xFFFFFFFFull);
    out[i].s = std::fabs(list[i].s_dir);
    out[i].u = list[i].u;
  }
}

}  // namespace

extern "C" {

size_t cs_gate_crossings(cs_engine* e, const cs_gate* gates, size_t n, double speed_max, const cs_selection* filter,
                         uint64_t* out_counts, cs_gate_crossing* out, size_t cap) {
  if (!e) return SIZE_MAX;
  hipSetDevice(e->device);
  if (gates_check(&e->error, gates, n, speed_max, filter)) return SIZE_MAX;
  if (sel_begin(e)) return SIZE_MAX;
  if (!n) return 0;
  const size_t want = out ? cap : 0u;
  GatePart part;
  if (gates_count(e, gates, n, speed_max, filter, want || out_counts, &part)) return SIZE_MAX;
  if (want && part.total > CS_PAIRS_MAX) {
    gates_too_many(&e->error);
    return SIZE_MAX;
  }
  std::vector<GateRec> list;
  if (gates_list(e, part, gates, n, speed_max, filter, want, &list)) return SIZE_MAX;
  if (out_counts) std::copy(part.counts.begin(), part.counts.end(), out_counts);
  if (want) gates_copy_out(e, list, out, cap);
  return (size_t)part.total;
}

// Collective: one gather of variable size (two collectives) for the counts and, when listing, one more for the rows,
// whatever the crowd and the answer: a rank that failed, or a listing that is refused, sends its word alone.  n == 0
// makes none: every rank passes the same n.  No halo exchange, no band: a tile's walk is clipped to the cells it owns and
// every agent is owned by one tile.
size_t cs_mesh_gate_crossings(cs_mesh* m, const cs_gate* gates, size_t n, double speed_max, const cs_selection* filter,
                              uint64_t* out_counts, cs_gate_crossing* out, size_t cap) {
  if (!m) return SIZE_MAX;
  if (m->dead()) return SIZE_MAX;
  if (gates_check(&m->error, gates, n, speed_max, filter)) return SIZE_MAX;
  if (cs_mesh_synchronize(m)) return SIZE_MAX;
  hipSetDevice(m->device);
  if (!n) return 0;
  const size_t want = out ? cap : 0u;
  const char* const other_failed = "a tile of another rank failed while listing gate crossings";
  int err = 0;
  std::string why;
  // 1. every tile counts; the counts of all tiles of all ranks: [0 ok / 1 failed, 2n counts]
  std::vector<GatePart> parts(m->tiles.size());
  std::vector<uint64_t> counts(2u * n, 0u);
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    cs_engine* e = m->tiles[k];
    if (!err) err = sel_begin(e);
    if (!err) err = gates_count(e, gates, n, speed_max, filter, true, &parts[k]);
    if (err && why.empty()) why = cs_last_error(e);
    if (!err)
      for (size_t i = 0; i < 2u * n; ++i) counts[i] += parts[k].counts[i];
  }
  if (m->distributed) {
    std::vector<uint64_t> mine(1u + (err ? 0u : 2u * n), err ? 1u : 0u);
    if (!err) std::copy(counts.begin(), counts.end(), mine.begin() + 1);
    std::vector<std::vector<unsigned char>> got;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(uint64_t), got)) {
      m->poison(rc, m->error);
      return SIZE_MAX;
    }
    counts.assign(2u * n, 0u);
    std::vector<uint64_t> w(1u + 2u * n);
    for (const auto& p : got) {
      if (p.size() != w.size() * sizeof(uint64_t)) {  // (a rank that failed sends its word alone)
        if (!err) {
          err = 90;
          why = other_failed;
        }
        continue;
      }
      std::memcpy(w.data(), p.data(), p.size());
      for (size_t i = 0; i < 2u * n; ++i) counts[i] += w[1u + i];
    }
  }
  uint64_t total = 0;
  for (uint64_t c : counts) total += c;
  const bool too_many = want && total > CS_PAIRS_MAX;
  // 2. when listing: the rows of every tile, merged; then those of every rank: [0 ok / 1 failed, keys, s with dir, u]
  std::vector<GateRec> all;
  if (want) {
    std::vector<size_t> ends;
    for (size_t k = 0; k < m->tiles.size() && !err && !too_many; ++k) {
      std::vector<GateRec> part;
      err = gates_list(m->tiles[k], parts[k], gates, n, speed_max, filter, want, &part);
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
        std::memcpy(&mine[1u + rows + i], &all[i].s_dir, sizeof(double));
        std::memcpy(&mine[1u + 2u * rows + i], &all[i].u, sizeof(double));
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
          GateRec r;
          r.key = w[1u + i];
          std::memcpy(&r.s_dir, &w[1u + rows_p + i], sizeof(double));
          std::memcpy(&r.u, &w[1u + 2u * rows_p + i], sizeof(double));
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
    gates_too_many(&m->error);
    return SIZE_MAX;
  }
  if (out_counts) std::copy(counts.begin(), counts.end(), out_counts);
  if (want && !m->tiles.empty()) gates_copy_out(m->tiles[0], all, out, cap);
  return (size_t)total;
}

}  // extern "C"
