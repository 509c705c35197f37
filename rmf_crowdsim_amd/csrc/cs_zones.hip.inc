// cs_zones.hip.inc — the agents inside polygon zones between steps: for each zone its number of agents and, when asked,
// the list of them (include/crowdstep_state.h, "Agents in polygon zones").  Part of the single translation unit
// crowdstep_hip.hip (included there, after cs_leg_intervals.hip.inc; it uses rays_uniform of cs_rays.hip.inc, pairs_args,
// pairs_in_grid, near_roles, pairs_header, pairs_read_count, pairs_read_header, pairs_radix, pairs_bits and PairsScratch
// of cs_near.hip.inc, sel_begin / sel_check / sel_up of cs_select.hip.inc and mesh_host_gatherv / mesh_merge_runs of
// cs_mesh.hip.inc, and changes none of them).
//
//   plan     on the host, per engine (zone_plan): the box of every zone, the exact minimum and maximum of its vertices, and
//            from it the rows and columns of cells the zone can hold agents in (below).  An ITEM is one zone, a group of
//            R consecutive rows of its range (R == 1 unless the zones cover more than 2^22 rows together) and one of
//            `split` shares of the slots of those rows.  A zone whose range misses the (owned) grid makes no item.  The
//            items of zone k are item0[k] .. item0[k + 1]; a wave finds its zone by a binary search in that table.
//   K_count  k_zone_count, one 64-lane wave per item, four items per workgroup.  The cells (row, c0 .. c1) of one row are
//            ONE run of slots of the cell-sorted arrays, cell_start[row * nx + c0] .. cell_start[row * nx + c1 + 1]; the
//            wave of share s takes the 64 slots from b + 64 * s on, then those 64 * split further on, and so on.  A lane
//            rebuilds its slot's position with sel_load's expression and tests the box; only if some lane of the wave is in
//            the box does the wave go round the ring.  The edges are the same for every lane: the vertices are read
//            through wave-uniform addresses (the zone's index comes from readfirstlane), so one read serves 64 agents.
//            Who is inside the ring is tested as a participant and against the filter last (near_roles: meta, group
//            table, velocity).  The tally is popcount(ballot) per 64 slots; the wave leaves with one atomic into
//            counts[zone] and one into the 64-bit total.
//   K_emit   k_zone_emit, only when listing: the same walk.  The rows of zone k go to list places offsets[k] ..
//            offsets[k + 1], the exclusive sums of the counts (made on the host, which has the counts by then).  The
//            waves of a zone take their places with one atomic per 64 slots that hold a row (cursor[k]), the rows of
//            those 64 slots by the ballot.  A row is the key (zone << 32 | device id).
//   sort     pairs_radix over the id half (the bits of the largest id listed) and the zone half (the bits of n - 1) of the
//            key, no payload; the first `want` keys come back and the host maps device ids to external ids.
//   mesh     every tile runs ALL zones against the agents it owns (the cell ranges are clipped to the owned cells, the
//            zones stay in world coordinates).  Agents are disjoint across tiles, so counts add and the rows of all tiles,
//            merged by their key, are the single engine's.  One gather for the counts, one for the rows.
//
// WHY THE CELL RANGE IS EXACT.  The box is part of the rule: an agent outside the box of a zone is not in it, whatever the
// ring says.  So it is enough to visit every participant whose reported position lies in the box.  A participant indexed
// under global row r reports x = off_x + (r * cs + off) with the stored offset `off` in [0, cs] up to one rounding (an f32
// offset can round up to cs itself; cs_near.hip.inc says who the others are, and none of them takes part).  Hence
// r <= (x - off_x) / cs <= r + 1 up to a few units of 2^-53 relative, far less than one cell for every grid of at most
// 2^31 cells.  With bx0 <= x <= bx1 this gives floor((bx0 - off_x) / cs) - 1 <= r <= floor((bx1 - off_x) / cs) + 1 whether
// or not the two quotients were rounded across an integer: both ends are widened by one cell, and the widened range is
// clipped to the (owned) grid.  The same holds for the columns and y.  Everything the widened range adds is judged by the
// rule itself, so it changes no answer.
//
// Scratch through PairsScratch: for the count the zone records (64 bytes each), the item table, the vertices and the
// counts; for a listing also the offsets, the cursors, two 8-byte arrays of one entry per row and the histogram of the sort.

static_assert(sizeof(cs_zone) == 16 && sizeof(cs_zone_agent) == 16, "zones and their rows travel as they are declared");

#define ZONE_WAVE_SLOTS 1024u  // the slots a wave is meant to handle: the shares of an item are cut for it
#define ZONE_SPLIT_MAX 256u    // shares of one group of rows
#define ZONE_ITEMS_ROWS ((uint64_t)1u << 22)  // above this many rows in all, an item takes several rows

// one zone as the device sees it
struct ZoneDev {
  double bx0, bx1, by0, by1;  // the box
  unsigned long long first;   // its first vertex
  uint32_t count;             // its vertices
  uint32_t r0, rows;          // the local rows r0 .. r0 + rows - 1 (rows == 0: none)
  uint32_t c0, c1;            // the local columns c0 .. c1
  uint32_t split;             // shares of a group of rows
};
static_assert(sizeof(ZoneDev) == 64, "zone records are uploaded as they are declared");

// Does the edge from (ax, ay) to (bx, by) cross for the agent at (x, y): the rule of the header, one f64 operation per
// operation there.  (lx, ly) is the end with the smaller y, whichever way the edge is given.
__device__ __forceinline__ bool zone_cross(double ax, double ay, double bx, double by, double x, double y) {
  const bool up = ay <= by;
  const double lx = up ? ax : bx, ly = up ? ay : by, hx = up ? bx : ax, hy = up ? by : ay;
  if (!(ly <= y && y < hy)) return false;  // (ly == hy never straddles)
  const double ex = hx - lx, ey = hy - ly, px = x - lx, py = y - ly;
  const double c = ex * py - ey * px;
  return c > 0.0;
}

// The walk of the wave of share s over the rows [ra, rb) of zone z.  Every lane of the wave calls v.row(is_row, j) once
// per 64 slots, all lanes together: is_row says whether the lane's slot j is a row of this zone.
template <class V>
__device__ __forceinline__ void zone_walk(const GridDev& g, const AgentArrays& a, uint32_t limit,
                                          const uint32_t* __restrict__ cell_start, const SelGroupDev* __restrict__ groups,
                                          const PairsArgs& P, const ZoneDev& z, const double* __restrict__ vertices,
                                          uint32_t ra, uint32_t rb, uint32_t s, uint32_t lane, V& v) {
  const double cs = P.cell_size;
  const double* __restrict__ vtx = vertices + 2u * z.first;
  for (uint32_t xr = ra; xr < rb; ++xr) {
    const uint32_t rowbase = xr * g.nx;  // (below ncells, which fits 32 bits)
    const double bx = (double)((uint64_t)g.org_x + (uint64_t)xr) * cs;
    const uint32_t b = rays_uniform(cell_start[rowbase + z.c0]);
    const uint32_t e = rays_uniform(min(cell_start[rowbase + z.c1 + 1u], limit));  // (index <= ncells: the table has ncells + 1)
    for (uint32_t j0 = b + 64u * s; j0 < e; j0 += 64u * z.split) {  // (e <= limit < 2^31, split <= ZONE_SPLIT_MAX)
      const uint32_t j = j0 + lane;
      bool in = false;
      double xq = 0.0, yq = 0.0;
      if (j < e) {
        const uint32_t cyj = a.cell[j] - rowbase;
        if (cyj <= z.c1) {  // (a slot that is not of this row's run cannot happen in sorted arrays)
          const float2 off = a.off[j];
          xq = P.off_x + (bx + (double)off.x);
          yq = P.off_y + ((double)((uint64_t)g.org_y + cyj) * cs + (double)off.y);
          in = z.bx0 <= xq && xq <= z.bx1 && z.by0 <= yq && yq <= z.by1;
        }
      }
      if (__ballot(in)) {  // (the same in every lane)
        uint32_t odd = 0u;
        double ax = vtx[2u * (z.count - 1u)], ay = vtx[2u * (z.count - 1u) + 1u];  // the closing edge first
        for (uint32_t i = 0; i < z.count; ++i) {
          const double ex = vtx[2u * i], ey = vtx[2u * i + 1u];
          odd ^= (in && zone_cross(ax, ay, ex, ey, xq, yq)) ? 1u : 0u;
          ax = ex;
          ay = ey;
        }
        in = in && odd != 0u;
        if (in) in = pairs_in_grid(P, xq, yq) && (near_roles(g, a, j, groups, P, xq, yq, 3u) & 1u);  // (role A: the filter)
      }
      v.row(in, j);
    }
  }
}

// Which item is wave w: its zone (the k with item0[k] <= w < item0[k + 1]; item0[0] == 0 and w < item0[n_zones]), its
// rows [*ra, *rb) and its share.  The same in every lane.
__device__ __forceinline__ uint32_t zone_item(const uint32_t* __restrict__ item0, const ZoneDev* __restrict__ zones,
                                              uint32_t n_zones, uint32_t group_rows, uint32_t w, ZoneDev* z, uint32_t* ra,
                                              uint32_t* rb, uint32_t* s) {
  uint32_t lo = 0u, hi = n_zones;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (item0[mid] <= w) lo = mid;
    else hi = mid;
  }
  lo = rays_uniform(lo);
  *z = zones[lo];
  const uint32_t i = w - item0[lo];
  const uint32_t grp = i / z->split;
  *s = rays_uniform(i - grp * z->split);
  const uint32_t at = min(grp * group_rows, z->rows);  // (grp * group_rows < rows for every item the host cut)
  *ra = rays_uniform(z->r0 + at);
  *rb = rays_uniform(z->r0 + min(at + group_rows, z->rows));
  return lo;
}

struct ZoneCount {
  uint32_t n;
  __device__ __forceinline__ void row(bool is_row, uint32_t) { n += (uint32_t)__popcll(__ballot(is_row)); }
};

// The rows of 64 slots take consecutive places of their zone's part of the list, in lane order, from where the zone's
// cursor stood.  Nothing is written at or beyond `end`, the first place of the next zone.
struct ZoneEmit {
  unsigned long long begin, end, zone_bits;
  uint32_t* __restrict__ cursor;  // of this zone: the rows placed so far
  const uint32_t* __restrict__ ids;
  unsigned long long* __restrict__ keys;
  uint32_t lane, top, n;
  __device__ __forceinline__ void row(bool is_row, uint32_t j) {
    const unsigned long long m = __ballot(is_row);
    if (!m) return;  // (the same in every lane)
    const uint32_t cnt = (uint32_t)__popcll(m);
    uint32_t base = 0u;
    if (lane == 0u) base = atomicAdd(cursor, cnt);
    base = rays_uniform(base);
    if (is_row) {
      const uint32_t id = ids[j];
      const unsigned long long k = begin + base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
      if (k < end) keys[k] = zone_bits | id;
      top = max(top, id);
    }
    n += cnt;
  }
};

// K_count.  counts[k] += the rows of zone k (start at 0); hdr[0] += them (starts at 0).
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_zone_count(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                 const SelGroupDev* __restrict__ groups, PairsArgs P, const ZoneDev* __restrict__ zones,
                 const uint32_t* __restrict__ item0, uint32_t n_zones, uint32_t n_items, uint32_t group_rows,
                 const double* __restrict__ vertices, unsigned long long* __restrict__ counts,
                 unsigned long long* __restrict__ hdr) {
  const uint32_t w = rays_uniform(blockIdx.x * PAIRS_WAVES + (threadIdx.x >> 6));
  if (w >= n_items) return;  // (the whole wave)
  const uint32_t lane = __lane_id();
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);  // the sorted arrays hold the live agents in front
  ZoneDev z;
  uint32_t ra, rb, s;
  const uint32_t k = zone_item(item0, zones, n_zones, group_rows, w, &z, &ra, &rb, &s);
  ZoneCount v{0u};
  zone_walk(g, a, limit, cell_start, groups, P, z, vertices, ra, rb, s, lane, v);
  if (lane == 0u && v.n) {
    atomicAdd(&counts[k], (unsigned long long)v.n);
    atomicAdd(&hdr[0], (unsigned long long)v.n);
  }
}

// K_emit.  offsets[k]: the list place of the first row of zone k (n_zones + 1 entries); cursor[k] starts at 0.
// hdr[1] += the rows placed (starts at 0), the low word of hdr[2]: the largest id listed.
__global__ void __launch_bounds__(PAIRS_BLOCK)
    k_zone_emit(GridDev g, AgentArrays a, uint32_t n_ub, const uint32_t* __restrict__ cell_start,
                const SelGroupDev* __restrict__ groups, PairsArgs P, const ZoneDev* __restrict__ zones,
                const uint32_t* __restrict__ item0, uint32_t n_zones, uint32_t n_items, uint32_t group_rows,
                const double* __restrict__ vertices, const unsigned long long* __restrict__ offsets,
                uint32_t* __restrict__ cursor, unsigned long long* __restrict__ hdr, unsigned long long* __restrict__ keys) {
  const uint32_t w = rays_uniform(blockIdx.x * PAIRS_WAVES + (threadIdx.x >> 6));
  if (w >= n_items) return;  // (the whole wave)
  const uint32_t lane = __lane_id();
  const uint32_t limit = min(n_ub, cell_start[g.ncells]);
  ZoneDev z;
  uint32_t ra, rb, s;
  const uint32_t k = zone_item(item0, zones, n_zones, group_rows, w, &z, &ra, &rb, &s);
  const unsigned long long at = offsets[k], end = offsets[k + 1u];
  if (at >= end) return;  // (no rows: the same in all the lanes)
  ZoneEmit v{at, end, (unsigned long long)k << 32, cursor + k, a.id, keys, lane, 0u, 0u};
  zone_walk(g, a, limit, cell_start, groups, P, z, vertices, ra, rb, s, lane, v);
  uint32_t top = v.top;
  for (int d = 32; d >= 1; d >>= 1) top = max(top, (uint32_t)__shfl_xor(top, d, 64));
  if (lane == 0u && v.n) {
    atomicAdd(&hdr[1], (unsigned long long)v.n);
    if (top) atomicMax(reinterpret_cast<uint32_t*>(&hdr[2]), top);
  }
}

namespace {

// what one engine planned and counted: the zones as it uploads them, the item table, the rows of each zone and of all
struct ZonePart {
  std::vector<ZoneDev> zones;
  std::vector<uint32_t> item0;  // n + 1 entries
  uint32_t group_rows = 1;
  std::vector<uint64_t> counts;
  uint64_t total = 0;
};

// null arrays, too many zones or vertices, a bad filter, then the first bad zone (3)
int zones_check(std::string* error, const cs_zone* zones, size_t n, const double* vertices_xy, size_t n_vertices,
                const cs_selection* filter) {
  if (n && (!zones || !vertices_xy)) {
    *error = "zone_agents: null zones or vertices";
    return 3;
  }
  if (n > CS_ZONES_MAX) {
    *error = "zone_agents: more zones than CS_ZONES_MAX = 65536 in one call";
    return 3;
  }
  if (n_vertices > CS_ZONE_VERTICES_MAX) {
    *error = "zone_agents: more vertices than CS_ZONE_VERTICES_MAX = 1048576 in one call";
    return 3;
  }
  if (filter)
    if (int rc = sel_check(error, filter, "zone_agents")) return rc;
  if (!n) return 0;
  // bad[i]: the vertices before i with a coordinate that is not finite (zones may share vertices: each is judged once)
  std::vector<uint32_t> bad(n_vertices + 1u, 0u);
  for (size_t i = 0; i < n_vertices; ++i)
    bad[i + 1u] = bad[i] + ((std::isfinite(vertices_xy[2u * i]) && std::isfinite(vertices_xy[2u * i + 1u])) ? 0u : 1u);
  for (size_t k = 0; k < n; ++k) {
    const cs_zone& z = zones[k];
    const char* what = nullptr;
    if (z.count < 3u) what = "fewer than 3 vertices";
    else if (z.first > n_vertices || z.count > n_vertices - z.first) what = "its vertices run beyond n_vertices";
    else if (z.flags != 0u) what = "unknown flags";
    else if (bad[z.first + z.count] != bad[z.first]) what = "a vertex is not finite";
    if (what) {
      *error = "zone_agents: zone " + std::to_string(k) + ": " + what;
      return 3;
    }
  }
  return 0;
}

// the cells along one axis an agent reported in [b0, b1] can be indexed under: local cells *lo .. *hi of [own0, own1);
// false: none (see WHY THE CELL RANGE IS EXACT)
bool zone_cells(double b0, double b1, double off, double cs, uint32_t org, uint32_t own0, uint32_t own1, uint32_t* lo,
                uint32_t* hi) {
  if (own0 >= own1) return false;
  const double l = std::max((std::floor((b0 - off) / cs) - 1.0) - (double)org, (double)own0);
  const double h = std::min((std::floor((b1 - off) / cs) + 1.0) - (double)org, (double)own1 - 1.0);
  if (!(l <= h)) return false;
  *lo = (uint32_t)l;
  *hi = (uint32_t)h;
  return true;
}

// The plan of all n checked zones for one engine: boxes, cell ranges, shares and the item table.
void zone_plan(const cs_engine* e, const cs_zone* zones, size_t n, const double* vertices_xy, const PairsArgs& P,
               ZonePart* part) {
  const GridDev& g = e->gdev;
  const uint32_t lo_x = P.owned_only ? g.own_x0 : 0u, hi_x = P.owned_only ? g.own_x1 : g.ny;
  const uint32_t lo_y = P.owned_only ? g.own_y0 : 0u, hi_y = P.owned_only ? g.own_y1 : g.nx;
  const double cells = std::max((double)(hi_x - lo_x) * (double)(hi_y - lo_y), 1.0);
  part->zones.assign(n, ZoneDev{});
  part->item0.assign(n + 1u, 0u);
  uint64_t rows_all = 0;
  for (size_t k = 0; k < n; ++k) {
    ZoneDev& z = part->zones[k];
    const double* v = vertices_xy + 2u * zones[k].first;
    z.bx0 = z.bx1 = v[0];
    z.by0 = z.by1 = v[1];
    for (uint32_t i = 1; i < zones[k].count; ++i) {
      z.bx0 = std::min(z.bx0, v[2u * i]);
      z.bx1 = std::max(z.bx1, v[2u * i]);
      z.by0 = std::min(z.by0, v[2u * i + 1u]);
      z.by1 = std::max(z.by1, v[2u * i + 1u]);
    }
    z.first = zones[k].first;
    z.count = zones[k].count;
    z.split = 1u;
    uint32_t r1 = 0;
    if (zone_cells(z.bx0, z.bx1, P.off_x, P.cell_size, g.org_x, lo_x, hi_x, &z.r0, &r1) &&
        zone_cells(z.by0, z.by1, P.off_y, P.cell_size, g.org_y, lo_y, hi_y, &z.c0, &z.c1))
      z.rows = r1 - z.r0 + 1u;
    rows_all += z.rows;
  }
  const uint64_t R = std::max<uint64_t>((rows_all + ZONE_ITEMS_ROWS - 1u) / ZONE_ITEMS_ROWS, 1u);
  part->group_rows = (uint32_t)R;  // (rows_all < 2^16 * 2^31)
  // the shares: as many as an even crowd would need for ZONE_WAVE_SLOTS slots per wave
  uint64_t items = 0;
  for (size_t k = 0; k < n; ++k) {
    ZoneDev& z = part->zones[k];
    part->item0[k] = (uint32_t)items;
    if (!z.rows) continue;
    const double slots = (double)e->n_slots * ((double)(z.c1 - z.c0 + 1u) * (double)std::min<uint64_t>(R, z.rows) / cells);
    z.split = (uint32_t)std::min(std::max(std::ceil(slots / (double)ZONE_WAVE_SLOTS), 1.0), (double)ZONE_SPLIT_MAX);
    items += ((z.rows + R - 1u) / R) * z.split;  // (at most (2^22 + 2^16) * 2^8 in all)
  }
  part->item0[n] = (uint32_t)items;
}

// the arrays both kernels read, at the front of a scratch block: where they are and how many bytes they take
struct ZoneTables {
  ZoneDev* zones;
  uint32_t* item0;
  double* vertices;
  size_t bytes;
};
size_t zone_tables_bytes(size_t n, size_t n_vertices) {
  return sel_up(n * sizeof(ZoneDev)) + sel_up((n + 1u) * sizeof(uint32_t)) + sel_up(n_vertices * 2u * sizeof(double));
}
int zone_tables_upload(cs_engine* e, unsigned char* p, const ZonePart& part, const double* vertices_xy, size_t n_vertices,
                       ZoneTables* t) {
  const size_t n = part.zones.size();
  t->zones = reinterpret_cast<ZoneDev*>(p);
  t->item0 = reinterpret_cast<uint32_t*>(p + sel_up(n * sizeof(ZoneDev)));
  t->vertices = reinterpret_cast<double*>(p + sel_up(n * sizeof(ZoneDev)) + sel_up((n + 1u) * sizeof(uint32_t)));
  t->bytes = zone_tables_bytes(n, n_vertices);
  HIP_OK_E(e, hipMemcpyAsync(t->zones, part.zones.data(), n * sizeof(ZoneDev), hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(t->item0, part.item0.data(), (n + 1u) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipMemcpyAsync(t->vertices, vertices_xy, n_vertices * 2u * sizeof(double), hipMemcpyHostToDevice, e->stream));
  return 0;
}

// All n zones (n > 0, checked) against the agents one engine holds (after sel_begin), counted: part->total, and with
// want_counts part->counts.  One memset of the header and one of the counts, three uploads, one kernel, one read back
// (and one download of the counts): no row is made.
int zone_count(cs_engine* e, const cs_zone* zones, size_t n, const double* vertices_xy, size_t n_vertices,
               const cs_selection* filter, bool want_counts, ZonePart* part) {
  part->zones.clear();
  part->item0.clear();
  part->counts.assign(n, 0u);
  part->total = 0;
  if (int rc = e->refresh_counts()) return rc;
  if (int rc = e->ensure_index()) return rc;
  if (!e->n_slots) return 0;
  const PairsArgs P = pairs_args(e, 0.0, filter, nullptr);
  zone_plan(e, zones, n, vertices_xy, P, part);
  const uint32_t items = part->item0[n];
  if (!items) return 0;
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  PairsScratch sc(e);
  const size_t b_tab = zone_tables_bytes(n, n_vertices);
  unsigned char* p = static_cast<unsigned char*>(sc.get(b_tab + n * sizeof(uint64_t)));
  if (!p) return 90;
  ZoneTables t;
  if (int rc = zone_tables_upload(e, p, *part, vertices_xy, n_vertices, &t)) return rc;
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(p + b_tab);
  HIP_OK_E(e, hipMemsetAsync(d_counts, 0, n * sizeof(uint64_t), e->stream));
  const uint32_t blocks = (items + PAIRS_WAVES - 1u) / PAIRS_WAVES;
  hipLaunchKernelGGL(k_zone_count, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], e->n_slots,
                     e->cell_start.get(), e->sel_groups_dev.get(), P, t.zones, t.item0, (uint32_t)n, items, part->group_rows, t.vertices,
                     d_counts, hdr);
  HIP_OK_E(e, hipGetLastError());
  if (want_counts)
    HIP_OK_E(e, hipMemcpyAsync(part->counts.data(), d_counts, n * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
  unsigned long long found = 0;
  if (int rc = pairs_read_count(e, hdr, &found)) return rc;  // (synchronised: the host staging may go)
  part->total = found;
  return 0;
}

// The first min(part.total, want) rows of what zone_count counted (with its counts; part.total at most CS_PAIRS_MAX),
// ascending by (zone, id), as keys (zone << 32 | DEVICE id).  Two memsets, four uploads, one kernel, one read back, three
// launches per 4 bits of the largest id and of the largest zone, one download.
int zone_list(cs_engine* e, const ZonePart& part, const double* vertices_xy, size_t n_vertices, const cs_selection* filter,
              size_t want, std::vector<uint64_t>* out) {
  out->clear();
  const size_t n = part.zones.size();
  const uint64_t found = part.total;
  if (!want || !found || !n) return 0;
  std::vector<uint64_t> offsets(n + 1u, 0u);
  for (size_t k = 0; k < n; ++k) offsets[k + 1u] = offsets[k] + part.counts[k];
  if (offsets[n] != found) {
    e->error = "zone_agents: the counts of the zones do not add up to the total";
    return 90;
  }
  const PairsArgs P = pairs_args(e, 0.0, filter, nullptr);
  const uint32_t items = part.item0[n];
  unsigned long long* hdr = nullptr;
  if (int rc = pairs_header(e, &hdr)) return rc;
  PairsScratch sc(e);
  const size_t b_tab = zone_tables_bytes(n, n_vertices);
  const size_t b_off = sel_up((n + 1u) * sizeof(uint64_t)), b_cur = sel_up(n * sizeof(uint32_t));
  const size_t b = sel_up((size_t)found * sizeof(uint64_t));
  const size_t tiles = ((size_t)found + IDS_TILE - 1u) / IDS_TILE;
  const size_t b_hist = sel_up(IDS_RADIX * std::max<size_t>(tiles, 1u) * sizeof(uint32_t));
  unsigned char* p = static_cast<unsigned char*>(sc.get(b_tab + b_off + b_cur + 2u * b + b_hist + 256u));
  if (!p) return 90;
  ZoneTables t;
  if (int rc = zone_tables_upload(e, p, part, vertices_xy, n_vertices, &t)) return rc;
  unsigned long long* d_off = reinterpret_cast<unsigned long long*>(p + b_tab);
  uint32_t* d_cur = reinterpret_cast<uint32_t*>(p + b_tab + b_off);
  unsigned char* q = p + b_tab + b_off + b_cur;
  unsigned long long *keys = reinterpret_cast<unsigned long long*>(q), *keys_other = reinterpret_cast<unsigned long long*>(q + b);
  uint32_t* hist = reinterpret_cast<uint32_t*>(q + 2u * b);
  HIP_OK_E(e, hipMemcpyAsync(d_off, offsets.data(), (n + 1u) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipMemsetAsync(d_cur, 0, n * sizeof(uint32_t), e->stream));
  const uint32_t blocks = (items + PAIRS_WAVES - 1u) / PAIRS_WAVES;
  hipLaunchKernelGGL(k_zone_emit, dim3(blocks), dim3(PAIRS_BLOCK), 0, e->stream, e->gdev, e->buf[e->cur], e->n_slots,
                     e->cell_start.get(), e->sel_groups_dev.get(), P, t.zones, t.item0, (uint32_t)n, items, part.group_rows, t.vertices,
                     d_off, d_cur, hdr, keys);
  HIP_OK_E(e, hipGetLastError());
  unsigned long long back[3];
  if (int rc = pairs_read_header(e, hdr, back)) return rc;  // (synchronised: the host staging may go)
  if (back[1] != found) {
    e->error = "zone_agents: the listing found another number of rows than the count";
    return 90;
  }
  const uint32_t rows = (uint32_t)found;  // (at most CS_PAIRS_MAX)
  if (rows > 1u) {  // the id in the low half, the zone in the high half
    if (int rc = pairs_radix(e, &keys, &keys_other, nullptr, nullptr, hist, rows, 0u, pairs_bits((uint32_t)back[2])))
      return rc;
    if (n > 1u)
      if (int rc = pairs_radix(e, &keys, &keys_other, nullptr, nullptr, hist, rows, 32u, pairs_bits((uint32_t)(n - 1u))))
        return rc;
  }
  const uint32_t take = (uint32_t)std::min<size_t>(want, rows);
  out->resize(take);
  HIP_OK_E(e, hipMemcpyAsync(out->data(), keys, take * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  return 0;
}

int zone_too_many(std::string* error) {
  *error = "zone_agents: too many zone agents to list (more than CS_PAIRS_MAX = 67108864); the count-only form has no limit";
  return 3;
}

// device ids -> external ids, into the caller's rows
void zone_copy_out(const cs_engine* ids_of, const std::vector<uint64_t>& list, cs_zone_agent* out, size_t cap) {
  const size_t k = std::min(list.size(), cap);
  for (size_t i = 0; i < k; ++i) {
    out[i].zone = list[i] >> 32;
    out[i].id = ids_of->ext_id(list[i] & 0xFFFFFFFFull);
  }
}

}  // namespace

extern "C" {

size_t cs_zone_agents(cs_engine* e, const cs_zone* zones, size_t n, const double* vertices_xy, size_t n_vertices,
                      const cs_selection* filter, uint64_t* out_counts, cs_zone_agent* out, size_t cap) {
  if (!e) return SIZE_MAX;
  hipSetDevice(e->device);
  if (zones_check(&e->error, zones, n, vertices_xy, n_vertices, filter)) return SIZE_MAX;
  if (sel_begin(e)) return SIZE_MAX;
  if (!n) return 0;
  const size_t want = out ? cap : 0u;
  ZonePart part;
  if (zone_count(e, zones, n, vertices_xy, n_vertices, filter, want || out_counts, &part)) return SIZE_MAX;
  if (want && part.total > CS_PAIRS_MAX) {
    zone_too_many(&e->error);
    return SIZE_MAX;
  }
  std::vector<uint64_t> list;
  if (zone_list(e, part, vertices_xy, n_vertices, filter, want, &list)) return SIZE_MAX;
  if (out_counts) std::copy(part.counts.begin(), part.counts.end(), out_counts);
  if (want) zone_copy_out(e, list, out, cap);
  return (size_t)part.total;
}

// Collective: one gather of variable size (two collectives) for the counts and, when listing, one more for the rows,
// whatever the crowd and the answer: a rank that failed, or a listing that is refused, sends its word alone.  n == 0
// makes none: every rank passes the same n.  No halo exchange, no band: a tile's walk is clipped to the cells it owns and
// every agent is owned by one tile.
size_t cs_mesh_zone_agents(cs_mesh* m, const cs_zone* zones, size_t n, const double* vertices_xy, size_t n_vertices,
                           const cs_selection* filter, uint64_t* out_counts, cs_zone_agent* out, size_t cap) {
  if (!m) return SIZE_MAX;
  if (m->dead()) return SIZE_MAX;
  if (zones_check(&m->error, zones, n, vertices_xy, n_vertices, filter)) return SIZE_MAX;
  if (cs_mesh_synchronize(m)) return SIZE_MAX;
  hipSetDevice(m->device);
  if (!n) return 0;
  const size_t want = out ? cap : 0u;
  const char* const other_failed = "a tile of another rank failed while listing zone agents";
  int err = 0;
  std::string why;
  // 1. every tile counts; the counts of all tiles of all ranks: [0 ok / 1 failed, n counts]
  std::vector<ZonePart> parts(m->tiles.size());
  std::vector<uint64_t> counts(n, 0u);
  for (size_t k = 0; k < m->tiles.size(); ++k) {
    cs_engine* e = m->tiles[k];
    if (!err) err = sel_begin(e);
    if (!err) err = zone_count(e, zones, n, vertices_xy, n_vertices, filter, true, &parts[k]);
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
  // 2. when listing: the rows of every tile, merged; then those of every rank: [0 ok / 1 failed, keys]
  std::vector<uint64_t> all;
  if (want) {
    std::vector<size_t> ends;
    for (size_t k = 0; k < m->tiles.size() && !err && !too_many; ++k) {
      std::vector<uint64_t> part;
      err = zone_list(m->tiles[k], parts[k], vertices_xy, n_vertices, filter, want, &part);
      if (err) why = cs_last_error(m->tiles[k]);
      all.insert(all.end(), part.begin(), part.end());
      ends.push_back(all.size());
    }
    mesh_merge_runs(all, ends);
    if (all.size() > want) all.resize(want);
    if (m->distributed) {
      const size_t rows = (err || too_many) ? 0u : all.size();
      std::vector<uint64_t> mine(1u + rows, err ? 1u : 0u);
      std::copy(all.begin(), all.begin() + (long)rows, mine.begin() + 1);
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
        if (!words || w[0] != 0u) {
          if (!err) {
            err = 90;
            why = other_failed;
          }
          continue;
        }
        all.insert(all.end(), w.begin() + 1, w.end());
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
    zone_too_many(&m->error);
    return SIZE_MAX;
  }
  if (out_counts) std::copy(counts.begin(), counts.end(), out_counts);
  if (want && !m->tiles.empty()) zone_copy_out(m->tiles[0], all, out, cap);
  return (size_t)total;
}

}  // extern "C"
