// cs_set_targets.hip.inc — sending agents to goals between steps, by id, a batch at a time (include/crowdstep_state.h).
// Part of the single translation unit crowdstep_hip.hip (included there, after cs_agents_by_id.hip.inc, whose id batch,
// match and scratch it shares).
//
// The reference's host calls `planner.set_target(&sim.agents[&id], goal, tol)` (rmf/mod.rs:217-236) whenever it wants
// somebody to go somewhere.  Here a batch of (id, goal) entries has the effect of those calls made in the order of the
// batch (DESIGN.md section 2, "Sending agents to goals between steps"):
//   host      external ids to device ids, sorted distinct keys (ids_prepare); the keys, and per entry its key and goal,
//             are uploaded
//   K_match   k_write_match as the read and the remove use it
//   K_probe   k_target_probe, one thread per entry: slot -> the agent's global f64 position exactly as step_epilogue
//             forms it -> its group; for a CS_HLP_ROUTE planner the four route_spatial_hash values -> route_book_find
//   host      one download of the probe records.  An entry nobody holds refuses the batch before any planner is called.
//             One pass over the entries in batch order, which for an entry the probe answered only notes its route (no
//             hash lookup); a pair the book lacks goes through route_lookup (it finds what an earlier entry of the batch
//             has just planned, else plans), a host planner's entry calls it
//   assign    flush_route_tables if routes were added, then k_route_assign with (slot, route) pairs, the last entry of
//             every agent only
// The step kernels are not touched.

// what the device knows of one entry (32 B); slot == 0xFFFFFFFF: no live (owned) slot holds the entry's agent
struct TargetRec {
  double px, py;
  uint32_t slot, group, route1, pad;
};

// K_probe.  key_of[k] indexes slot_of (the match's answer per distinct key) or is 0xFFFFFFFF; every index is checked.
__global__ void __launch_bounds__(256)
    k_target_probe(GridDev g, AgentArrays a, uint32_t n_slots, const GroupDev* __restrict__ groups, uint32_t n_groups,
                   const double* __restrict__ hlp_scale, const RouteBookEntry* __restrict__ book, uint32_t book_mask,
                   double grid_off_x, double grid_off_y, double cell_size, const uint32_t* __restrict__ slot_of,
                   uint32_t n_keys, const uint32_t* __restrict__ key_of, const double* __restrict__ goals, uint32_t n,
                   TargetRec* __restrict__ out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  TargetRec r;
  r.px = 0.0; r.py = 0.0; r.slot = 0xFFFFFFFFu; r.group = 0xFFFFFFFFu; r.route1 = 0u; r.pad = 0u;
  const uint32_t key = key_of[k];
  const uint32_t i = key < n_keys ? slot_of[key] : 0xFFFFFFFFu;
  const uint32_t cell = i < n_slots ? a.cell[i] : CS_INVALID_CELL;
  if (cell != CS_INVALID_CELL) {
    const uint32_t gx = cell / g.nx, gy = cell - gx * g.nx;
    const float2 off = a.off[i];
    // (the expression of step_epilogue and cs_engine::to_global: the host plans from the very same f64 value)
    r.px = grid_off_x + ((double)(g.org_x + gx) * cell_size + (double)off.x);
    r.py = grid_off_y + ((double)(g.org_y + gy) * cell_size + (double)off.y);
    r.slot = i;
    r.group = meta_group(g, a.meta[i]);
    if (r.group < n_groups) {
      const GroupDev grp = groups[r.group];
      if (grp.hlp_kind == CS_HLP_ROUTE && hlp_scale) {
        const double res = hlp_scale[grp.hlp];
        r.route1 = route_book_find(book, book_mask, grp.hlp, route_spatial_hash(r.px, res), route_spatial_hash(r.py, res),
                                   route_spatial_hash(goals[2 * (size_t)k], res),
                                   route_spatial_hash(goals[2 * (size_t)k + 1], res));
      }
    }
  }
  out[k] = r;
}

namespace {

// null arrays, a batch too long for one launch, a non-finite goal or tolerance (3): before anything else
int targets_check(std::string* error, const uint64_t* ids, const double* goals, size_t n, double tol_x, double tol_y) {
  if (n && (!ids || !goals)) {
    *error = "set_targets: null array";
    return 3;
  }
  if (n >= 0xFFFFFFFFull) {
    *error = "set_targets: more than 2^32 - 2 entries in one batch";
    return 3;
  }
  bool finite = std::isfinite(tol_x) && std::isfinite(tol_y);
  for (size_t k = 0; finite && k < 2 * n; ++k) finite = std::isfinite(goals[k]);
  if (!finite) {
    *error = "set_targets: a goal or tolerance is not finite";
    return 3;
  }
  return 0;
}

// A batch on one engine between the probe and the assignment
struct TargetBatch {
  IdBatch ids;
  std::vector<TargetRec> recs;  // per entry, as downloaded (slot: in THIS engine's arrays)
  uint2* d_pairs = nullptr;     // room for one (slot, route) pair per distinct key
};

// The queued steps first, the tables the probe reads, then upload, K_match, K_probe and the one download.
// recs[k].slot stays 0xFFFFFFFF for an entry whose agent this engine does not hold.  Changes nothing but the scratch.
int targets_probe(cs_engine* e, const uint64_t* ids, const double* goals, size_t n, TargetBatch* t) {
  if (e->poisoned) {
    e->error = e->poison_error;
    return 1;
  }
  if (int rc = cs_synchronize(e)) return rc;
  TargetRec none;
  std::memset(&none, 0, sizeof none);
  none.slot = none.group = 0xFFFFFFFFu;
  t->recs.assign(n, none);
  ids_prepare(e, ids, n, std::vector<uint8_t>(n, 0), &t->ids);
  const size_t nk = t->ids.keys.size();
  if (!n || !nk || !e->n_slots) return 0;
  if (int rc = e->upload_groups()) return rc;
  if (e->any_route_hlp)
    if (int rc = e->flush_route_tables()) return rc;
  // the call's own arrays lie behind the match's in the engine's scratch
  auto up = [](size_t bytes) { return (bytes + 255u) & ~(size_t)255u; };
  const size_t b_keyof = up(n * sizeof(uint32_t)), b_goals = up(2 * n * sizeof(double));
  const size_t b_recs = up(n * sizeof(TargetRec)), b_pairs = up(nk * sizeof(uint2));
  unsigned char* s = nullptr;
  if (int rc = ids_match(e, &t->ids, false, false, b_keyof + b_goals + b_recs + b_pairs, &s)) return rc;
  if (!s) return 0;
  uint32_t* d_keyof = reinterpret_cast<uint32_t*>(s);
  double* d_goals = reinterpret_cast<double*>(s + b_keyof);
  TargetRec* d_recs = reinterpret_cast<TargetRec*>(s + b_keyof + b_goals);
  t->d_pairs = reinterpret_cast<uint2*>(s + b_keyof + b_goals + b_recs);
  {  // key_of and the goals in one upload (the scratch lays them out the same way)
    std::vector<unsigned char> host(b_keyof + 2 * n * sizeof(double));
    std::memcpy(host.data(), t->ids.key_of.data(), n * sizeof(uint32_t));
    std::memcpy(host.data() + b_keyof, goals, 2 * n * sizeof(double));
    HIP_OK_E(e, hipMemcpyAsync(d_keyof, host.data(), host.size(), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_target_probe, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, e->stream, e->gdev, e->view(e->cur),
                       e->n_slots, e->groups_dev.get(), (uint32_t)e->groups.size(), e->any_route_hlp ? e->hlp_scale_dev.get() : nullptr,
                       e->any_route_hlp ? e->route_book_dev.get() : nullptr, e->route_book_size ? e->route_book_size - 1u : 0u,
                       e->grid.offset_x, e->grid.offset_y, e->grid.cell_size, t->ids.d_slot, (uint32_t)nk, d_keyof, d_goals,
                       (uint32_t)n, d_recs);
    HIP_OK_E(e, hipGetLastError());
    HIP_OK_E(e, hipMemcpyAsync(t->recs.data(), d_recs, n * sizeof(TargetRec), hipMemcpyDeviceToHost, e->stream));
    HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (the host staging dies here)
  }
  for (TargetRec& r : t->recs)
    if (r.slot != 0xFFFFFFFFu && r.group >= e->groups.size()) r.slot = r.group = 0xFFFFFFFFu;
  return 0;
}

// What every tile knows of entry k once the probes are merged: where the agent stands, its group, what the book said.
struct TargetInfo {
  double px, py;
  uint32_t group, route1;
};

// The book part for the whole batch in batch order, then the assignment to the agents THIS engine holds (t->recs[k].slot).
// Every tile of a mesh runs it with the same `info` and so plans the same routes in the same order; a host planner is
// called by the tile that holds the agent (`call_planners`; a mesh makes those calls itself, in batch order over all its
// tiles).  `status` may be null.
int targets_resolve(cs_engine* e, TargetBatch* t, const uint64_t* ids, const double* goals, size_t n, double tol_x,
                    double tol_y, const std::vector<TargetInfo>& info, bool call_planners, uint8_t* status) {
  const size_t nk = t->ids.keys.size();
  std::vector<uint32_t> last(nk, 0u), slot_of_key(nk, 0xFFFFFFFFu);  // per key: the route of its last routed entry
  bool any_routed = false;
  for (size_t k = 0; k < n; ++k) {
    const TargetInfo& a = info[k];
    const uint32_t hlp = e->groups[a.group].hlp;
    const cs_hlp_desc& p = e->hlps[hlp];
    const bool mine = t->recs[k].slot != 0xFFFFFFFFu;
    uint8_t st = CS_TARGET_IGNORED;
    if (p.kind == CS_HLP_CALLBACK && p.set_target) {
      if (mine && call_planners) p.set_target(p.user, ids[k], a.px, a.py, goals[2 * k], goals[2 * k + 1], tol_x, tol_y);
      st = CS_TARGET_FORWARDED;
    } else if (p.kind == CS_HLP_ROUTE && p.route_plan) {
      uint32_t r1 = a.route1;  // (the book only grows: what the device found still stands)
      st = CS_TARGET_BOOKED;
      if (r1) e->n_targets_from_device_book += 1;
      if (!r1) {
        const size_t before = e->route_desc_host.size();
        r1 = e->route_lookup(hlp, a.px, a.py, goals[2 * k], goals[2 * k + 1]);
        if (!r1) st = CS_TARGET_NO_PATH;
        else if (e->route_desc_host.size() != before) st = CS_TARGET_PLANNED;
      }
      if (r1 && mine && t->ids.key_of[k] != kNoKey) {
        last[t->ids.key_of[k]] = r1;  // (route, waypoint 0)
        slot_of_key[t->ids.key_of[k]] = t->recs[k].slot;
        any_routed = true;
      }
    }
    if (status) status[k] = st;
  }
  if (e->routes_dirty)
    if (int rc = e->flush_route_tables()) return rc;
  if (any_routed) {
    std::vector<uint2> pairs;
    pairs.reserve(nk);
    for (size_t r = 0; r < nk; ++r)
      if (last[r]) pairs.push_back(make_uint2(slot_of_key[r], last[r]));
    const uint32_t np = (uint32_t)pairs.size();
    HIP_OK_E(e, hipMemcpyAsync(t->d_pairs, pairs.data(), np * sizeof(uint2), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_route_assign, dim3((np + 255u) / 256u), dim3(256), 0, e->stream, e->buf[e->cur].route, e->n_slots,
                       t->d_pairs, np);
    HIP_OK_E(e, hipGetLastError());
    HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (the pairs and the call's scratch are reused)
  }
  e->halo_invalidate();  // route state travels in halo records: an exchange made ahead is void
  return 0;
}

}  // namespace

extern "C" {

uint64_t cs_set_targets_device_hits(cs_engine* e) { return e ? e->n_targets_from_device_book : 0; }

int cs_set_targets(cs_engine* e, const uint64_t* ids, const double* goals_xy, size_t n, double tol_x, double tol_y,
                   uint8_t* out_status) {
  if (!e) return 3;
  hipSetDevice(e->device);
  if (int rc = targets_check(&e->error, ids, goals_xy, n, tol_x, tol_y)) return rc;
  TargetBatch t;
  if (int rc = targets_probe(e, ids, goals_xy, n, &t)) return rc;
  std::vector<TargetInfo> info(n);
  for (size_t k = 0; k < n; ++k) {
    const TargetRec& r = t.recs[k];
    if (r.slot == 0xFFFFFFFFu) {
      e->error = "unknown agent id";  // (as the write: a removed id, or an agent the index never took)
      return 2;
    }
    info[k] = TargetInfo{r.px, r.py, r.group, r.route1};
  }
  if (!n) return 0;
  return targets_resolve(e, &t, ids, goals_xy, n, tol_x, tol_y, info, true, out_status);
}

// Collective.  Every tile probes the batch against the agents it owns; what they found is merged over the tiles and the
// ranks (one gather, whatever n is) before any planner is called; then every tile runs the book part for the whole batch,
// so that all route books number routes alike, and assigns to the agents it owns.
int cs_mesh_set_targets(cs_mesh* m, const uint64_t* ids, const double* goals_xy, size_t n, double tol_x, double tol_y,
                        uint8_t* out_status) {
  if (!m) return 3;
  if (m->dead()) return m->poison_rc;
  if (int rc = targets_check(&m->error, ids, goals_xy, n, tol_x, tol_y)) return rc;
  if (int rc = cs_mesh_synchronize(m)) return rc;  // queued steps first; a failure of one of them is the call's
  hipSetDevice(m->device);
  const size_t nt = m->tiles.size();
  std::vector<TargetBatch> batch(nt);
  std::vector<TargetInfo> info(n, TargetInfo{0.0, 0.0, 0xFFFFFFFFu, 0u});
  std::vector<uint8_t> hit(n, 0);
  int err = 0;
  std::string why;
  for (size_t t = 0; t < nt; ++t) {
    if (!err && (err = targets_probe(m->tiles[t], ids, goals_xy, n, &batch[t])) != 0) why = cs_last_error(m->tiles[t]);
    for (size_t k = 0; !err && k < n; ++k) {
      const TargetRec& r = batch[t].recs[k];
      if (r.slot == 0xFFFFFFFFu || hit[k]) continue;
      info[k] = TargetInfo{r.px, r.py, r.group, r.route1};
      hit[k] = 1;
    }
  }
  if (m->distributed) {
    // what this rank's tiles hold, as (entry, info); a rank that failed says so in the first word
    struct Sent {
      uint64_t k;
      TargetInfo v;
    };
    std::vector<Sent> mine;
    mine.push_back(Sent{(uint64_t)(err ? 1 : 0), TargetInfo{0.0, 0.0, 0u, 0u}});
    for (size_t k = 0; !err && k < n; ++k)
      if (hit[k]) mine.push_back(Sent{(uint64_t)k, info[k]});
    std::vector<std::vector<unsigned char>> parts;
    if (int rc = mesh_host_gatherv(m, mine.data(), mine.size() * sizeof(Sent), parts)) return m->poison(rc, m->error);
    for (size_t r = 0; r < parts.size(); ++r) {
      const size_t cnt = parts[r].size() / sizeof(Sent);
      for (size_t j = 0; j < cnt; ++j) {
        Sent s;
        std::memcpy(&s, parts[r].data() + j * sizeof(Sent), sizeof s);
        if (j == 0) {
          if (s.k && !err) {
            err = 90;
            why = "a tile of another rank failed while setting targets";
          }
          continue;
        }
        if ((int)r == m->rank || s.k >= n || hit[s.k]) continue;
        info[s.k] = s.v;
        hit[s.k] = 1;
      }
    }
  }
  if (err) {
    m->error = why;
    return err;
  }
  for (size_t k = 0; k < n; ++k)
    for (size_t t = 0; t < nt; ++t)
      if (!hit[k] || info[k].group >= m->tiles[t]->groups.size()) {
        m->error = "unknown agent id";
        return 2;
      }
  if (!n) return 0;
  // the host planners first, in batch order, each called for the agents this rank's tiles own
  for (size_t k = 0; k < n; ++k)
    for (size_t t = 0; t < nt; ++t) {
      if (batch[t].recs[k].slot == 0xFFFFFFFFu) continue;
      const cs_engine* e = m->tiles[t];
      const cs_hlp_desc& p = e->hlps[e->groups[info[k].group].hlp];
      if (p.kind == CS_HLP_CALLBACK && p.set_target)
        p.set_target(p.user, ids[k], info[k].px, info[k].py, goals_xy[2 * k], goals_xy[2 * k + 1], tol_x, tol_y);
      break;
    }
  for (size_t t = 0; t < nt; ++t)
    if (int rc = targets_resolve(m->tiles[t], &batch[t], ids, goals_xy, n, tol_x, tol_y, info, false,
                                 t == 0 ? out_status : nullptr))
      return m->poison(rc, std::string("cs_mesh_set_targets failed half way: ") + cs_last_error(m->tiles[t]));
  return 0;
}

}  // extern "C"
