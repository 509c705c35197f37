// cs_agents_by_id.hip.inc — reading and removing agents between steps, by id, a batch at a time
// (include/crowdstep_state.h).  Part of the single translation unit crowdstep_hip.hip (included there, after
// cs_agent_write.hip.inc, whose match kernel, launch and scratch it shares).
//
// The reference's host reads `agents.get(&id)` and calls `remove_agents(id)` (lib.rs:71, :176-192).  cs_read_agents
// downloads every column of every slot and cs_remove_agent scans all slots once per id; both have the shape of the
// write: a sorted batch of ids matched against the slots in one pass (DESIGN.md section 2, "Reading and removing
// agents by id").
//   host      map external ids to device ids, sort them (the read drops repeats, the remove refuses them), serve the
//             agents the index never took (`limbo`) from the host list, upload the keys once
//   K_match   k_write_match as the write uses it: slot_of[r] (and meta_of[r]) of every key that a live (owned) slot holds
//   read      k_agents_gather: one thread per key packs its slot's columns into one 32-byte record; one download of the
//             records; the host converts them exactly as cs_read_agents converts a downloaded slot
//   remove    one read back of the match count and the meta words; anything short refuses the batch with nothing
//             changed; k_agents_kill then marks the matched slots dead and the host clears, once, the flags a single
//             remove clears and queues the events and planner callbacks in the order of the batch
// The step kernels are not touched.  A read changes no flag of the engine.

// one matched agent as the device packs it (32 B); `found` = 0: no live (owned) slot holds the key, the rest is zero
struct AgentRec {
  uint32_t cell, meta;
  float ox, oy, vx, vy;
  uint32_t id, found;
};

// K_gather: record r from slot slot_of[r] (below n_slots: checked, whatever the match found)
__global__ void __launch_bounds__(256)
    k_agents_gather(AgentArrays a, uint32_t n_slots, const uint32_t* __restrict__ slot_of, uint32_t n,
                    AgentRec* __restrict__ out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t i = slot_of[r];
  AgentRec v;
  v.cell = 0u; v.meta = 0u; v.ox = 0.f; v.oy = 0.f; v.vx = 0.f; v.vy = 0.f; v.id = 0u; v.found = 0u;
  if (i < n_slots) {
    const float2 off = a.off[i], vel = a.vel[i];
    v.cell = a.cell[i];
    v.meta = a.meta[i];
    v.ox = off.x; v.oy = off.y; v.vx = vel.x; v.vy = vel.y;
    v.id = a.id[i];
    v.found = 1u;
  }
  out[r] = v;
}

// K_kill: the slot of every matched key dies (launched only after the host has seen a full match count)
__global__ void __launch_bounds__(256)
    k_agents_kill(AgentArrays a, uint32_t n_slots, const uint32_t* __restrict__ slot_of, uint32_t n) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t i = slot_of[r];
  if (i < n_slots) a.cell[i] = CS_INVALID_CELL;
}

namespace {

constexpr uint32_t kNoKey = 0xFFFFFFFFu;

// A batch of ids on its way: the distinct device ids among them, ascending, and where each asked id went.
struct IdBatch {
  std::vector<uint32_t> keys;    // distinct device ids, ascending
  std::vector<uint32_t> key_of;  // per asked id: its index in `keys`, or kNoKey (no live agent can hold this id)
  bool repeats = false;          // some device id was asked for more than once
  // device scratch of the call: keys, slot_of, [count | meta_of], records
  uint32_t* d_keys = nullptr;
  uint32_t* d_slot = nullptr;
  uint32_t* d_words = nullptr;
  AgentRec* d_recs = nullptr;
};

// Host part: external ids to device ids (the engine's own mapping, so a renumbered id is found under its external
// name), sorted.  `skip[k]` != 0: the id is served elsewhere (the limbo list) and gets no key.
void ids_prepare(const cs_engine* e, const uint64_t* ids, size_t n, const std::vector<uint8_t>& skip, IdBatch* b) {
  std::vector<std::pair<uint32_t, uint32_t>> order;  // (device id, asked index)
  order.reserve(n);
  b->key_of.assign(n, kNoKey);
  for (size_t k = 0; k < n; ++k) {
    uint64_t dev = 0;
    if (skip[k] || !e->dev_id(ids[k], &dev) || dev >= e->id_limit || dev >= 0xFFFFFFFFull) continue;
    order.emplace_back((uint32_t)dev, (uint32_t)k);
  }
  std::sort(order.begin(), order.end());
  b->keys.clear();
  b->repeats = false;
  for (size_t j = 0; j < order.size(); ++j) {
    if (j && order[j].first == order[j - 1].first) b->repeats = true;
    else b->keys.push_back(order[j].first);
    b->key_of[order[j].second] = (uint32_t)b->keys.size() - 1u;
  }
}

// The queued steps first (a failure of one of them is the call's), then one upload of the keys and K_match on the
// engine's stream.  Nothing is waited for here: the caller queues its own kernel and read back behind the match and
// synchronises once (b->keys stays alive until then).  `records`: room for the gather's output.  `extra_bytes`: room
// behind the match's own arrays for the caller's (cs_set_targets.hip.inc), returned in *extra (null where nothing was laid
// out: no keys or no slots).
int ids_match(cs_engine* e, IdBatch* b, bool want_meta, bool records, size_t extra_bytes = 0,
              unsigned char** extra = nullptr) {
  if (extra) *extra = nullptr;
  if (e->poisoned) {
    e->error = e->poison_error;
    return 1;
  }
  if (int rc = cs_synchronize(e)) return rc;
  const size_t n = b->keys.size();
  if (!n || !e->n_slots) return 0;
  auto up = [](size_t bytes) { return (bytes + 255u) & ~(size_t)255u; };
  const size_t b_keys = up(n * sizeof(uint32_t)), b_slot = b_keys, b_words = up((n + 1) * sizeof(uint32_t));
  const size_t b_recs = records ? up(n * sizeof(AgentRec)) : 0u;
  if (int rc = write_scratch_reserve(e, b_keys + b_slot + b_words + b_recs + extra_bytes)) return rc;
  unsigned char* s = static_cast<unsigned char*>(e->write_scratch.get());
  if (extra) *extra = s + b_keys + b_slot + b_words + b_recs;
  b->d_keys = reinterpret_cast<uint32_t*>(s);
  b->d_slot = reinterpret_cast<uint32_t*>(s + b_keys);
  b->d_words = reinterpret_cast<uint32_t*>(s + b_keys + b_slot);
  b->d_recs = records ? reinterpret_cast<AgentRec*>(s + b_keys + b_slot + b_words) : nullptr;
  HIP_OK_E(e, hipMemcpyAsync(b->d_keys, b->keys.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIP_OK_E(e, hipMemsetAsync(b->d_slot, 0xFF, n * sizeof(uint32_t), e->stream));
  HIP_OK_E(e, hipMemsetAsync(b->d_words, 0, sizeof(uint32_t), e->stream));
  if (want_meta) HIP_OK_E(e, hipMemsetAsync(b->d_words + 1, 0xFF, n * sizeof(uint32_t), e->stream));
  write_launch_match(e, b->d_keys, n, b->d_slot, want_meta ? b->d_words + 1 : nullptr, b->d_words);
  HIP_OK_E(e, hipGetLastError());
  return 0;
}

// ---- read ----

// What this engine holds of the batch: view[k] / found[k] for every asked id whose agent lives in one of its (owned)
// slots.  Entries of ids it does not hold are left alone (a mesh asks every tile in turn).  One upload, two kernels,
// one download, one wait.
int ids_read(cs_engine* e, const uint64_t* ids, size_t n, const std::vector<uint8_t>& skip, cs_agent_view* view,
             uint8_t* found, size_t* n_found) {
  IdBatch b;
  ids_prepare(e, ids, n, skip, &b);
  if (int rc = ids_match(e, &b, false, true)) return rc;
  const size_t nk = b.keys.size();
  if (!nk || !e->n_slots) return 0;
  hipLaunchKernelGGL(k_agents_gather, dim3((uint32_t)((nk + 255u) / 256u)), dim3(256), 0, e->stream, e->view(e->cur),
                     e->n_slots, b.d_slot, (uint32_t)nk, b.d_recs);
  HIP_OK_E(e, hipGetLastError());
  std::vector<AgentRec> recs(nk);
  HIP_OK_E(e, hipMemcpyAsync(recs.data(), b.d_recs, nk * sizeof(AgentRec), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  for (size_t k = 0; k < n; ++k) {
    if (b.key_of[k] == kNoKey) continue;
    const AgentRec& r = recs[b.key_of[k]];
    if (!r.found) continue;
    const uint32_t g = meta_group(e->gdev, r.meta);
    if (r.cell == CS_INVALID_CELL || g >= e->groups.size()) continue;
    cs_agent_view& v = view[k];  // (field by field as cs_read_agents fills it)
    v.id = e->ext_id(r.id);
    e->to_global(r.cell, r.ox, r.oy, &v.x, &v.y);
    v.vx = r.vx;
    v.vy = r.vy;
    v.next_waypoint = meta_waypoint(e->gdev, r.meta);
    v.eyesight_range = e->groups[g].eyesight;
    found[k] = 1;
    *n_found += 1;
  }
  return 0;
}

// found == NULL: every id must have been found; else the zeroed record of a missing id.  Writes `out` only on success.
int ids_read_finish(std::string* error, const uint64_t* ids, size_t n, std::vector<cs_agent_view>& view,
                    const std::vector<uint8_t>& hit, size_t n_found, cs_agent_view* out, uint8_t* found) {
  if (!found && n_found != n) {
    *error = "unknown agent id";
    return 2;
  }
  for (size_t k = 0; k < n; ++k) {
    if (!hit[k]) {
      std::memset(&view[k], 0, sizeof(cs_agent_view));
      view[k].id = ids[k];
    }
    out[k] = view[k];
    if (found) found[k] = hit[k];
  }
  return 0;
}

// ---- remove ----

// after the match, on one engine: its count and the meta words of what it holds, read back in one copy
int ids_read_back_match(cs_engine* e, const IdBatch& b, uint32_t* matched, std::vector<uint32_t>* meta_of) {
  const size_t nk = b.keys.size();
  *matched = 0;
  meta_of->assign(nk, 0xFFFFFFFFu);
  if (!nk || !e->n_slots) return 0;
  std::vector<uint32_t> words(nk + 1);
  HIP_OK_E(e, hipMemcpyAsync(words.data(), b.d_words, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_OK_E(e, hipStreamSynchronize(e->stream));
  *matched = words[0];
  std::copy(words.begin() + 1, words.end(), meta_of->begin());
  return 0;
}

// K_kill and, once, what cs_remove_agent does to the engine's flags and counts for every agent it removes
int ids_kill(cs_engine* e, const IdBatch& b, uint32_t matched) {
  e->halo_invalidate();
  if (!matched) return 0;
  const uint32_t nk = (uint32_t)b.keys.size();
  hipLaunchKernelGGL(k_agents_kill, dim3((nk + 255u) / 256u), dim3(256), 0, e->stream, e->view(e->cur), e->n_slots, b.d_slot,
                     nk);
  HIP_OK_E(e, hipGetLastError());
  HIP_OK_E(e, hipStreamSynchronize(e->stream));  // (the call's scratch is reused by the next call)
  e->sorted = false;
  e->hist_valid = false;
  e->occ_valid = false;
  e->n_alive_host -= matched;
  return 0;
}

// the planner callback and the DESTROYED event of one removed agent, as cs_remove_agent makes them
void ids_removed(cs_engine* e, uint64_t id, uint32_t hlp, uint32_t source_sink) {
  const cs_hlp_desc& p = e->hlps[hlp];
  if (p.kind == CS_HLP_CALLBACK && p.remove_agent) p.remove_agent(p.user, id);
  cs_event ev;
  ev.kind = CS_EVENT_DESTROYED;
  ev.source_sink = source_sink;
  ev.id = id;
  ev.x = ev.y = 0;
  if (e->record_events) e->events.push_back(ev);
}
void ids_removed(cs_engine* e, uint64_t id, uint32_t meta) {
  const HostGroup& g = e->groups[meta_group(e->gdev, meta)];
  ids_removed(e, id, g.hlp, g.sink >= 0 ? (uint32_t)g.sink : UINT32_MAX);
}

int ids_null_check(std::string* error, const void* ids, const void* out, size_t n, const char* what) {
  if (n && (!ids || !out)) {  // (`out`: the read's; a remove passes its ids again)
    *error = std::string(what) + ": null array";
    return 3;
  }
  return 0;
}

const char* const kIdTwice = "remove_agents: an agent id appears twice in the batch";

}  // namespace

extern "C" {

int cs_read_agents_by_id(cs_engine* e, const uint64_t* ids, size_t n, cs_agent_view* out, uint8_t* found) {
  if (!e) return 3;
  hipSetDevice(e->device);
  if (int rc = ids_null_check(&e->error, ids, out, n, "read_agents_by_id")) return rc;
  std::vector<cs_agent_view> view(n);
  std::vector<uint8_t> hit(n, 0);
  size_t n_found = 0;
  // the agents the index never took are served as cs_read_agents lists them: as created (lib.rs:133-144)
  for (size_t k = 0; k < n && !e->limbo.empty(); ++k)
    for (const cs_engine::LimboAgent& l : e->limbo)
      if (l.id == ids[k]) {
        cs_agent_view& v = view[k];
        std::memset(&v, 0, sizeof v);
        v.id = l.id;
        v.x = l.x;
        v.y = l.y;
        v.eyesight_range = e->groups[l.group].eyesight;
        hit[k] = 1;
        n_found += 1;
        break;
      }
  const std::vector<uint8_t> in_limbo(hit);
  if (int rc = ids_read(e, ids, n, in_limbo, view.data(), hit.data(), &n_found)) return rc;
  return ids_read_finish(&e->error, ids, n, view, hit, n_found, out, found);
}

int cs_remove_agents(cs_engine* e, const uint64_t* ids, size_t n) {
  if (!e) return 3;
  hipSetDevice(e->device);
  if (int rc = ids_null_check(&e->error, ids, ids, n, "remove_agents")) return rc;
  // the host's part of the batch: agents the index never took (cs_remove_agent serves them from the same list)
  std::vector<uint8_t> in_limbo(n, 0);
  std::vector<size_t> limbo_at(n, 0);
  std::vector<uint8_t> limbo_taken(e->limbo.size(), 0);
  size_t n_limbo = 0;
  for (size_t k = 0; k < n && !e->limbo.empty(); ++k)
    for (size_t j = 0; j < e->limbo.size(); ++j)
      if (e->limbo[j].id == ids[k]) {
        if (limbo_taken[j]) {
          e->error = kIdTwice;
          return 3;
        }
        limbo_taken[j] = 1;
        in_limbo[k] = 1;
        limbo_at[k] = j;
        n_limbo += 1;
        break;
      }
  IdBatch b;
  ids_prepare(e, ids, n, in_limbo, &b);
  for (size_t k = 0; k < n; ++k)
    if (!in_limbo[k] && b.key_of[k] == kNoKey) {
      e->error = "unknown agent id";
      return 2;
    }
  if (b.repeats) {
    e->error = kIdTwice;
    return 3;
  }
  uint32_t matched = 0;
  std::vector<uint32_t> meta_of;
  if (int rc = ids_match(e, &b, true, false)) return rc;
  if (int rc = ids_read_back_match(e, b, &matched, &meta_of)) return rc;
  bool all = (size_t)matched + n_limbo == n;
  for (size_t r = 0; all && r < meta_of.size(); ++r)
    all = meta_of[r] != 0xFFFFFFFFu && meta_group(e->gdev, meta_of[r]) < e->groups.size();
  if (!all) {
    e->error = "unknown agent id";  // (as cs_remove_agent: a removed or despawned id)
    return 2;
  }
  if (!n) return 0;
  if (int rc = ids_kill(e, b, matched)) return rc;
  for (size_t k = 0; k < n; ++k) {
    // (a limbo agent's event names no source-sink: cs_remove_agent)
    if (in_limbo[k]) ids_removed(e, ids[k], e->groups[e->limbo[limbo_at[k]].group].hlp, UINT32_MAX);
    else ids_removed(e, ids[k], meta_of[b.key_of[k]]);
  }
  if (n_limbo) {
    std::vector<cs_engine::LimboAgent> kept;
    for (size_t j = 0; j < e->limbo.size(); ++j)
      if (!limbo_taken[j]) kept.push_back(e->limbo[j]);
    e->limbo.swap(kept);
  }
  return 0;
}

// Collective.  The mesh's limbo list (the same on every rank) is served on the host; every tile matches the rest against
// the agents it owns; the found records travel in one gather, so that every rank returns the whole answer.
int cs_mesh_read_agents_by_id(cs_mesh* m, const uint64_t* ids, size_t n, cs_agent_view* out, uint8_t* found) {
  if (!m) return 3;
  if (m->dead()) return m->poison_rc;
  if (int rc = ids_null_check(&m->error, ids, out, n, "read_agents_by_id")) return rc;
  if (int rc = cs_mesh_synchronize(m)) return rc;  // queued steps first; a failure of one of them is the read's
  hipSetDevice(m->device);
  std::vector<cs_agent_view> view(n);
  std::vector<uint8_t> hit(n, 0);
  size_t n_found = 0;
  for (size_t k = 0; k < n && !m->limbo.empty(); ++k)
    for (const cs_mesh::Limbo& l : m->limbo)
      if (l.view.id == ids[k]) {
        view[k] = l.view;
        hit[k] = 1;
        n_found += 1;
        break;
      }
  const std::vector<uint8_t> in_limbo(hit);
  int err = 0;
  std::string why;
  for (cs_engine* e : m->tiles)
    if (!err && (err = ids_read(e, ids, n, in_limbo, view.data(), hit.data(), &n_found)) != 0) why = cs_last_error(e);
  if (m->distributed) {
    // what this rank's tiles found, as (asked index, record); a rank that failed says so in the first word
    struct Sent {
      uint64_t k;
      cs_agent_view v;
    };
    std::vector<Sent> mine;
    mine.push_back(Sent{(uint64_t)(err ? 1 : 0), cs_agent_view{}});
    for (size_t k = 0; !err && k < n; ++k)
      if (hit[k] && !in_limbo[k]) mine.push_back(Sent{(uint64_t)k, view[k]});
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
            why = "a tile of another rank failed while reading agents";
          }
          continue;
        }
        if ((int)r == m->rank || s.k >= n || hit[s.k]) continue;
        view[s.k] = s.v;
        hit[s.k] = 1;
        n_found += 1;
      }
    }
  }
  if (err) {
    m->error = why;
    return err;
  }
  return ids_read_finish(&m->error, ids, n, view, hit, n_found, out, found);
}

// Collective.  Every tile matches the batch against the agents it owns; the counts are summed over the tiles and the
// ranks (one gather, whatever n is) before any slot dies.
int cs_mesh_remove_agents(cs_mesh* m, const uint64_t* ids, size_t n) {
  if (!m) return 3;
  if (m->dead()) return m->poison_rc;
  if (int rc = ids_null_check(&m->error, ids, ids, n, "remove_agents")) return rc;
  if (int rc = cs_mesh_synchronize(m)) return rc;
  hipSetDevice(m->device);
  // host checks: the same batch gives the same answer on every rank (the limbo list and the id tables are the same)
  std::vector<uint8_t> in_limbo(n, 0);
  std::vector<size_t> limbo_at(n, 0);
  std::vector<uint8_t> limbo_taken(m->limbo.size(), 0);
  size_t n_limbo = 0;
  for (size_t k = 0; k < n && !m->limbo.empty(); ++k)
    for (size_t j = 0; j < m->limbo.size(); ++j)
      if (m->limbo[j].view.id == ids[k]) {
        if (limbo_taken[j]) {
          m->error = kIdTwice;
          return 3;
        }
        limbo_taken[j] = 1;
        in_limbo[k] = 1;
        limbo_at[k] = j;
        n_limbo += 1;
        break;
      }
  const size_t nt = m->tiles.size();
  std::vector<IdBatch> batch(nt);
  for (size_t t = 0; t < nt; ++t) {
    ids_prepare(m->tiles[t], ids, n, in_limbo, &batch[t]);
    for (size_t k = 0; k < n; ++k)
      if (!in_limbo[k] && batch[t].key_of[k] == kNoKey) {
        m->error = "unknown agent id";
        return 2;
      }
    if (batch[t].repeats) {
      m->error = kIdTwice;
      return 3;
    }
  }
  struct Found {
    uint64_t matched;
    int32_t err;
    int32_t pad;
  } mine{0, 0, 0};
  std::string local_error;
  std::vector<uint32_t> matched(nt, 0);
  std::vector<std::vector<uint32_t>> meta_of(nt);
  for (size_t t = 0; t < nt; ++t) {
    cs_engine* e = m->tiles[t];
    int rc = ids_match(e, &batch[t], true, false);
    if (!rc) rc = ids_read_back_match(e, batch[t], &matched[t], &meta_of[t]);
    for (size_t r = 0; !rc && r < meta_of[t].size(); ++r)
      if (meta_of[t][r] != 0xFFFFFFFFu && meta_group(e->gdev, meta_of[t][r]) >= e->groups.size()) {
        e->error = "remove_agents: an agent of an unknown planner group";
        rc = 90;
      }
    if (rc && !mine.err) {
      mine.err = 90;
      local_error = e->error;
    }
    mine.matched += matched[t];
  }
  Found all_found = mine;
  if (m->distributed) {
    std::vector<Found> all((size_t)m->n_ranks);
    if (int rc = mesh_allgather(m, &mine, sizeof mine, all.data())) return m->poison(rc, m->error);
    all_found = Found{0, 0, 0};
    for (const Found& f : all) {
      all_found.matched += f.matched;
      if (!all_found.err) all_found.err = f.err;
    }
  }
  if (all_found.err) return m->poison(90, local_error.empty() ? "a tile of this mesh failed while removing agents" : local_error);
  if (all_found.matched + n_limbo != n) {
    m->error = "unknown agent id";
    return 2;
  }
  if (!n) return 0;
  for (size_t t = 0; t < nt; ++t)
    if (int rc = ids_kill(m->tiles[t], batch[t], matched[t]))
      return m->poison(rc, std::string("cs_mesh_remove_agents failed half way: ") + cs_last_error(m->tiles[t]));
  // events and callbacks in the order of the batch, each where cs_mesh_remove_agent puts it: the owning tile's queue,
  // rank 0 for an agent of the limbo list
  for (size_t k = 0; k < n; ++k) {
    if (in_limbo[k]) {
      cs_engine* e = m->tiles[0];
      const cs_hlp_desc& p = e->hlps[m->limbo[limbo_at[k]].hlp];
      if (p.kind == CS_HLP_CALLBACK && p.remove_agent && m->rank == 0) p.remove_agent(p.user, ids[k]);
      if (m->recording && m->rank == 0) {
        cs_event ev;
        ev.kind = CS_EVENT_DESTROYED;
        ev.source_sink = UINT32_MAX;
        ev.id = ids[k];
        ev.x = ev.y = 0;
        e->events.push_back(ev);
      }
      continue;
    }
    for (size_t t = 0; t < nt; ++t) {
      const uint32_t meta = meta_of[t].empty() ? 0xFFFFFFFFu : meta_of[t][batch[t].key_of[k]];
      if (meta != 0xFFFFFFFFu) ids_removed(m->tiles[t], ids[k], meta);
    }
  }
  if (n_limbo) {
    std::vector<cs_mesh::Limbo> kept;
    for (size_t j = 0; j < m->limbo.size(); ++j)
      if (!limbo_taken[j]) kept.push_back(m->limbo[j]);
    m->limbo.swap(kept);
  }
  return 0;
}

}  // extern "C"
