// cs_engine.hip.inc — host side: the engine (state machine of the step, tables, tiles, events)
// Part of the single translation unit crowdstep_hip.hip (included there, in order).

// ===========================================================================
// host side
// ===========================================================================
namespace {

inline uint64_t sat_usize(double v) {
  if (!(v > 0.0)) return 0;
  if (v >= 18446744073709551615.0) return UINT64_MAX;
  return (uint64_t)v;
}

inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// Seeded stand-in for PoissonCrowd (source_sink.rs:75-82, whose thread_rng is
// unseedable): Knuth's product method on uniforms from splitmix64(seed, step,
// draw).  Integer mixing + IEEE f64 products: the same sequence on any host.
inline uint64_t poisson_seeded(uint64_t seed, uint64_t step, double mean) {
  if (!(mean > 0.0)) return 0;
  double limit = std::exp(-mean), prod = 1.0;
  uint64_t k = 0;
  for (uint64_t draw = 0; draw < 1000000; ++draw) {
    uint64_t r = splitmix64(seed ^ splitmix64(step * 0x100000001B3ull + draw));
    double u = (double)((r >> 11) + 1) * (1.0 / 9007199254740993.0);
    prod *= u;
    if (prod <= limit) break;
    ++k;
  }
  return k;
}

struct HostSink {
  cs_source_sink_desc d;
  std::vector<double> waypoints;
  uint64_t calls = 0;
  bool alive = true;
  uint32_t group = 0;
  uint32_t spawn_route = 0;  // CS_HLP_ROUTE: (route + 1) of source -> first waypoint once planned
};

struct HostGroup {
  uint32_t hlp, lp;
  double eyesight;
  int32_t sink;
};

// CS_HLP_FIELD (cs_hlp_field.hip.inc): one entry per planner handle of the device table k_hlp_field reads; vxy == null:
// the planner is no field
struct HlpFieldDev {
  cs_field_desc d;
  const float2* vxy;
  uint32_t sampling, pad;
};
// ... and what the host keeps of a field planner: its samples on the device, and a pinned copy of the caller's buffer of
// the last cs_hlp_field_update with the event behind its upload (the next update waits for that one copy only)
struct HostHlpField {
  cs_field_desc d;
  uint32_t sampling = 0;
  DevBuf<float2> data;
  PinnedBuf<float2> stage;
  hipEvent_t staged = nullptr;
  bool stage_busy = false;
};

}  // namespace

#define HIP_OK(call)                                                                          \
  do {                                                                                        \
    hipError_t _e = (call);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      error = std::string("HIP error: ") + hipGetErrorString(_e) + " at " #call;              \
      return 90;                                                                              \
    }                                                                                         \
  } while (0)

struct cs_engine;
struct StepParams;
// the host LocalPlanners' turn in a step (crowdstep_hip.hip, next to the batch spatial queries it uses)
static int lp_callbacks_eval(cs_engine* e, const StepParams& P, const EpilogueCtx* Ep);
// the field planners' turn in a step: k_hlp_field fills `pref` for their agents (cs_hlp_field.hip.inc)
static int hlp_field_eval(cs_engine* e);

struct cs_engine {
  // grid (LocationHash2D::new, location_hash_2d.rs:33-51)
  cs_grid_desc grid;
  uint64_t nx = 0, ny = 0, ncells = 0;  // LOCAL grid: nx = row stride (columns), ny = rows
  uint64_t gnx = 0, gny = 0;            // global grid (== local unless this is a tile)
  GridDev gdev;
  bool tile = false;
  uint32_t halo_cells = 0;
  // Agents whose index insert failed in add_agents.  The reference has put such an agent into `agents` before
  // `add_or_update` returns Err (lib.rs:133-149): it exists (it is counted, read, and removable), it is in nobody's
  // neighbourhood, and every later `step` fails on it with "Index out of bounds" (lib.rs:299-302) until it is removed.
  // Kept on the host (a tile leaves this to its mesh).  One difference remains: an agent whose first step would carry it
  // INTO the grid is indexed by the reference from then on; here the step fails until the agent is removed.
  struct LimboAgent {
    uint64_t id;
    double x, y;
    uint32_t group;
  };
  std::vector<LimboAgent> limbo;
  uint64_t last_failed_add_id = UINT64_MAX;  // (for the mesh: id of the agent the last add_agents failed on)
  size_t last_failed_add_index = SIZE_MAX;
  struct HaloDir {
    HaloRecord* send = nullptr;
    HaloRecord* recv = nullptr;
    uint32_t cap = 0;
  } halo[8];  // 0..3 edges (XLO, XHI, YLO, YHI), 4..7 corners (one-phase exchange)
  void* rccl_comm = nullptr;    // ncclComm_t of the RCCL transport (cs_rccl_comm_init / _adopt)
  bool rccl_comm_owned = false;
  int32_t halo_peer[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  bool ghosts_present = false;  // a halo exchange (or a ghost spawn) ran since the last step: the arrays hold ghosts
  bool halo_all_clean = false;  // one-phase form: the send record counts are zero
  // One-phase form: the step kernels pack the agents they move into the band along a shared edge
  // themselves (EpilogueCtx::halo_band), so the next cs_halo_pack_all has nothing to launch.  Anything
  // that changes the agents between the step and that pack (add / remove / import / a failed step)
  // clears the flag, and the pack then runs over all agents as before.
  bool halo_one_phase = false;  // the host uses cs_halo_pack_all (set by its first call)
  bool halo_prepacked = false;  // the send buffers hold the records of the state in buf[cur]
  bool halo_fuse = true;        // CS_HALO_FUSE=0: always pack with the separate launch
  // CS_CFG_TILE_OVERLAP: the border windows' launch on a second stream, the next step's exchange
  // behind it (cs_tile_step_rccl), the interior windows meanwhile on the engine's stream
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_sorted = nullptr, ev_border = nullptr, ev_xchg = nullptr;
  bool tile_split_force = false;  // CS_TILE_SPLIT=1: split the launch without a communicator (tests: one stream)
  bool overlap_ready = false;    // set by cs_tile_step_rccl around its cs_step: an exchange may follow on aux_stream
  bool border_on_aux = false;    // the last step's border launch went to aux_stream
  bool exchanged_ahead = false;  // the recv buffers already hold the halo of the state in buf[cur] (ev_xchg)
  uint64_t n_exchanges_ahead = 0, n_exchanges_ahead_used = 0;  // (cs_kernel_stat)
  uint64_t n_targets_from_device_book = 0;  // entries of cs_set_targets that k_target_probe answered (cs_set_targets_device_hits)
  // the agents changed behind the step kernel's back: what it packed (and what may already have
  // been exchanged ahead) no longer describes buf[cur]
  void halo_invalidate() {
    halo_prepacked = false;
    exchanged_ahead = false;
  }
  int ensure_aux() {
    if (aux_stream) return 0;
    int lo = 0, hi = 0;
    HIP_OK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    // The second stream has the engine stream's priority.  Until round 5 it was created with the highest priority (so
    // that the border windows and the exchange behind them would not queue behind the interior launch): measured on
    // MI355X, a high-priority stream that merely WAITS on an event starves the dispatches of the normal-priority one:
    // every kernel on the engine's stream took ~7x longer (scan 7 -> 56 us, scatter 9 -> 68, interior windows 35 -> 106)
    // and a 125k-agent step went from 64 to 330 us (profiles/r05/overlap_ab_one_gpu.txt; CS_AUX_STREAM_PRIORITY=high
    // brings that back).
    const char* pr = getenv("CS_AUX_STREAM_PRIORITY");
    if (pr && pr[0] == 'h') HIP_OK(hipStreamCreateWithPriority(&aux_stream, hipStreamNonBlocking, hi));
    else HIP_OK(hipStreamCreateWithFlags(&aux_stream, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&ev_sorted, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&ev_border, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&ev_xchg, hipEventDisableTiming));
    return 0;
  }
  bool halo_counts_clean[2] = {false, false};  // send-buffer record counts of an axis are zero
  int device = 0;
  uint32_t flags = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string error;
  std::string backend;
  bool poisoned = false;
  std::string poison_error = "Index out of bounds";  // what every later call of a poisoned engine reports

  // agent buffers: buf[cur] holds the state, buf[cur^1] is the scatter / step target
  AgentArrays buf[2] = {};  // (views of buf_mem, which owns the columns)
  AgentBuf buf_mem[2];
  int cur = 0;
  uint64_t cap = 0;
  uint32_t n_slots = 0;     // slots in use in buf[cur]
  bool sorted = true;       // buf[cur] is in cell order, cell_start/n_alive match it
  bool hist_valid = false;  // cell_count + rank describe buf[cur]
  bool occ_valid = false;   // src_occupied describes the current positions
  DevBuf<float2> pref;      // callback-HLP velocities in sorted order
  DevBuf<uint32_t> cell_count, cell_start, block_totals;
  uint32_t n_scan_blocks = 0;
  DevBuf<Counters> ctr;
  PinnedBuf<Counters> ctr_host;
  DevBuf<uint2> destroyed;
  uint32_t destroyed_cap = 0;
  DevBuf<WpEvent> wp_events;
  uint32_t wp_events_cap = 0;
  DevBuf<BlockDesc> blk_desc;  // work decomposition of the tiled neighbour kernel
  uint32_t blk_desc_cap = 0;
  DevBuf<uint32_t> n_blocks_dev;
  DevBuf<EpilogueCtx> epi_dev;      // the step kernels' EpilogueCtx, one per output buffer (device)
  EpilogueCtx* epi_host = nullptr;  // ... and what was written there last
  bool epi_valid[2] = {false, false};
  double max_eyesight = 0.0;
  uint32_t tile_blocks_per_cu = 4;  // LDS budget target of the tiled kernel (tuning knobs)
  uint32_t tile_list_cap = 0;       // 0 = derive from the budget
  uint32_t tile_static_lds = 512;   // the kernel's own __shared__ arrays (queried at creation)
  uint32_t tile_static_lds_builders = 512;  // ... of the instantiations that carry builder workgroups
  uint32_t tile_min_rows = 0;       // list rows worth more than occupancy (0 = from the mean neighbour count)
  uint32_t tile_agents_slack = 0;
  uint32_t tile_rows = 2;      // owned rows per workgroup (1 = strips cut at agent granularity)
  uint32_t tile_target = TILE_THREADS;  // most agents a band window may hold (greedy windows)
  uint32_t tile_stage_cap = 0;  // test knob: the staging bound the window builder works with (0 = the real one)
  uint32_t tile_windows_cap = 0;  // test knob: the launch is sized for at most this many band windows (0 = the bound)
  DevBuf<uint32_t> band_prefix;
  DevBuf<uint32_t> tile_spill;  // spilled neighbour-list rows of the tiled kernel, per workgroup
  int tile_spill_rows = -1;        // -1: fill the 64-entry mask (64 - list_cap); CS_TILE_SPILL_ROWS

  // streaming agents view (cs_snapshot_request / _acquire): two buffers, a copy stream
  struct Snapshot {
    DevBuf<cs_snapshot_record> dev;
    PinnedBuf<cs_snapshot_record> host;
    DevBuf<uint32_t> count_dev;
    PinnedBuf<uint32_t> count_host;
    uint64_t cap = 0;
    hipEvent_t gathered = nullptr, copied = nullptr;
    bool in_flight = false;
    uint64_t step_index = 0;
  } snap[2];
  int snap_next = 0, snap_latest = -1;
  hipStream_t copy_stream = nullptr;
  uint64_t steps_done = 0;

  int snapshot_request() {
    if (poisoned) {
      error = poison_error;
      return 1;
    }
    Snapshot& s = snap[snap_next];
    if (!copy_stream) HIP_OK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    if (!s.gathered) {
      HIP_OK(hipEventCreateWithFlags(&s.gathered, hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
      HIP_OK(s.count_dev.alloc(1));
      HIP_OK(s.count_host.alloc(1));
    }
    if (s.in_flight) HIP_OK(hipEventSynchronize(s.copied));  // its previous transfer still owns the buffer
    const uint64_t need = std::max<uint64_t>(n_slots, 1);
    if (need > s.cap) {
      s.cap = 0;
      s.dev.release();
      s.host.release();
      const uint64_t ncap = need + need / 4 + 1024;
      HIP_OK(s.dev.alloc(ncap));
      HIP_OK(s.host.alloc(ncap));
      s.cap = ncap;
    }
    HIP_OK(hipMemsetAsync(s.count_dev.get(), 0, sizeof(uint32_t), stream));
    if (n_slots)
      hipLaunchKernelGGL(k_snapshot, dim3((n_slots + 255u) / 256u), dim3(256), 0, stream, gdev, buf[cur],
                         n_slots, grid.offset_x, grid.offset_y, grid.cell_size, s.dev.get(), (uint32_t)s.cap,
                         s.count_dev.get(), ext_tab_dev[0].get(), (uint32_t)ext_of.size(), (uint32_t)dev_base, ext_base);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(s.gathered, stream));
    HIP_OK(hipStreamWaitEvent(copy_stream, s.gathered, 0));
    HIP_OK(hipMemcpyAsync(s.count_host.get(), s.count_dev.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, copy_stream));
    if (n_slots)
      HIP_OK(hipMemcpyAsync(s.host.get(), s.dev.get(), (size_t)n_slots * sizeof(cs_snapshot_record),
                            hipMemcpyDeviceToHost, copy_stream));
    HIP_OK(hipEventRecord(s.copied, copy_stream));
    // the step kernels that follow on `stream` do not touch s.dev; the next request that wants
    // this buffer waits for s.copied first
    s.in_flight = true;
    s.step_index = steps_done;
    snap_latest = snap_next;
    snap_next ^= 1;
    return 0;
  }
  int snapshot_acquire(int wait, const cs_snapshot_record** out, size_t* n, uint64_t* step_index) {
    if (snap_latest < 0) return 1;
    Snapshot& s = snap[snap_latest];
    if (s.in_flight) {
      if (wait) {
        if (hipEventSynchronize(s.copied) != hipSuccess) {
          error = "HIP error while waiting for a snapshot";
          return 3;
        }
      } else {
        hipError_t q = hipEventQuery(s.copied);
        if (q == hipErrorNotReady) return 2;
        if (q != hipSuccess) {
          error = "HIP error while polling a snapshot";
          return 3;
        }
      }
      s.in_flight = false;
    }
    *out = s.host.get();
    *n = std::min<uint64_t>(*s.count_host.get(), s.cap);
    if (step_index) *step_index = s.step_index;
    return 0;
  }

  // planners as data
  std::vector<cs_zanlungo_params> lp_params;
  std::vector<uint32_t> lp_kinds;  // 0 NoLocalPlan, 1 Zanlungo, 2 a host LocalPlanner (lp_callbacks)
  struct LpCallback {
    cs_lp_batch_fn fn = nullptr;
    void* user = nullptr;
  };
  std::vector<LpCallback> lp_callbacks;  // by local-planner handle, like lp_params
  bool any_callback_lp = false;          // some group's local planner is host code: evaluated each step (slow path)
  DevBuf<float2> lp_vel;                 // per slot of the sorted arrays: recommended velocity out, the planner's answer in
  std::vector<cs_hlp_desc> hlps;
  std::vector<HostGroup> groups;
  DevBuf<GroupDev> groups_dev;
  bool groups_dirty = true;
  bool any_callback_hlp = false;        // a planner needs set_target / remove events on the host
  bool any_velocity_callback = false;   // a planner is asked for velocities on the host each step
  bool any_route_hlp = false;
  // CS_HLP_FIELD (cs_hlp_field.hip.inc).  On the device a field planner's groups are CS_HLP_CALLBACK groups: the step
  // kernels read pref[i], which k_hlp_field has filled; on the host the planner is a kind of its own and sets none of the
  // flags above.
  std::map<uint32_t, HostHlpField> hlp_fields;  // by planner handle
  DevBuf<HlpFieldDev> hlp_field_tab;            // device, one entry per planner handle
  uint32_t hlp_field_tab_n = 0;                 // entries of it that were uploaded
  bool hlp_fields_dirty = false;     // a field was registered since the table was uploaded
  bool any_field_hlp = false;        // some group's planner is a field: k_hlp_field runs every step
  bool any_silent_callback = false;  // some group's planner is a CS_HLP_CALLBACK without a velocity function (None: its
                                     // slots of pref must read zero, which nothing but k_hlp_field could have changed)
  uint64_t n_hlp_field_launches = 0;  // (CS_STAT_HLP_FIELD_LAUNCHES)
  // CS_HLP_FIELD_TIME=1 (measurement: tools/hlp_field_bench.py): an event either side of every launch of k_hlp_field,
  // read and added up by cs_kernel_stat(CS_STAT_HLP_FIELD_NS); at most 4,096 pairs wait to be read
  bool hlp_field_timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> hlp_field_timed;
  uint64_t hlp_field_ns = 0;
  uint64_t hlp_field_time_read() {
    for (auto& p : hlp_field_timed) {
      float ms = 0.0f;
      if (hipEventSynchronize(p.second) == hipSuccess && hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess)
        hlp_field_ns += (uint64_t)((double)ms * 1e6);
      hipEventDestroy(p.first);
      hipEventDestroy(p.second);
    }
    hlp_field_timed.clear();
    return hlp_field_ns;
  }
  uint64_t hlp_field_bytes() const {
    uint64_t b = hlp_field_tab.bytes();
    for (const auto& kv : hlp_fields) b += (uint64_t)kv.second.d.nx * kv.second.d.ny * sizeof(float2);
    return b;
  }

  // CS_HLP_ROUTE: the route book of RMFPlanner (rmf/mod.rs:83-94).  Routes are planned on the host
  // once per (planner, start hash, goal hash) and live on the device as (first waypoint, count)
  // into a flat f64 array; AgentArrays::route[slot] = (route + 1) | waypoint << 22 is the agent_cache
  // (it travels with the agent, so it costs 4 B per agent SLOT, not per id ever handed out); the
  // book itself is mirrored on the device as a hash table (RouteBookEntry) for the step kernel.
  struct RouteKey {
    uint32_t hlp;
    long long sx, sy, gx, gy;
    bool operator<(const RouteKey& o) const {
      return std::tie(hlp, sx, sy, gx, gy) < std::tie(o.hlp, o.sx, o.sy, o.gx, o.gy);
    }
  };
  std::map<RouteKey, uint32_t> route_by_location;  // route_plans_by_location, rmf/mod.rs:90
  std::vector<uint2> route_desc_host;
  std::vector<double> route_xy_host;
  DevBuf<uint2> route_desc_dev;
  DevBuf<double> route_xy_dev;
  bool routes_dirty = false;
  DevBuf<RouteBookEntry> route_book_dev;
  uint32_t route_book_size = 0;  // slots (a power of two), 0 = no table yet
  DevBuf<double> hlp_scale_dev;
  // tile engines: set_target calls of the last step that missed the route book.  The host merges the
  // misses of all tiles and has every tile plan them in the same order (cs_route_resolve), so that
  // route numbers, which travel in halo records, mean the same thing everywhere.
  std::vector<cs_route_miss> route_misses;
  std::vector<uint2> route_pending;  // (slot in buf[cur], entry) assignments not yet on the device
  uint32_t spawn_first_slot = 0;     // slot of this step's first spawned agent (before the re-sort)
  DevBuf<uint2> route_pending_dev;

  // source-sinks: slot == handle (registry.rs:16-21 hands out ascending integers)
  std::vector<HostSink> sinks;
  DevBuf<SinkDev> sinks_dev;
  DevBuf<double> waypoints_dev;
  DevBuf<uint32_t> src_cell_start, src_sorted, src_occupied, want_dev;
  PinnedBuf<uint32_t> want_host;  // pinned: the H2D copy of a step may still be in flight at return
  DevBuf<uint32_t> spawned_slots_dev;
  DevBuf<uint32_t> spawn_scratch;  // id of the step's first spawn + spawns per block of sinks
  std::vector<uint32_t> want_on_device;  // what want_dev holds
  bool sinks_dirty = true;
  uint32_t n_live_sinks = 0;
  bool spawn_committed = false;          // tile engines: Phase A ran through cs_spawn_probe/commit
  uint32_t committed_spawns = 0;
  uint32_t slots_added = 0;              // tile: slots appended (upper bound) since the last step kernel
  bool spawn_on_device = false;          // ... through cs_spawn_probe_dev/commit_dev: ids are handed out on the device
  uint32_t n_owned_sinks = 0;            // sinks whose source this tile owns (upper bound of its spawns per step)
  DevBuf<SpawnRecord> spawn_rec_dev;
  DevBuf<uint32_t> find_dev;  // cs_remove_agent: (slot, meta) of the id looked up on the device
  DevBytes query_scratch;  // device scratch of the batch spatial queries (grown as needed, never shrunk)
  DevBytes write_scratch;  // device scratch of the by-id calls: cs_write_agents, cs_read_agents_by_id, cs_remove_agents
                           // (grown as needed, never shrunk: cs_agent_write.hip.inc)
  // the selections' view of the planner groups (cs_select.hip.inc): refreshed inside a selection when a group was added
  // since, with a flag of its own, so that a selection leaves groups_dirty and the step's tables alone
  DevBuf<SelGroupDev> sel_groups_dev;
  bool sel_groups_dirty = true;
  // the raster of cs_agent_field (cs_field.hip.inc): grown to the largest raster asked for, never shrunk
  DevBytes field_scratch;
  // the rasters of cs_flow_field_solve (cs_flow_solve.hip.inc): grown to the largest solve asked for, never shrunk
  DevBytes flow_scratch;
  // the lists of cs_close_pairs, cs_agent_clusters and cs_agent_neighbours (PairsScratch, cs_near.hip.inc): kept while
  // they need at most PAIRS_SCRATCH_KEEP bytes; a larger list is allocated for its call and freed before it returns
  DevBytes pairs_scratch;
  DevBuf<int> step_flags_dev;  // cs_tile_step_rccl: the spawn flags of the step
  uint32_t step_colls = 0;        // cs_tile_step_rccl: the collectives its last call issued (bit 0 exchange, bit 1 flags)
  int reserve_step_flags(size_t ns) {
    if (ns <= step_flags_dev.count()) return 0;
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(step_flags_dev.alloc(ns * 2 + 64));
    HIP_OK(hipMemsetAsync(step_flags_dev.get(), 0, step_flags_dev.bytes(), stream));
    return 0;
  }

  uint64_t next_id = 0;  // last_alloc_agent_id, lib.rs:83 (host mirror; the device copy leads while
                         // source-sink steps run without a host sync)
  // CS_CFG_WIDE_IDS: the ids the caller sees are 64-bit EXTERNAL ids; next_id and everything on the device count
  // 32-bit device ids below id_limit, mapped by ext(d) = d < dev_base ? ext_of[d >> 1] : ext_base + (d - dev_base)
  // (cs_kernels_ids.hip.inc).  When the counter would reach id_limit the live agents are renumbered in place
  // (renumber_ids).  Without the flag the table stays empty and dev_base = ext_base = 0: ext(d) = d.
  bool wide_ids = false;
  uint64_t id_limit = CS_ID_LIMIT;  // device ids stay below it (CS_DEVICE_ID_LIMIT lowers it under the flag)
  std::vector<uint64_t> ext_of;     // external ids of the agents alive at the last renumbering, ascending
  uint64_t dev_base = 0, ext_base = 0;
  DevBuf<uint64_t> ext_tab_dev[2];  // [0]: ext_of on the device (k_snapshot), [1]: the next one
  DevBuf<uint32_t> ids_scratch;  // the renumbering's sort: two key arrays, the digit histogram, the live count
  uint64_t n_renumberings = 0;
  uint64_t renumber_ns = 0;  // host wall time inside the renumberings (CS_STAT_RENUMBER_NS)
  uint64_t ext_id(uint64_t d) const {
    if (d < dev_base) return (d >> 1) < ext_of.size() ? ext_of[d >> 1] : UINT64_MAX;
    return ext_base + (d - dev_base);
  }
  // the device id of external id x; false when no live agent can hold it
  bool dev_id(uint64_t x, uint64_t* d) const {
    if (x >= ext_base) {
      if (x - ext_base >= 0xFFFFFFFFull) return false;
      *d = dev_base + (x - ext_base);
      return true;
    }
    const auto it = std::lower_bound(ext_of.begin(), ext_of.end(), x);
    if (it == ext_of.end() || *it != x) return false;
    *d = 2u * (uint64_t)(it - ext_of.begin()) + (x & 1u);
    return true;
  }
  bool counts_stale = false;   // steps ran fire-and-forget since the counters were last read
  bool errors_stale = false;   // ... steps of a plain crowd: counts cannot change, the error state can
  uint32_t async_steps = 0;
  uint32_t want_ring = 0;
  static constexpr uint32_t kWantRing = 16;
  // A tile's slot bound grows by the halo capacities with every exchange.  It is brought down again
  // without waiting and without a call: the step kernel's first thread stores (step number, n_alive)
  // as one 64-bit word into pinned host memory; a later call that finds a newer word takes n_alive
  // of THAT step + the slots appended since as the new bound.  The blocking refresh every
  // kTileAsync steps remains for the error counters (at 4 steps it cost 6 us per step).
  uint32_t kTileAsync = 32;
  static constexpr uint32_t kPeek = 16;
  PinnedBuf<unsigned long long> peek_host;  // pinned; the device writes through the same pointer
  uint64_t peek_mark[kPeek] = {};  // slots_added_total when step (seq % kPeek) was launched
  uint32_t peek_seq = 0, peek_seen = 0;
  uint64_t slots_added_total = 0;  // every slot ever appended to buf[cur] outside the step kernel
  // the step being launched: its number (never 0), remembered with the appends so far
  uint32_t peek_next() {
    ++peek_seq;
    if (peek_seq == 0) ++peek_seq;
    peek_mark[peek_seq % kPeek] = slots_added_total;
    return peek_seq;
  }
  // ... and the host stays at most kFlight steps ahead of the device: before launching a step it
  // waits (on the pinned word, no call into the runtime) until the step kernel launched kFlight
  // steps earlier has STARTED.  The device still has steps queued, so the wait costs it nothing,
  // while the word is never more than kFlight steps old and the bound never more than kFlight + 1
  // exchanges' capacities above the truth.  (An event per step in the stream did the same and cost
  // the stream 4 us per step.)
  static constexpr uint32_t kFlight = 3;
  uint32_t flight_seq[kFlight + 1] = {};  // numbers of the last step kernels launched
  uint32_t flight_n = 0;
  void flight_launched(uint32_t seq) { flight_seq[flight_n++ % (kFlight + 1)] = seq; }
  int flight_throttle() {
    if (!peek_host.get() || flight_n < kFlight) return 0;
    const uint32_t target = flight_seq[(flight_n - kFlight) % (kFlight + 1)];
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; ++spin) {
      const uint32_t seen = (uint32_t)(*reinterpret_cast<volatile unsigned long long*>(peek_host.get()) >> 32);
      if ((int32_t)(seen - target) >= 0) return 0;
      if ((spin & 63u) == 63u) std::this_thread::yield();  // (RCCL's proxy threads and the other ranks want the core too)
      if ((spin & 1023u) == 1023u &&
          std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {  // (a failed launch, a stalled queue)
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
      }
    }
  }
  // takes what has arrived (never waits)
  void peek_poll() {
    if (!peek_host.get()) return;
    const unsigned long long v = *reinterpret_cast<volatile unsigned long long*>(peek_host.get());
    const uint32_t seq = (uint32_t)(v >> 32);
    if (seq == 0 || seq == peek_seen || peek_seq - seq >= kPeek) return;  // nothing new (or too old to have its mark)
    peek_seen = seq;
    const uint64_t bound = (v & 0xFFFFFFFFull) + (slots_added_total - peek_mark[seq % kPeek]);
    if (bound < n_slots) n_slots = (uint32_t)bound;
  }
  // The second pinned word: the cumulative error counters (an agent off the grid, one that outran the border
  // launch of an overlapped step, a dropped band window) as the last step kernel that has STARTED found them, i.e.
  // those of the steps before it.  Non-zero = the next cs_step reads the counters the blocking way and fails
  // (a few steps after the event, where the periodic read alone would take up to kTileAsync steps).
  bool peek_errors() const {
    return peek_host.get() && *reinterpret_cast<volatile unsigned long long*>(peek_host.get() + 1) != 0ull;
  }
  // The third pinned word: Counters::mesh_fail_step as the last step kernel that has started found it (cs_mesh).
  uint32_t peek_mesh_fail() const {
    return peek_host.get() ? (uint32_t)*reinterpret_cast<volatile unsigned long long*>(peek_host.get() + 2) : 0u;
  }
  // CS_CFG_TILE_OVERLAP, how: true (default since round 5) = ONE launch with the border windows first and the exchange of
  // the next step behind a one-wave kernel that waits for them (no split-launch cost: k_step_tiled, TileCfg::split == 2);
  // false (CS_OVERLAP_MODE=split) = rounds 2-4's two launches on two streams
  bool overlap_early = true;
  bool early_pending = false;   // the last step was such a launch: its sequence number is early_seq
  uint32_t early_seq = 0;
  bool no_exchange_ahead = false;  // set by cs_mesh_step for the last step of a run that is about to stop (cs_tile_step_rccl)
  uint32_t mesh_step_tag = 0;  // set by cs_mesh_step before a step of a distributed mesh (k_halo_unpack_all's step_tag)
  uint64_t n_alive_host = 0;
  std::vector<cs_event> events;
  bool record_events = true;

  // per-kernel hipEvent timing
  uint32_t profiling = 0;  // bitmask of CS_K_* kernels to time
  bool prof_open = false;
  struct Timed {
    hipEvent_t a, b;
    uint32_t k;
  };
  std::vector<Timed> timed;
  std::vector<hipEvent_t> event_pool;
  double prof_ms[CS_K_COUNT] = {};
  uint64_t prof_n[CS_K_COUNT] = {};

  // ---- memory ----
  // the agent arrays as the kernels see them: no route column while no route planner exists
  AgentArrays view(int b) const {
    AgentArrays a = buf[b];
    if (!any_route_hlp) a.route = nullptr;
    return a;
  }
  int reserve(uint64_t need) {
    for (int d = 0; d < 4; ++d) need += 2ull * halo[d].cap;  // last step's ghosts + this step's arrivals
    if (need <= cap) return 0;
    uint64_t ncap = std::max<uint64_t>(need, std::max<uint64_t>(1024, cap * 2));
    if (ncap >= 0xFFFFFFF0ull) {
      error = "agent capacity exceeds 32-bit slots";
      return 4;
    }
    HIP_OK(hipStreamSynchronize(stream));
    for (int b = 0; b < 2; ++b) {
      AgentBuf mem;
      HIP_OK(mem.alloc(ncap));
      const AgentArrays na = mem.view();
      if (cap && b == cur && n_slots) {
        HIP_OK(hipMemcpy(na.off, buf[b].off, n_slots * sizeof(float2), hipMemcpyDeviceToDevice));
        HIP_OK(hipMemcpy(na.vel, buf[b].vel, n_slots * sizeof(float2), hipMemcpyDeviceToDevice));
        HIP_OK(hipMemcpy(na.id, buf[b].id, n_slots * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        HIP_OK(hipMemcpy(na.cell, buf[b].cell, n_slots * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        HIP_OK(hipMemcpy(na.meta, buf[b].meta, n_slots * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        HIP_OK(hipMemcpy(na.rank, buf[b].rank, n_slots * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        HIP_OK(hipMemcpy(na.route, buf[b].route, n_slots * sizeof(uint32_t), hipMemcpyDeviceToDevice));
      }
      buf_mem[b] = std::move(mem);  // (frees the old columns)
      buf[b] = na;
    }
    HIP_OK(pref.alloc(ncap));
    HIP_OK(hipMemset(pref.get(), 0, ncap * sizeof(float2)));
    lp_vel.release();  // (allocated by the first step that has a host local planner)
    destroyed_cap = wp_events_cap = 0;
    HIP_OK(destroyed.alloc(ncap));
    destroyed_cap = (uint32_t)ncap;
    HIP_OK(wp_events.alloc(ncap));
    wp_events_cap = (uint32_t)ncap;
    // band windows: at most 2 * agents / tile_target + one per band (the builder keeps every band
    // within that); one-row strips: agents / 256 + one per row
    if (int rc = alloc_window_arrays((uint32_t)(ncap / 32 + ncells / std::max<uint64_t>(nx, 1) + 8))) return rc;
    if (!n_blocks_dev.get()) {
      HIP_OK(n_blocks_dev.alloc(2));  // [0] windows, [1] border windows
      HIP_OK(n_blocks_back.alloc(2));
      HIP_OK(hipMemset(n_blocks_dev.get(), 0, 2 * sizeof(uint32_t)));
      HIP_OK(hipMemset(n_blocks_back.get(), 0, 2 * sizeof(uint32_t)));
    }
    cap = ncap;
    return 0;
  }

  // ---- profiling helpers ----
  hipEvent_t get_event() {
    if (!event_pool.empty()) {
      hipEvent_t e = event_pool.back();
      event_pool.pop_back();
      return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
  }
  uint32_t prof_stride = 1, prof_seen[CS_K_COUNT] = {};
  // a timed region on `on` (default: the engine's stream); returns its handle, or -1 when this launch is not timed.
  // Regions of different kinds may nest (the border / interior launches inside the neighbour pass).
  int prof_open_on(uint32_t k, hipStream_t on) {
    bool want = (profiling >> k) & 1u;
    if (want && prof_stride > 1u) want = (prof_seen[k % CS_K_COUNT]++ % prof_stride) == 0u;
    if (!want) return -1;
    Timed t;
    t.a = get_event();
    t.b = get_event();
    t.k = k;
    hipEventRecord(t.a, on);
    timed.push_back(t);
    return (int)timed.size() - 1;
  }
  void prof_close_on(int handle, hipStream_t on) {
    if (handle >= 0) hipEventRecord(timed[(size_t)handle].b, on);
  }
  int prof_last = -1;
  void prof_begin(uint32_t k) {
    prof_last = prof_open_on(k, stream);
    prof_open = prof_last >= 0;
  }
  void prof_end() {
    if (!prof_open) return;
    prof_open = false;
    prof_close_on(prof_last, stream);
  }
  void prof_collect() {
    if (timed.empty()) return;
    hipStreamSynchronize(stream);
    if (aux_stream) hipStreamSynchronize(aux_stream);
    for (auto& t : timed) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
        prof_ms[t.k] += ms;
        prof_n[t.k] += 1;
      }
      event_pool.push_back(t.a);
      event_pool.push_back(t.b);
    }
    timed.clear();
  }

  // ---- conversions ----
  // location_to_index (location_hash_2d.rs:54-66) in f64, then the offset from
  // the stored cell's geometric origin, rounded once to f32.
  // returns 0 = ok, 1 = "Index out of bounds", 2 = valid but not in this tile's owned cells
  int to_cell(double x, double y, uint32_t* cell, float* ox, float* oy) const {
    uint64_t xi = sat_usize((x - grid.offset_x) / grid.cell_size);
    uint64_t yi = sat_usize((y - grid.offset_y) / grid.cell_size);
    if (!tile) {
      unsigned __int128 idx = (unsigned __int128)xi * nx + yi;
      if (idx >= ncells) return 1;
      uint64_t flat = (uint64_t)idx;
      uint64_t sx = flat / nx, sy = flat % nx;
      *cell = (uint32_t)flat;
      *ox = (float)((x - grid.offset_x) - (double)sx * grid.cell_size);
      *oy = (float)((y - grid.offset_y) - (double)sy * grid.cell_size);
      return 0;
    }
    // The domain's own low edges clamp as in the reference (the saturating cast above: a negative or NaN
    // coordinate lands in row / column 0 and keeps its exact position), so the tile that owns that cell owns the
    // agent.  The alias of y beyond the stride would store the agent in another x row, i.e. on another tile: on a
    // mesh that stays Err, like x beyond the last row.
    if (xi >= gny || yi >= gnx) return 1;
    if (xi < gdev.org_x + gdev.own_x0 || xi >= gdev.org_x + gdev.own_x1 ||
        yi < gdev.org_y + gdev.own_y0 || yi >= gdev.org_y + gdev.own_y1)
      return 2;
    *cell = (uint32_t)((xi - gdev.org_x) * nx + (yi - gdev.org_y));
    *ox = (float)((x - grid.offset_x) - (double)xi * grid.cell_size);
    *oy = (float)((y - grid.offset_y) - (double)yi * grid.cell_size);
    return 0;
  }
  // tile engines: a point of the ghost ring (inside the local grid, owned by another tile)
  bool to_ring_cell(double x, double y, uint32_t* cell, float* ox, float* oy) const {
    if (!tile) return false;
    const uint64_t xi = sat_usize((x - grid.offset_x) / grid.cell_size);
    const uint64_t yi = sat_usize((y - grid.offset_y) / grid.cell_size);
    if (xi >= gny || yi >= gnx) return false;
    if (xi < gdev.org_x || xi >= gdev.org_x + ny || yi < gdev.org_y || yi >= gdev.org_y + nx) return false;
    if (xi >= gdev.org_x + gdev.own_x0 && xi < gdev.org_x + gdev.own_x1 && yi >= gdev.org_y + gdev.own_y0 &&
        yi < gdev.org_y + gdev.own_y1)
      return false;  // owned
    *cell = (uint32_t)((xi - gdev.org_x) * nx + (yi - gdev.org_y));
    *ox = (float)((x - grid.offset_x) - (double)xi * grid.cell_size);
    *oy = (float)((y - grid.offset_y) - (double)yi * grid.cell_size);
    return true;
  }
  void to_global(uint32_t cell, float ox, float oy, double* x, double* y) const {
    uint64_t sx = cell / nx + gdev.org_x, sy = cell % nx + gdev.org_y;
    *x = grid.offset_x + ((double)sx * grid.cell_size + (double)ox);
    *y = grid.offset_y + ((double)sy * grid.cell_size + (double)oy);
  }

  // ---- tables ----
  // One group per add_agents call signature (planners, eyesight) and one per source-sink
  std::map<std::tuple<uint32_t, uint32_t, double>, uint32_t> plain_groups;  // the groups without a sink
  uint32_t make_group(uint32_t hlp, uint32_t lp, double eyesight, int32_t sink) {
    if (sink < 0) {
      auto it = plain_groups.find(std::make_tuple(hlp, lp, eyesight));
      if (it != plain_groups.end()) return it->second;
      plain_groups[std::make_tuple(hlp, lp, eyesight)] = (uint32_t)groups.size();
    }
    groups.push_back(HostGroup{hlp, lp, eyesight, sink});
    groups_dirty = true;
    sel_groups_dirty = true;
    return (uint32_t)groups.size() - 1;
  }
  // Room for one more group (and for a waypoint counter up to n_waypoints): meta holds 65,535 groups and 65,535
  // waypoints (16 / 16 bits) or, once an engine has more groups than that, 1,048,575 groups and 4,095
  // waypoints (20 / 12): the live agents' words are re-packed on the device, halo records packed for the next
  // exchange are void.  Every tile of a mesh registers the same groups in the same order and switches with the
  // same call.
  int room_for_group(size_t n_waypoints) {
    const uint32_t wp_bits = 32u - gdev.grp_bits;
    if (groups.size() + 1 >= (1ull << gdev.grp_bits)) {
      size_t most_wp = n_waypoints;
      for (const HostSink& s : sinks) most_wp = std::max(most_wp, s.waypoints.size() / 2);
      if (gdev.grp_bits != 16u || groups.size() + 1 >= CS_MAX_GROUPS || most_wp > 4095u) {
        error = "too many planner groups: an engine holds 65,535 of them (one per source-sink and per distinct add_agents "
                "signature), or 1,048,575 while no source-sink has more than 4,095 waypoints";
        return 5;
      }
      halo_invalidate();
      HIP_OK(hipStreamSynchronize(stream));
      for (int b = 0; b < 2; ++b)
        if (buf[b].meta && cap)
          hipLaunchKernelGGL(k_repack_meta, dim3((uint32_t)((cap + 255) / 256)), dim3(256), 0, stream, buf[b].meta, (uint32_t)cap,
                             16u, 20u);
      HIP_OK(hipGetLastError());
      HIP_OK(hipStreamSynchronize(stream));
      gdev.grp_bits = 20u;
      epi_valid[0] = epi_valid[1] = false;
      return 0;
    }
    if (n_waypoints >= (1ull << wp_bits)) {
      error = gdev.grp_bits == 16u ? "a source-sink holds at most 65,535 waypoints"
                                   : "a source-sink holds at most 4,095 waypoints on an engine with more than 65,535 planner groups";
      return 5;
    }
    return 0;
  }

  int upload_groups() {
    if (!groups_dirty) return 0;
    std::vector<GroupDev> g(groups.size());
    any_callback_hlp = false;
    any_velocity_callback = false;
    any_route_hlp = false;
    any_callback_lp = false;
    any_field_hlp = false;
    any_silent_callback = false;
    max_eyesight = 0.0;
    for (size_t i = 0; i < groups.size(); ++i) {
      GroupDev& d = g[i];
      d.eyesight = (float)groups[i].eyesight;
      if (lp_kinds[groups[i].lp] == 1u) max_eyesight = std::max(max_eyesight, groups[i].eyesight);
      d.lp_kind = lp_kinds[groups[i].lp];
      if (d.lp_kind == 2u) any_callback_lp = true;
      const cs_zanlungo_params& z = lp_params[groups[i].lp];
      d.A = (float)z.agent_scale;
      d.D = (float)z.force_distance;
      d.inv_mass = 1.0f / (float)z.agent_mass;  // force * (1/m), zanlungo.rs:216
      d.R = (float)z.agent_radius;
      d.vanish2 = zanlungo_vanish2(d.eyesight, d.R, d.D, gdev);
      const cs_hlp_desc& h = hlps[groups[i].hlp];
      d.hlp_kind = h.kind;
      d.hvx = (float)h.vx;
      d.hvy = (float)h.vy;
      d.sink = groups[i].sink;
      d.hlp = groups[i].hlp;
      if (d.sink >= 0 && !sinks[d.sink].alive) d.sink = -1;  // removed sink: no more waypoint tests
      if (h.kind == CS_HLP_CALLBACK) {
        any_callback_hlp = true;
        if (h.velocity) any_velocity_callback = true;
        else any_silent_callback = true;
      }
      if (h.kind == CS_HLP_FIELD) {  // (to the step kernels: a planner whose answers wait in pref)
        d.hlp_kind = CS_HLP_CALLBACK;
        any_field_hlp = true;
      }
      if (h.kind == CS_HLP_ROUTE) {
        d.hvx = (float)h.route_speed;
        d.hvy = (float)h.route_arrive;
        any_route_hlp = true;
        // set_target events reach the host only where the device cannot answer them: the first
        // spawn of a sink (route not planned yet) and waypoint advances (a route from wherever
        // the agent stands)
        const int32_t sk = groups[i].sink;
        if (sk >= 0 && sinks[sk].alive && (sinks[sk].spawn_route == 0 || sinks[sk].waypoints.size() > 2))
          any_callback_hlp = true;
      }
    }
    if (g.size() > groups_dev.count()) {  // (grows by doubling: 200,000 source-sinks are 200,000 groups)
      HIP_OK(hipStreamSynchronize(stream));
      HIP_OK(groups_dev.alloc(std::max<size_t>(1024, 2 * g.size())));
      epi_valid[0] = epi_valid[1] = false;  // (the step kernels' context names the table)
    }
    if (!g.empty())
      HIP_OK(hipMemcpyAsync(groups_dev.get(), g.data(), g.size() * sizeof(GroupDev), hipMemcpyHostToDevice,
                            stream));
    HIP_OK(hipStreamSynchronize(stream));
    groups_dirty = false;
    return 0;
  }

  int upload_sinks() {
    if (!sinks_dirty) return 0;
    HIP_OK(hipStreamSynchronize(stream));
    size_t ns = sinks.size();
    std::vector<SinkDev> sd(ns);
    std::vector<double> wps;
    std::vector<std::pair<uint32_t, uint32_t>> by_cell;  // (cell, slot)
    n_live_sinks = 0;
    for (size_t s = 0; s < ns; ++s) {
      const HostSink& h = sinks[s];
      SinkDev& d = sd[s];
      d.src_x = h.d.source_x;
      d.src_y = h.d.source_y;
      d.src_cell = CS_INVALID_CELL;
      d.ghost_cell = CS_INVALID_CELL;
      d.src_ox = d.src_oy = 0;
      if (h.alive) {
        uint32_t c;
        float ox, oy;
        if (to_cell(h.d.source_x, h.d.source_y, &c, &ox, &oy) == 0) {
          d.src_cell = c;
          d.src_ox = ox;
          d.src_oy = oy;
          by_cell.push_back({c, (uint32_t)s});
        } else if (to_ring_cell(h.d.source_x, h.d.source_y, &c, &ox, &oy)) {
          d.ghost_cell = c;
          d.src_ox = ox;
          d.src_oy = oy;
        }
        ++n_live_sinks;
      }
      d.radius_sink = (float)h.d.radius_sink;
      d.wp_begin = (uint32_t)(wps.size() / 2);
      d.wp_count = (uint32_t)(h.waypoints.size() / 2);
      wps.insert(wps.end(), h.waypoints.begin(), h.waypoints.end());
      d.loop_forever = h.d.loop_forever ? 1u : 0u;
      d.group = h.group;
      d.eyesight = (float)h.d.agent_eyesight_range;
      d.spawn_route = h.spawn_route;
    }
    n_owned_sinks = 0;  // (+ the sources in the ring: their spawns arrive as ghosts)
    for (const SinkDev& d : sd)
      if (d.src_cell != CS_INVALID_CELL || d.ghost_cell != CS_INVALID_CELL) n_owned_sinks += 1;
    sinks_dev.release(); waypoints_dev.release(); src_sorted.release(); src_occupied.release();
    want_dev.release(); spawned_slots_dev.release(); spawn_scratch.release(); want_host.release();
    want_on_device.clear();
    size_t nalloc = std::max<size_t>(ns, 1);
    HIP_OK(sinks_dev.alloc(nalloc));
    HIP_OK(waypoints_dev.alloc(std::max<size_t>(wps.size(), 2)));
    HIP_OK(src_sorted.alloc(nalloc));
    HIP_OK(src_occupied.alloc(nalloc));
    HIP_OK(want_dev.alloc(nalloc));
    HIP_OK(want_host.alloc((size_t)kWantRing * nalloc));
    HIP_OK(spawned_slots_dev.alloc(nalloc));
    HIP_OK(spawn_scratch.alloc(nalloc / SPAWN_BLOCK + 3));
    HIP_OK(hipMemset(src_occupied.get(), 0, nalloc * sizeof(uint32_t)));
    if (ns) HIP_OK(hipMemcpy(sinks_dev.get(), sd.data(), ns * sizeof(SinkDev), hipMemcpyHostToDevice));
    if (!wps.empty())
      HIP_OK(hipMemcpy(waypoints_dev.get(), wps.data(), wps.size() * sizeof(double), hipMemcpyHostToDevice));
    // static source grid: sources sorted by cell + per-cell start
    std::sort(by_cell.begin(), by_cell.end());
    std::vector<uint32_t> start(ncells + 1, 0), sorted_slots(by_cell.size());
    for (auto& bc : by_cell) start[bc.first + 1]++;
    for (uint64_t c = 0; c < ncells; ++c) start[c + 1] += start[c];
    for (size_t k = 0; k < by_cell.size(); ++k) sorted_slots[k] = by_cell[k].second;
    if (!src_cell_start.get()) HIP_OK(src_cell_start.alloc(ncells + 1));
    HIP_OK(hipMemcpy(src_cell_start.get(), start.data(), (ncells + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!sorted_slots.empty())
      HIP_OK(hipMemcpy(src_sorted.get(), sorted_slots.data(), sorted_slots.size() * sizeof(uint32_t),
                       hipMemcpyHostToDevice));
    sinks_dirty = false;
    occ_valid = false;
    groups_dirty = true;  // a removed sink detaches its group
    return 0;
  }

  // ---- histogram of buf[cur] (only when the one kept by the step kernel is stale) ----
  int recount() {
    if (hist_valid) return 0;
    HIP_OK(hipMemsetAsync(cell_count.get(), 0, (ncells + 1) * sizeof(uint32_t), stream));
    if (n_slots)
      hipLaunchKernelGGL(k_count, dim3((n_slots + 255) / 256), dim3(256), 0, stream, buf[cur], 0u,
                         n_slots, cell_count.get(), ctr.get(), gdev.tile);
    HIP_OK(hipGetLastError());
    hist_valid = true;
    return 0;
  }

  // ---- rebuild: histogram (if stale) -> scan -> scatter; leaves buf[cur] sorted ----
  // LDS slots for the staged agents of one window of the tiled kernel: the owned rows' share is
  // `tile_target`, the ghost rows add 2h/rb of that, the 2h halo columns add their cells at the
  // crowd's mean occupancy (wide cells: many agents per halo column)
  uint32_t tile_agents_cap(int h) const {
    const uint32_t rb = tile_rows;
    if (rb <= 1)
      return std::min<uint32_t>(TILE_AGENTS_MAX, ((uint32_t)(2 * h + 1) * TILE_THREADS * 9u / 8u + 192u + tile_agents_slack + 63u) & ~63u);
    const double per_cell = (double)n_slots / (double)std::max<uint64_t>(ncells, 1);
    const double halo_cols = 2.0 * h * per_cell * 1.25;
    const double want = (rb + 2.0 * h) * ((double)tile_target / rb * 9.0 / 8.0 + halo_cols) + 64.0 + tile_agents_slack;
    const uint32_t base = ((rb + 2u * h) * (tile_target / rb) * 9u / 8u + 192u + tile_agents_slack + 63u) & ~63u;
    const uint32_t cap = std::max(base, ((uint32_t)want + 63u) & ~63u);
    return std::min<uint32_t>(TILE_AGENTS_MAX, cap);
  }

  // `bands` > 0: also build the band windows of the tiled kernel in the scatter launch
  bool bands_built = false;
  // The window builder off the critical path (small crowds; round 4).  The builder is a chain of dependent LDS searches
  // per band: ~10 us that a crowd of 125k agents, whose scatter takes 3, waits for in every step before its neighbour
  // kernel can start.  Band windows do not depend on the agents for CORRECTNESS, only for balance, as long as they tile
  // the band's owned cells completely.  So a small crowd steps on the windows of the step BEFORE (`blk_desc`, built in
  // `cover` mode: filler windows over the columns no window owns, a target a little below the workgroup's 256 lanes:
  // room for the agents that walk in within a step), while this step's windows are cut INSIDE the neighbour kernel's
  // launch, by workgroups of their own in front of the windows' (a launch that does not fill the chip has the room),
  // into the other descriptor array (`blk_desc_back`); the two are swapped after the step.  No launch, no stream, no
  // event is added; the scan clears the other array's window count, the scatter launch has no builder blocks.  (A builder
  // on a second stream beside the neighbour kernel was measured first: +10 us per step for the two events and the
  // cross-stream waits; profiles/K4_LEVERS.md.)  A window that outgrows 256 agents is walked in chunks, one that outgrows
  // its LDS tile takes the gather path: slower, never wrong.  Any change of what the windows were cut for (the grid, the
  // tile's rectangle, the eyesight's cells, the descriptor arrays, the LDS budget) builds them in the scatter's launch
  // once, as large crowds do every step.  CS_WINDOWS_KEEP=0 turns it off.
  bool windows_shadow = true;
  uint32_t windows_keep_max_agents = 300000, windows_slack_pct = 10;  // (measured: pays up to ~250k slots, even beyond)
  bool windows_valid = false;
  bool scan_onepass = true;  // CS_SCAN_ONEPASS=0: the two-launch scan
  DevBuf<unsigned long long> scan_tile_sums;
  uint32_t scan_seq = 0;
  uint32_t debug_sort_every = 0, debug_sort_phase = 0, debug_sorted_slots = 0;  // CS_DEBUG_SORT_EVERY (measurement only: rebuild)
  bool debug_sorted_once = false;
  bool debug_ctx_by_value = false;  // CS_DEBUG_CTX_BY_VALUE (measurement only)
  uint32_t scan_ticket_base = 0;  // tickets handed out by all earlier launches of k_scan_onepass (the word behind the sums)
  uint32_t kept_agents_cap = 0;  // the staging slots per window the kept list was cut for (sticky: see step())
  uint32_t windows_bound = 0;  // the most windows the kept arrays can hold: band_windows_max of the step that cut them
  DevBuf<BlockDesc> blk_desc_back;
  DevBuf<uint32_t> n_blocks_back;
  struct WindowsKey {
    uint32_t ncells, nx, own_x0, own_x1, own_y0, own_y1, org_x, org_y, h, desc_cap, rows, target, stage_cap, split;
    const void* desc;
    bool operator==(const WindowsKey& o) const { return std::memcmp(this, &o, sizeof *this) == 0; }
  } windows_key{};
  // (both descriptor arrays, and both window counters, are allocated together)
  int alloc_window_arrays(uint32_t cap_each) {
    blk_desc.release();
    blk_desc_back.release();
    blk_desc_cap = 0;
    windows_valid = false;
    HIP_OK(blk_desc.alloc(cap_each));
    HIP_OK(blk_desc_back.alloc(cap_each));
    blk_desc_cap = cap_each;
    return 0;
  }
  uint64_t n_steps_on_kept_windows = 0;
  // the window counters (both lists) of the list the last step's neighbour kernel walked; null: no tiled step yet
  const uint32_t* last_windows_count = nullptr;
  int windows_listed(uint64_t* out) {
    *out = 0;
    if (!last_windows_count) return 0;
    uint32_t cnt[2] = {0, 0};
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(cnt, last_windows_count, sizeof cnt, hipMemcpyDeviceToHost));
    *out = (uint64_t)cnt[0] + cnt[1];
    return 0;
  }
  // CS_CHECK_WINDOWS=1 (debugging): before the neighbour kernel runs, the band windows it is about to walk are read back
  // and checked on the host: inside the owned rectangle, within the column bound, and (cover mode) tiling every band
  // exactly once.  A bad list fails the step instead of being launched.
  bool check_windows = false;
  std::string check_windows_error;
  int check_window_list(const BlockDesc* list_dev, const uint32_t* count_dev, uint32_t rows, uint32_t n_bands, uint32_t max_cols,
                        bool cover, uint32_t launch_windows) {
    HIP_OK(hipStreamSynchronize(stream));
    uint32_t cnt[2] = {0, 0};
    HIP_OK(hipMemcpy(cnt, count_dev, sizeof cnt, hipMemcpyDeviceToHost));
    char msg[512];
    if (cnt[0] > blk_desc_cap || cnt[0] > launch_windows) {
      std::snprintf(msg, sizeof msg, "window check: %u windows listed, the array holds %u, the launch %u", cnt[0], blk_desc_cap, launch_windows);
      check_windows_error = msg;
      error = check_windows_error.c_str();
      return 7;
    }
    std::vector<BlockDesc> d(cnt[0]);
    if (cnt[0]) HIP_OK(hipMemcpy(d.data(), list_dev, (size_t)cnt[0] * sizeof(BlockDesc), hipMemcpyDeviceToHost));
    const uint32_t ncols = gdev.own_y1 - gdev.own_y0;
    std::vector<std::vector<uint8_t>> seen(n_bands, std::vector<uint8_t>(cover ? ncols : 0u, 0));
    // the slots every window owns, per owned row (a window of whole cells owns its cells' members): they must tile the
    // row's owned slots exactly once
    std::vector<uint32_t> cs((size_t)ncells + 1u);
    HIP_OK(hipMemcpy(cs.data(), cell_start.get(), ((size_t)ncells + 1u) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint32_t own_rows = gdev.own_x1 - gdev.own_x0;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> runs(own_rows);
    for (uint32_t k = 0; k < cnt[0]; ++k) {
      const BlockDesc& w = d[k];
      const bool in_rows = w.row0 >= gdev.own_x0 && w.row0 < gdev.own_x1 && (w.row0 - gdev.own_x0) % rows == 0u && w.nrows >= 1u &&
                           w.nrows <= rows && w.row0 + w.nrows <= gdev.own_x1;
      // (bands wider than the builder's LDS prefix are cut at quantiles of the band's agent count: a window wider than
      // max_cols is allowed there and takes the step kernel's gather path)
      const bool in_cols = w.y0 <= w.y1 && w.y0 >= gdev.own_y0 && w.y1 < gdev.own_y1 &&
                           (w.y1 - w.y0 + 1u <= max_cols || ncols > BAND_LDS_COLS);
      // a window cut at agent granularity: plain lists only, one or two rows, a workgroup's agents at most, each row's
      // slots inside the cells y0 .. y1 of that row, the first and the last of them in columns y0 and y1
      bool cut_ok = w.cut ? (!cover && w.nrows <= 2u && w.count + w.count1 >= 1u && w.count + w.count1 <= (uint32_t)TILE_THREADS &&
                             (w.nrows == 2u || w.count1 == 0u))
                          : (w.count == 0u && w.count1 == 0u);
      if (in_rows && in_cols && cut_ok && w.cut) {
        bool at_y0 = false, at_y1 = false;
        for (uint32_t r = 0; r < w.nrows; ++r) {
          const uint32_t f = r ? w.first1 : w.first, c = r ? w.count1 : w.count;
          if (!c) continue;
          const size_t q = (size_t)(w.row0 + r) * gdev.nx;
          cut_ok = cut_ok && f >= cs[q + w.y0] && f + c <= cs[q + w.y1 + 1u];
          at_y0 = at_y0 || (f < cs[q + w.y0 + 1u]);
          at_y1 = at_y1 || (f + c > cs[q + w.y1]);
        }
        cut_ok = cut_ok && at_y0 && at_y1;
      }
      if (!in_rows || !in_cols || !cut_ok) {
        std::snprintf(msg, sizeof msg, "window check: window %u of %u is {row0 %u nrows %u cut %u y0 %u y1 %u first %u count %u first1 %u count1 %u}; owned rows [%u, %u) columns [%u, %u), %u rows per band, %u columns at most",
                      k, cnt[0], w.row0, (unsigned)w.nrows, (unsigned)w.cut, w.y0, w.y1, w.first, w.count, w.first1, w.count1, gdev.own_x0, gdev.own_x1, gdev.own_y0, gdev.own_y1, rows, max_cols);
        check_windows_error = msg;
        error = check_windows_error.c_str();
        return 7;
      }
      for (uint32_t r = 0; r < w.nrows; ++r) {
        const size_t q = (size_t)(w.row0 + r) * gdev.nx;
        const uint32_t f = w.cut ? (r ? w.first1 : w.first) : cs[q + w.y0];
        const uint32_t c = w.cut ? (r ? w.count1 : w.count) : cs[q + w.y1 + 1u] - f;
        if (c) runs[w.row0 + r - gdev.own_x0].push_back({f, f + c});
      }
      if (cover) {
        std::vector<uint8_t>& band = seen[(w.row0 - gdev.own_x0) / rows];
        for (uint32_t y = w.y0; y <= w.y1; ++y) band[y - gdev.own_y0] += 1;
      }
    }
    // (bands wider than the builder's LDS prefix: windows at quantiles, see above; not checked slot by slot)
    for (uint32_t r = 0; r < own_rows && ncols <= BAND_LDS_COLS; ++r) {
      std::sort(runs[r].begin(), runs[r].end());
      const size_t q = (size_t)(gdev.own_x0 + r) * gdev.nx;
      uint32_t at = cs[q + gdev.own_y0], bad = 0xFFFFFFFFu;
      for (const auto& s : runs[r]) {
        if (s.first != at && bad == 0xFFFFFFFFu) bad = std::min(at, s.first);
        at = s.second;
      }
      if (at != cs[q + gdev.own_y1] && bad == 0xFFFFFFFFu) bad = std::min(at, cs[q + gdev.own_y1]);
      if (bad != 0xFFFFFFFFu) {
        std::snprintf(msg, sizeof msg, "window check: the windows' slots of row %u do not tile its owned slots [%u, %u) exactly once (%zu runs, %u windows; first gap or overlap at slot %u)",
                      gdev.own_x0 + r, cs[q + gdev.own_y0], cs[q + gdev.own_y1], runs[r].size(), cnt[0], bad);
        check_windows_error = msg;
        error = check_windows_error.c_str();
        return 7;
      }
    }
    if (cover)
      for (uint32_t b = 0; b < n_bands; ++b)
        for (uint32_t y = 0; y < ncols; ++y)
          if (seen[b][y] != 1) {
            std::snprintf(msg, sizeof msg, "window check: column %u of band %u is covered %u times (%u windows)", y, b, (unsigned)seen[b][y], cnt[0]);
            check_windows_error = msg;
            error = check_windows_error.c_str();
            return 7;
          }
    return 0;
  }
  // most owned columns a band window may have: the staged tile (2h more columns and an end marker)
  // must fit the fixed-point range of window-relative positions (k_step_tiled: tiled_ok)
  uint32_t tile_max_cols(uint32_t h) const {
    const long long half = (long long)FIX_LIM / std::max(gdev.cs_fix, 1) - 2;  // W1 / 2 + 2 <= FIX_LIM / cs_fix
    const long long cols = 2 * half - 2 * (long long)h - 2;
    return (uint32_t)std::max<long long>(1, std::min<long long>(cols, 4096));
  }
  // CS_CFG_TILE_OVERLAP on a tile with band windows: windows with an owned cell within this many
  // cells of the owned rectangle's edge run as a launch of their own (see build_band).  The halo
  // band reaches halo_cells owned cells inwards and an agent moves less than a cell per step.
  uint32_t split_margin() const {
    const bool wanted = ((flags & CS_CFG_TILE_OVERLAP) && rccl_comm != nullptr) || tile_split_force;
    return (tile && wanted && tile_rows > 1) ? halo_cells + 1u : 0u;
  }
  // keep_windows: the step runs on the band windows of an earlier one (no builder blocks; bands = 0 then);
  // cover / band_target: how the builder cuts (see windows_period)
  int rebuild(uint32_t bands = 0, uint32_t band_rows = 0, uint32_t band_h = 0, uint32_t band_stage_cap = 0,
              bool keep_windows = false, bool cover = false, uint32_t band_target = 0) {
    const bool bands_were_built = bands_built;
    bands_built = false;
    if (sorted) return 0;
    if (int rc = recount()) return rc;
    // MEASUREMENT ONLY (profiles/K4_LEVERS.md, round 5: "a sort kept for k steps"): CS_DEBUG_SORT_EVERY=k skips the
    // scan and the scatter (and the window builder in their launch) on k - 1 of k steps of a plain crowd.  Correct ONLY
    // while no agent changes its cell (the creep scene: the output of a step is then still in cell order and the
    // windows still fit); it prices the most a Verlet-style reuse of the sort could save, nothing else uses it.
    if (debug_sort_every > 1 && !tile && n_live_sinks == 0 && debug_sorted_once && !keep_windows && n_slots == debug_sorted_slots &&
        (++debug_sort_phase % debug_sort_every) != 0) {
      HIP_OK(hipMemsetAsync(cell_count.get(), 0, (size_t)ncells * sizeof(uint32_t), stream));  // (what the scan does while it reads)
      HIP_OK(hipMemsetAsync(&ctr.get()->n_destroyed, 0, 6 * sizeof(uint32_t), stream));        // n_destroyed .. n_wp_events
      bands_built = bands_were_built;
      sorted = true;
      hist_valid = false;
      return 0;
    }
    debug_sorted_once = true;
    debug_sorted_slots = n_slots;
    prof_begin(CS_K_SCAN);
    uint32_t* const scan_clears = (keep_windows || windows_valid) ? n_blocks_back.get() : n_blocks_dev.get();
    if (scan_onepass && n_scan_blocks <= SCAN_ONEPASS_MAX_BLOCKS) {
      if (!scan_tile_sums.get()) {  // (one 64-bit word per tile: sequence number | sum; sequence numbers start at 1; behind
                              //  them the ticket counter)
        HIP_OK(scan_tile_sums.alloc((size_t)SCAN_ONEPASS_MAX_BLOCKS + 1));
        HIP_OK(hipMemsetAsync(scan_tile_sums.get(), 0, ((size_t)SCAN_ONEPASS_MAX_BLOCKS + 1) * sizeof(unsigned long long), stream));
        scan_ticket_base = 0;
      }
      if (++scan_seq == 0u) scan_seq = 1u;
      hipLaunchKernelGGL(k_scan_onepass, dim3(n_scan_blocks), dim3(SCAN_BLOCK), 0, stream, cell_count.get(), (uint32_t)ncells,
                         cell_start.get(), ctr.get(), scan_clears, scan_tile_sums.get(), scan_seq,
                         reinterpret_cast<uint32_t*>(scan_tile_sums.get() + SCAN_ONEPASS_MAX_BLOCKS), scan_ticket_base);
      scan_ticket_base += n_scan_blocks;  // (every workgroup of a launch takes exactly one ticket)
    } else {
      hipLaunchKernelGGL(k_scan_totals, dim3(n_scan_blocks), dim3(SCAN_BLOCK), 0, stream, cell_count.get(),
                         (uint32_t)ncells, block_totals.get());
      hipLaunchKernelGGL(k_scan_bases, dim3(1), dim3(SCAN_BASES_BLOCK), 0, stream, block_totals.get(), n_scan_blocks);
      hipLaunchKernelGGL(k_scan_apply, dim3(n_scan_blocks), dim3(SCAN_BLOCK), 0, stream, cell_count.get(),
                         (uint32_t)ncells, block_totals.get(), cell_start.get(), ctr.get(), scan_clears);
    }
    // (kept windows: the scan clears the counters of the array the builder workgroups of this step fill.  A sort BETWEEN
    // two steps, for a query or a read, must leave the windows the next step will run on alone: windows_valid is still
    // set then, step() clears it before it sorts)
    prof_end();
    prof_begin(CS_K_SCATTER);
    if (n_slots && (bands || keep_windows)) {
      const uint32_t sb = (n_slots + 255) / 256;
      hipLaunchKernelGGL(k_scatter_and_bands, dim3(sb + bands), dim3(256), 0, stream, view(cur), view(cur ^ 1),
                         n_slots, cell_start.get(), bands, gdev, band_rows, band_target ? band_target : tile_target, band_h,
                         band_stage_cap, tile_max_cols(band_h), split_margin(), cover ? 1u : 0u,
                         band_prefix.get(), blk_desc.get(), blk_desc_cap, n_blocks_dev.get(), ctr.get());
      bands_built = true;
    } else if (n_slots) {
      hipLaunchKernelGGL(k_scatter, dim3((n_slots + 255) / 256), dim3(256), 0, stream, view(cur),
                         view(cur ^ 1), n_slots, cell_start.get(), ctr.get(), gdev.tile, (uint32_t)ncells);
    }
    prof_end();
    HIP_OK(hipGetLastError());
    cur ^= 1;
    sorted = true;
    hist_valid = false;  // the scan zeroed cell_count
    return 0;
  }

  int mark_occupancy() {
    if (occ_valid || n_live_sinks == 0) return 0;
    HIP_OK(hipMemsetAsync(src_occupied.get(), 0, std::max<size_t>(sinks.size(), 1) * sizeof(uint32_t), stream));
    if (n_slots)
      hipLaunchKernelGGL(k_mark_sources, dim3((n_slots + 255) / 256), dim3(256), 0, stream, gdev,
                         buf[cur], n_slots, sinks_dev.get(), src_cell_start.get(), src_sorted.get(), src_occupied.get(), ctr.get());
    HIP_OK(hipGetLastError());
    occ_valid = true;
    return 0;
  }

  static constexpr const char* kScanStalled =
      "the one-launch cell scan gave up waiting for an earlier tile's total (k_scan_onepass): the step's sort is void; "
      "CS_SCAN_ONEPASS=0 selects the two-launch scan (please report the device and driver)";
  static constexpr const char* kEarlyStalled =
      "the exchange made ahead gave up waiting for the border windows of its step (k_wait_border): the two streams share a "
      "hardware queue, or the step's launch never ran; CS_OVERLAP_MODE=split selects the two-launch form of the overlap";
  static constexpr const char* kWindowsDropped =
      "the window builder made more band windows than the step kernel's launch was sized for: some agents were not stepped "
      "(band_windows_max is a bound on the builder's output; please report the scene)";
  int read_counters(Counters* out) {
    HIP_OK(hipMemcpyAsync(ctr_host.get(), ctr.get(), sizeof(Counters), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    *out = *ctr_host.get();
    return 0;
  }

  // Steps with source-sinks but nobody listening run fire-and-forget; before the host looks at
  // counts, ids or the error state it catches up here.
  int refresh_counts() {
    if (!counts_stale && !errors_stale) return 0;
    Counters c;
    if (int rc = read_counters(&c)) return rc;
    const bool counts = counts_stale;
    counts_stale = false;
    errors_stale = false;
    async_steps = 0;
    if (c.n_scan_stalled) {  // (before anything else: a void sort explains every other counter)
      poisoned = true;
      error = poison_error = kScanStalled;
      return 7;
    }
    if (c.n_out_of_bounds) {
      poisoned = true;
      error = "Index out of bounds";
      return 1;
    }
    if (c.n_early_stalled) {
      poisoned = true;
      error = poison_error = kEarlyStalled;
      return 7;
    }
    if (c.n_halo_late) {
      poisoned = true;
      error = poison_error = "an agent of an interior window landed in the halo band within one step (it moved more than a cell, or its position became NaN and was binned to cell 0): it would miss the overlapped exchange";
      return 7;
    }
    if (c.n_win_dropped) {
      poisoned = true;
      error = poison_error = kWindowsDropped;
      return 7;
    }
    if (!counts) return 0;
    if (!tile || spawn_on_device) next_id = c.next_id;  // (host-side cs_spawn_commit keeps its own count)
    if (c.n_halo_overflow) {
      poisoned = true;
      error = poison_error = "halo buffer overflow: raise capacity_records of cs_halo_set_buffers";
      return 7;
    }
    // buf[cur] is the output of the last step kernel: one slot per sorted agent, plus what a tile's
    // halo unpack / spawn commit appended since
    n_slots = c.n_alive + (tile ? slots_added : 0u);
    n_alive_host = tile ? (uint64_t)c.n_owned - c.n_destroyed : (uint64_t)c.n_alive - c.n_destroyed;
    return 0;
  }

  // ---- host copy of buf[cur] ----
  struct HostState {
    std::vector<float2> off, vel;
    std::vector<uint32_t> id, cell, meta;
  };
  int download(HostState* h) {
    uint32_t n = n_slots;
    h->off.resize(n); h->vel.resize(n); h->id.resize(n); h->cell.resize(n); h->meta.resize(n);
    if (!n) return 0;
    const AgentArrays& a = buf[cur];
    HIP_OK(hipMemcpyAsync(h->off.data(), a.off, n * sizeof(float2), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(h->vel.data(), a.vel, n * sizeof(float2), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(h->id.data(), a.id, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(h->cell.data(), a.cell, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(h->meta.data(), a.meta, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
  }

  // ---- CS_HLP_ROUTE: RMFPlanner::set_target, rmf/mod.rs:217-236 ----
  // `slot`: where the agent sits in buf[cur] right now (the entry is written there by
  // flush_route_pending before anything reorders the arrays)
  uint32_t route_set_target(uint32_t hlp, uint32_t slot, double px, double py, double tx, double ty) {
    const uint32_t st = route_lookup(hlp, px, py, tx, ty);
    if (st) route_pending.push_back(make_uint2(slot, st));  // (route, waypoint 0)
    return st;
  }
  // the route book alone: find or plan the route of a (start, goal) pair
  uint32_t route_lookup(uint32_t hlp, double px, double py, double tx, double ty) {
    const cs_hlp_desc& p = hlps[hlp];
    if (!p.route_plan) return 0;
    const RouteKey key{hlp, route_spatial_hash(px, p.route_scale), route_spatial_hash(py, p.route_scale),
                       route_spatial_hash(tx, p.route_scale), route_spatial_hash(ty, p.route_scale)};
    uint32_t route;
    auto it = route_by_location.find(key);
    if (it != route_by_location.end()) {
      route = it->second;
    } else {
      double buf[2 * CS_ROUTE_MAX_WAYPOINTS];
      const size_t n = std::min<size_t>(p.route_plan(p.user, px, py, tx, ty, buf, CS_ROUTE_MAX_WAYPOINTS),
                                        CS_ROUTE_MAX_WAYPOINTS);
      if (n == 0) return 0;  // "Failed to find contiguous path": the agent keeps what it had
      route = (uint32_t)route_desc_host.size();
      if (route + 1u >= CS_ROUTE_IDX_MASK) return 0;
      route_desc_host.push_back(make_uint2((uint32_t)(route_xy_host.size() / 2), (uint32_t)n));
      route_xy_host.insert(route_xy_host.end(), buf, buf + 2 * n);
      route_by_location.emplace(key, route);
      routes_dirty = true;
    }
    return route + 1u;
  }
  // halo records carry agent_cache entries: both ends need the same route tables
  int routes_for_halo() {
    if (int rc = upload_groups()) return rc;
    if (!any_route_hlp) return 0;
    return flush_route_tables();
  }
  // Bring the device tables up to date: the routes, the route book (hash table) and the planners'
  // SpatialHash resolutions.  Runs before any kernel that may read them.
  int flush_route_tables() {
    if (hlps.size() > hlp_scale_dev.count() || (any_route_hlp && !hlp_scale_dev.get())) {
      HIP_OK(hipStreamSynchronize(stream));
      HIP_OK(hlp_scale_dev.alloc(hlps.size() * 2 + 8));
      routes_dirty = true;
    }
    if (!routes_dirty) return 0;
    HIP_OK(hipStreamSynchronize(stream));  // a kernel in flight may still read the old tables
    {
      std::vector<double> scale(hlps.size(), 1.0);
      for (size_t k = 0; k < hlps.size(); ++k)
        if (hlps[k].kind == CS_HLP_ROUTE) scale[k] = hlps[k].route_scale;
      if (!scale.empty())
        HIP_OK(hipMemcpy(hlp_scale_dev.get(), scale.data(), scale.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (route_desc_host.size() > route_desc_dev.count()) HIP_OK(route_desc_dev.alloc(route_desc_host.size() * 2));
    if (route_xy_host.size() > route_xy_dev.count()) HIP_OK(route_xy_dev.alloc(route_xy_host.size() * 2));
    if (!route_desc_host.empty()) {
      HIP_OK(hipMemcpy(route_desc_dev.get(), route_desc_host.data(), route_desc_host.size() * sizeof(uint2),
                       hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(route_xy_dev.get(), route_xy_host.data(), route_xy_host.size() * sizeof(double),
                       hipMemcpyHostToDevice));
    }
    // the route book as an open-addressing table, at most half full
    uint32_t want = 64;
    while (want < 2u * route_by_location.size() + 2u) want <<= 1;
    if (want != route_book_size) {
      route_book_size = 0;
      HIP_OK(route_book_dev.alloc(want));
      route_book_size = want;
    }
    std::vector<RouteBookEntry> table(route_book_size, RouteBookEntry{0, 0, 0, 0, 0u, 0u});
    for (const auto& kv : route_by_location) {
      const RouteKey& key = kv.first;
      uint32_t k = route_book_slot(key.hlp, key.sx, key.sy, key.gx, key.gy) & (route_book_size - 1u);
      while (table[k].route1 != 0u) k = (k + 1u) & (route_book_size - 1u);
      table[k] = RouteBookEntry{key.sx, key.sy, key.gx, key.gy, key.hlp, kv.second + 1u};
    }
    HIP_OK(hipMemcpy(route_book_dev.get(), table.data(), table.size() * sizeof(RouteBookEntry), hipMemcpyHostToDevice));
    routes_dirty = false;
    return 0;
  }
  // Write the agent_cache entries the host decided on into buf[cur] (by slot).  Must run before
  // anything reorders the arrays: right after the events that produced them were handled.
  int flush_route_pending() {
    if (route_pending.empty()) return 0;
    if (route_pending.size() > route_pending_dev.count()) {
      HIP_OK(hipStreamSynchronize(stream));
      HIP_OK(route_pending_dev.alloc(route_pending.size() * 2));
    }
    HIP_OK(hipMemcpy(route_pending_dev.get(), route_pending.data(), route_pending.size() * sizeof(uint2),
                     hipMemcpyHostToDevice));
    const uint32_t m = (uint32_t)route_pending.size();
    hipLaunchKernelGGL(k_route_assign, dim3((m + 255u) / 256u), dim3(256), 0, stream, buf[cur].route, n_slots,
                       route_pending_dev.get(), m);
    HIP_OK(hipGetLastError());
    route_pending.clear();
    return 0;
  }

  // ---- callback high-level planners: the documented slow path ----
  // get_desired_velocity for every agent of a CALLBACK planner, batched per
  // planner, on the sorted state (lib.rs:264-273).
  int eval_callback_hlps() {
    HostState h;
    if (int rc = download(&h)) return rc;
    uint32_t n = n_slots;
    std::vector<float2> pv(n, make_float2(0.f, 0.f));
    for (uint32_t p = 0; p < hlps.size(); ++p) {
      if (hlps[p].kind != CS_HLP_CALLBACK || !hlps[p].velocity) continue;
      std::vector<uint32_t> slots;
      for (uint32_t i = 0; i < n; ++i)
        if (h.cell[i] != CS_INVALID_CELL && groups[meta_group(gdev, h.meta[i])].hlp == p) slots.push_back(i);
      if (slots.empty()) continue;
      size_t m = slots.size();
      std::vector<uint64_t> ids(m);
      std::vector<double> pos(2 * m), vel(2 * m), out(2 * m, 0.0);
      std::vector<uint8_t> some(m, 0);
      for (size_t k = 0; k < m; ++k) {
        uint32_t i = slots[k];
        ids[k] = ext_id(h.id[i]);
        to_global(h.cell[i], h.off[i].x, h.off[i].y, &pos[2 * k], &pos[2 * k + 1]);
        vel[2 * k] = h.vel[i].x;
        vel[2 * k + 1] = h.vel[i].y;
      }
      hlps[p].velocity(hlps[p].user, m, ids.data(), pos.data(), vel.data(), 0.0, out.data(), some.data());
      for (size_t k = 0; k < m; ++k)
        if (some[k]) pv[slots[k]] = make_float2((float)out[2 * k], (float)out[2 * k + 1]);
    }
    if (n) {
      HIP_OK(hipMemcpyAsync(pref.get(), pv.data(), n * sizeof(float2), hipMemcpyHostToDevice, stream));
      HIP_OK(hipStreamSynchronize(stream));
    }
    return 0;
  }

  // ---- CS_CFG_WIDE_IDS: room for the next allocation ----
  // n_new ids are about to be handed out, `in_flight` more may have been by steps still running on the device.  Without
  // the flag the id space simply ends; with it the live agents are renumbered (renumber_ids), and only a crowd whose 2L
  // device ids plus this allocation do not fit is refused.
  int ids_room(uint64_t n_new, uint64_t in_flight) {
    if (next_id + in_flight + n_new < id_limit) return 0;
    if (!wide_ids) {
      error = "agent id space exhausted (device ids are 31-bit)";
      return 4;
    }
    if (int rc = refresh_counts()) return rc;  // the steps in flight
    if (next_id + n_new < id_limit) return 0;
    if (tile) {  // every tile of a mesh must agree on the new numbering: the mesh renumbers (mesh_ids_room) before this
      error = "agent id space exhausted: a tile engine renumbers only through its mesh (cs_mesh_*)";
      return 4;
    }
    const uint64_t live = n_alive_host;
    if (2u * live + 1u + n_new >= id_limit) {
      error = "agent id space exhausted: " + std::to_string(live) + " live agents need " + std::to_string(2u * live + 1u) +
              " device ids after a renumbering, and this allocation " + std::to_string(n_new) +
              " more; the device id limit is " + std::to_string(id_limit);
      return 4;
    }
    return renumber_ids();
  }

  // Renumber the live agents in place: rank r (ascending device id) gets 2r + parity; ext_of becomes their external ids.
  // Gather, radix sort and rewrite run on the device; the new table comes to the host once.
  int renumber_ids() {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_OK(hipStreamSynchronize(stream));
    const uint32_t n = n_slots;
    const size_t tiles_max = (n + IDS_TILE - 1u) / IDS_TILE;
    const size_t words = 2u * (size_t)n + IDS_RADIX * tiles_max + 1u;
    if (words > ids_scratch.count()) HIP_OK(ids_scratch.alloc(words));
    uint32_t* keys = ids_scratch.get();
    uint32_t* other = keys + n;
    uint32_t* hist = other + n;
    uint32_t* count_dev = hist + IDS_RADIX * tiles_max;
    uint32_t n_live = 0;
    if (n) {
      HIP_OK(hipMemsetAsync(count_dev, 0, sizeof(uint32_t), stream));
      hipLaunchKernelGGL(k_ids_gather, dim3((n + 255u) / 256u), dim3(256), 0, stream, buf[cur], n, keys, count_dev);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(&n_live, count_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      HIP_OK(hipStreamSynchronize(stream));
    }
    if (n_live > n) {
      error = "renumbering agent ids: the live count exceeds the slots";
      return 90;
    }
    if (n_live) {
      const uint32_t tiles = (n_live + IDS_TILE - 1u) / IDS_TILE;
      const uint32_t bits = next_id > 1 ? 64u - (uint32_t)__builtin_clzll(next_id - 1) : 1u;  // every id < next_id
      for (uint32_t shift = 0; shift < bits; shift += 4u) {
        hipLaunchKernelGGL(k_ids_hist, dim3(tiles), dim3(IDS_BLOCK), 0, stream, keys, n_live, shift, hist, tiles);
        hipLaunchKernelGGL(k_ids_scan, dim3(1), dim3(IDS_BLOCK), 0, stream, hist, IDS_RADIX * tiles);
        hipLaunchKernelGGL(k_ids_scatter, dim3(tiles), dim3(IDS_BLOCK), 0, stream, keys, other, n_live, shift, hist, tiles);
        std::swap(keys, other);
      }
      if (ext_tab_dev[1].count() < n_live) HIP_OK(ext_tab_dev[1].alloc(n_live));
      hipLaunchKernelGGL(k_ids_renumber, dim3((n + 255u) / 256u), dim3(256), 0, stream, buf[cur], n, keys, n_live);
      hipLaunchKernelGGL(k_ids_table, dim3((n_live + 255u) / 256u), dim3(256), 0, stream, keys, n_live, ext_tab_dev[0].get(),
                         (uint32_t)ext_of.size(), (uint32_t)dev_base, ext_base, ext_tab_dev[1].get());
      HIP_OK(hipGetLastError());
    }
    std::vector<uint64_t> tab(n_live);
    if (n_live)
      HIP_OK(hipMemcpyAsync(tab.data(), ext_tab_dev[1].get(), (size_t)n_live * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    const uint64_t next_ext = ext_id(next_id);  // what the next allocation would have been called
    ext_of.swap(tab);
    std::swap(ext_tab_dev[0], ext_tab_dev[1]);
    ext_base = next_ext;
    dev_base = 2u * (uint64_t)n_live + ((2u * (uint64_t)n_live ^ ext_base) & 1u);
    next_id = dev_base;
    const uint32_t nid = (uint32_t)next_id;
    HIP_OK(hipMemcpy(&ctr.get()->next_id, &nid, sizeof nid, hipMemcpyHostToDevice));
    halo_invalidate();
    ++n_renumberings;
    renumber_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    return 0;
  }

  // ---- a mesh's renumbering, in two halves around the gather of the mesh (cs_mesh.hip.inc: mesh_ids_room) ----
  // 1. this tile's live agents' external ids, ascending (no ghosts may be present: between two mesh steps a tile holds
  //    exactly the agents it stepped, each agent is held by one tile)
  // the device counter, exactly (a tile hands out ids on the device without the host: cs_spawn_commit_dev)
  int sync_next_id() {
    if (int rc = refresh_counts()) return rc;
    if (aux_stream) HIP_OK(hipStreamSynchronize(aux_stream));  // (an exchange made ahead)
    Counters c;
    if (int rc = read_counters(&c)) return rc;
    next_id = c.next_id;
    return 0;
  }
  int wide_owned_ext(std::vector<uint64_t>* out) {
    if (int rc = sync_next_id()) return rc;
    if (ghosts_present) {
      error = "renumbering agent ids: the tile holds ghosts (only between two mesh steps)";
      return 90;
    }
    const uint32_t n = n_slots;
    const size_t tiles_max = (n + IDS_TILE - 1u) / IDS_TILE;
    const size_t words = 2u * (size_t)n + IDS_RADIX * tiles_max + 1u;
    if (words > ids_scratch.count()) HIP_OK(ids_scratch.alloc(words));
    uint32_t* keys = ids_scratch.get();
    uint32_t* other = keys + n;
    uint32_t* hist = other + n;
    uint32_t* count_dev = hist + IDS_RADIX * tiles_max;
    uint32_t n_live = 0;
    if (n) {
      HIP_OK(hipMemsetAsync(count_dev, 0, sizeof(uint32_t), stream));
      hipLaunchKernelGGL(k_ids_gather, dim3((n + 255u) / 256u), dim3(256), 0, stream, buf[cur], n, keys, count_dev);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(&n_live, count_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      HIP_OK(hipStreamSynchronize(stream));
    }
    if (n_live > n) {
      error = "renumbering agent ids: the live count exceeds the slots";
      return 90;
    }
    out->assign(n_live, 0);
    if (!n_live) return 0;
    const uint32_t tiles = (n_live + IDS_TILE - 1u) / IDS_TILE;
    const uint32_t bits = next_id > 1 ? 64u - (uint32_t)__builtin_clzll(next_id - 1) : 1u;
    for (uint32_t shift = 0; shift < bits; shift += 4u) {
      hipLaunchKernelGGL(k_ids_hist, dim3(tiles), dim3(IDS_BLOCK), 0, stream, keys, n_live, shift, hist, tiles);
      hipLaunchKernelGGL(k_ids_scan, dim3(1), dim3(IDS_BLOCK), 0, stream, hist, IDS_RADIX * tiles);
      hipLaunchKernelGGL(k_ids_scatter, dim3(tiles), dim3(IDS_BLOCK), 0, stream, keys, other, n_live, shift, hist, tiles);
      std::swap(keys, other);
    }
    if (int rc = ext_tab_reserve(1, n_live)) return rc;
    hipLaunchKernelGGL(k_ids_table, dim3((n_live + 255u) / 256u), dim3(256), 0, stream, keys, n_live, ext_tab_dev[0].get(),
                       (uint32_t)ext_of.size(), (uint32_t)dev_base, ext_base, ext_tab_dev[1].get());
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(out->data(), ext_tab_dev[1].get(), (size_t)n_live * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
  }
  // 2. the mesh-wide table (ascending external ids of every live agent of the mesh, the same on every tile): every live
  //    agent here takes 2 * (its rank in it) + parity; new ids continue from 2L with the parity of next_ext
  int wide_apply_table(const std::vector<uint64_t>& all, uint64_t next_ext) {
    const uint32_t L = (uint32_t)all.size();
    if (int rc = ext_tab_reserve(1, L)) return rc;
    if (L) HIP_OK(hipMemcpyAsync(ext_tab_dev[1].get(), all.data(), (size_t)L * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    if (n_slots && L)
      hipLaunchKernelGGL(k_ids_renumber_ext, dim3((n_slots + 255u) / 256u), dim3(256), 0, stream, buf[cur], n_slots,
                         ext_tab_dev[0].get(), (uint32_t)ext_of.size(), (uint32_t)dev_base, ext_base, ext_tab_dev[1].get(), L);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(stream));
    ext_of = all;
    std::swap(ext_tab_dev[0], ext_tab_dev[1]);
    ext_base = next_ext;
    dev_base = 2u * (uint64_t)L + ((2u * (uint64_t)L ^ ext_base) & 1u);
    next_id = dev_base;
    const uint32_t nid = (uint32_t)next_id;
    HIP_OK(hipMemcpy(&ctr.get()->next_id, &nid, sizeof nid, hipMemcpyHostToDevice));
    halo_invalidate();
    ++n_renumberings;
    return 0;
  }
  int ext_tab_reserve(int k, uint32_t n) {
    if (ext_tab_dev[k].count() >= n) return 0;
    HIP_OK(ext_tab_dev[k].alloc(std::max<uint32_t>(n, 1u)));
    return 0;
  }

  // ---- Simulation::add_agents, lib.rs:119-156 ----
  int add_agents(const double* xy, size_t n, uint32_t group, uint32_t owner, uint64_t* out_ids) {
    halo_invalidate();  // on every tile alike, whether or not it keeps any of them (exchange made ahead)
    last_failed_add_id = UINT64_MAX;
    last_failed_add_index = SIZE_MAX;
    if (n == 0) return 0;
    if (int rc = refresh_counts()) return rc;
    if (int rc = ids_room(n, 0)) return rc;
    if (int rc = reserve((uint64_t)n_slots + n)) return rc;
    std::vector<float2> off, vel;
    std::vector<uint32_t> ids, cells, meta;
    off.reserve(n); ids.reserve(n); cells.reserve(n);
    int rc = 0;
    for (size_t k = 0; k < n; ++k) {
      uint32_t c;
      float ox, oy;
      const uint64_t dev = next_id++;  // consumed even when the insert fails (lib.rs:128-129)
      const uint64_t id = ext_id(dev);
      int where = to_cell(xy[2 * k], xy[2 * k + 1], &c, &ox, &oy);
      if (where == 1) {
        // The reference has already put the agent into `agents` when the index insert
        // fails (lib.rs:133-149): it stays, outside the index (`limbo`), and the same error is reported.
        if (!tile) limbo.push_back(LimboAgent{id, xy[2 * k], xy[2 * k + 1], group});
        last_failed_add_id = id;
        last_failed_add_index = k;
        error = "Index out of bounds";
        rc = 1;
        break;
      }
      if (out_ids) out_ids[k] = id;
      if (where == 2) continue;  // another tile owns it
      off.push_back(make_float2(ox, oy));
      ids.push_back((uint32_t)dev);
      cells.push_back(c);
      cs_event ev;
      ev.kind = CS_EVENT_SPAWNED;
      ev.source_sink = owner;
      ev.id = id;
      ev.x = xy[2 * k];
      ev.y = xy[2 * k + 1];
      if (record_events) events.push_back(ev);
    }
    const size_t ok = ids.size();
    vel.assign(ok, make_float2(0.f, 0.f));
    meta.assign(ok, group);
    if (ok) {
      AgentArrays& a = buf[cur];
      uint32_t at = n_slots;
      HIP_OK(hipMemcpyAsync(a.off + at, off.data(), ok * sizeof(float2), hipMemcpyHostToDevice, stream));
      HIP_OK(hipMemcpyAsync(a.vel + at, vel.data(), ok * sizeof(float2), hipMemcpyHostToDevice, stream));
      HIP_OK(hipMemcpyAsync(a.id + at, ids.data(), ok * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
      HIP_OK(hipMemcpyAsync(a.cell + at, cells.data(), ok * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
      HIP_OK(hipMemcpyAsync(a.meta + at, meta.data(), ok * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
      HIP_OK(hipMemsetAsync(a.route + at, 0, ok * sizeof(uint32_t), stream));  // no agent_cache entry yet
      HIP_OK(hipStreamSynchronize(stream));  // the host vectors die at return
      n_slots += (uint32_t)ok;
      slots_added_total += ok;
      n_alive_host += ok;
      sorted = false;
      hist_valid = false;
      occ_valid = false;
      halo_invalidate();
      HIP_OK(hipMemcpy(&ctr.get()->n_pending, &n_slots, sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    {
      uint32_t nid = (uint32_t)next_id;
      HIP_OK(hipMemcpy(&ctr.get()->next_id, &nid, sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return rc;
  }

  // CrowdGenerator::get_number_to_spawn for every live sink, ascending handle (lib.rs:199-222);
  // want[s] = 1 iff the generator asked for at least one agent.  Returns the number of 1s.
  uint32_t eval_generators(double dt_seconds, uint32_t* want) {
    uint32_t n_want = 0;
    for (size_t s = 0; s < sinks.size(); ++s) {
      HostSink& h = sinks[s];
      want[s] = 0;
      if (!h.alive) continue;
      uint64_t call = h.calls++;
      uint64_t nsp = 0;
      switch (h.d.generator_kind) {
        case CS_GEN_MONOTONIC: {  // (dt * rate).round() as usize, source_sink.rs:96-100
          double v = std::round(dt_seconds * h.d.rate);
          nsp = v > 0 ? (uint64_t)v : 0;
          break;
        }
        case CS_GEN_POISSON_SEEDED:
          nsp = poisson_seeded(h.d.seed, call, dt_seconds * h.d.rate);
          break;
        case CS_GEN_CALLBACK:
          nsp = h.d.generator ? (uint64_t)h.d.generator(h.d.generator_user, dt_seconds) : 0;
          break;
      }
      want[s] = nsp > 0 ? 1u : 0u;  // the loop over n is commented out (lib.rs:207)
      n_want += want[s];
    }
    return n_want;
  }

  // ---- tile engines: Phase A split in two so that ids follow the GLOBAL sink order ----
  // probe: flags[s] = 1 iff sink s is owned by this tile, its generator fired and nobody (owned
  // agent or ghost) stands within 0.4 of its source.
  int spawn_probe(double dt_seconds, uint8_t* flags) {
    if (spawn_on_device) {
      // ids were handed out on the device since the last sync: fetch the counter.  Not
      // refresh_counts(): the halo unpack of this step has already appended to the slot count.
      Counters c;
      if (int rc = read_counters(&c)) return rc;
      next_id = c.next_id;
    }
    if (int rc = upload_sinks()) return rc;
    if (int rc = upload_groups()) return rc;
    std::memset(flags, 0, sinks.size());
    uint32_t n_want = eval_generators(dt_seconds, want_host.get());
    if (!n_want) return 0;
    occ_valid = false;  // ghosts arrived since the step kernel marked its own agents
    if (int rc = mark_occupancy()) return rc;
    std::vector<uint32_t> occ(sinks.size());
    HIP_OK(hipMemcpyAsync(occ.data(), src_occupied.get(), sinks.size() * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          stream));
    HIP_OK(hipStreamSynchronize(stream));
    std::vector<SinkDev> dummy;
    for (size_t s = 0; s < sinks.size(); ++s) {
      if (!want_host.get()[s] || occ[s]) continue;
      uint32_t c;
      float ox, oy;
      if (to_cell(sinks[s].d.source_x, sinks[s].d.source_y, &c, &ox, &oy) == 0) flags[s] = 1;
    }
    return 0;
  }
  // commit: `flags` is the OR over all tiles.  Ids are next_id + rank in ascending handle order;
  // this tile appends the agents of the sinks it owns.
  int spawn_commit(const uint8_t* flags) {
    std::vector<SpawnRecord> mine;
    uint32_t n_ghost_spawns = 0;
    uint64_t id = next_id;
    for (size_t s = 0; s < sinks.size(); ++s) {
      if (!flags[s]) continue;
      const uint64_t my_id = id++;
      uint32_t c;
      float ox, oy;
      if (to_cell(sinks[s].d.source_x, sinks[s].d.source_y, &c, &ox, &oy) != 0) {
        // another tile's spawn inside my ring: a ghost for this step (see SinkDev.ghost_cell)
        if (my_id < id_limit && to_ring_cell(sinks[s].d.source_x, sinks[s].d.source_y, &c, &ox, &oy)) {
          mine.push_back(SpawnRecord{ox, oy, (uint32_t)my_id, c, sinks[s].group, sinks[s].spawn_route});
          ++n_ghost_spawns;
        }
        continue;
      }
      if (my_id >= id_limit) {
        error = "agent id space exhausted (device ids are 31-bit)";
        return 4;
      }
      mine.push_back(SpawnRecord{ox, oy, (uint32_t)my_id, c, sinks[s].group, sinks[s].spawn_route});
      if (record_events) {
        cs_event ev;
        ev.kind = CS_EVENT_SPAWNED;
        ev.source_sink = (uint32_t)s;
        ev.id = ext_id(my_id);
        ev.x = sinks[s].d.source_x;
        ev.y = sinks[s].d.source_y;
        events.push_back(ev);
      }
      const cs_hlp_desc& p = hlps[sinks[s].d.hlp];
      if (p.kind == CS_HLP_CALLBACK && p.set_target && !sinks[s].waypoints.empty())
        p.set_target(p.user, ext_id(my_id), sinks[s].d.source_x, sinks[s].d.source_y, sinks[s].waypoints[0],
                     sinks[s].waypoints[1], sinks[s].d.radius_sink, sinks[s].d.radius_sink);
    }
    next_id = id;
    {
      const uint32_t nid = (uint32_t)next_id;  // the device path (cs_spawn_commit_dev) continues from here
      HIP_OK(hipMemcpyAsync(&ctr.get()->next_id, &nid, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
      HIP_OK(hipStreamSynchronize(stream));
    }
    committed_spawns = (uint32_t)mine.size() - n_ghost_spawns;
    spawn_committed = true;
    spawn_on_device = false;
    if (mine.empty()) return 0;
    if (int rc = recount()) return rc;
    if (int rc = reserve((uint64_t)n_slots + mine.size())) return rc;
    if (mine.size() > spawn_rec_dev.count()) HIP_OK(spawn_rec_dev.alloc((uint32_t)mine.size() * 2u + 64u));
    HIP_OK(hipMemcpyAsync(spawn_rec_dev.get(), mine.data(), mine.size() * sizeof(SpawnRecord),
                          hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_append_spawns, dim3(((uint32_t)mine.size() + 255) / 256), dim3(256), 0, stream,
                       view(cur), (uint32_t)cap, spawn_rec_dev.get(), (uint32_t)mine.size(), cell_count.get(), ctr.get());
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(stream));  // `mine` dies at return
    n_slots += (uint32_t)mine.size();
    slots_added += (uint32_t)mine.size();
    slots_added_total += mine.size();
    if (n_ghost_spawns) ghosts_present = true;
    sorted = false;
    return 0;
  }

  // Phase A on a tile without the host: see k_spawn_probe_dev.  `flags_dev`: one int per sink.
  uint32_t pending_want = 0;
  int spawn_probe_dev(double dt_seconds, int* flags_dev) {
    if (int rc = upload_sinks()) return rc;
    if (int rc = upload_groups()) return rc;
    uint32_t* want = want_host.get() + (size_t)want_ring * std::max<size_t>(sinks.size(), 1);
    want_ring = (want_ring + 1) % kWantRing;
    pending_want = eval_generators(dt_seconds, want);
    if (want_on_device.size() != sinks.size() ||
        std::memcmp(want_on_device.data(), want, sinks.size() * sizeof(uint32_t)) != 0) {
      HIP_OK(hipMemcpyAsync(want_dev.get(), want, sinks.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
      want_on_device.assign(want, want + sinks.size());
    }
    occ_valid = false;  // ghosts arrived since the step kernel marked its own agents
    if (int rc = mark_occupancy()) return rc;
    const uint32_t ns = (uint32_t)sinks.size();
    if (ns)
      hipLaunchKernelGGL(k_spawn_probe_dev, dim3((ns + 255u) / 256u), dim3(256), 0, stream, sinks_dev.get(), want_dev.get(), ns,
                         src_occupied.get(), flags_dev);
    HIP_OK(hipGetLastError());
    return 0;
  }
  int spawn_commit_dev(const int* flags_dev) {
    const uint32_t ns = (uint32_t)sinks.size();
    spawn_committed = true;
    spawn_on_device = true;
    committed_spawns = 0;
    if (!ns || !pending_want) return 0;
    if (next_id + (uint64_t)(async_steps + 1) * ns >= id_limit) {
      error = "agent id space exhausted (device ids are 31-bit)";
      return 4;
    }
    if (int rc = recount()) return rc;
    if (int rc = routes_for_halo()) return rc;
    const uint32_t mine = std::min(n_owned_sinks, pending_want);
    if (int rc = reserve((uint64_t)n_slots + mine)) return rc;
    const uint32_t nb = (ns + SPAWN_BLOCK - 1u) / SPAWN_BLOCK;
    prof_begin(CS_K_SPAWN);
    hipLaunchKernelGGL(k_spawn_count_flags, dim3(nb), dim3(SPAWN_BLOCK), 0, stream, flags_dev, ns, ctr.get(),
                       spawn_scratch.get());
    hipLaunchKernelGGL(k_spawn_commit_dev, dim3(nb), dim3(SPAWN_BLOCK), 0, stream, view(cur), (uint32_t)cap,
                       sinks_dev.get(), flags_dev, ns, cell_count.get(), ctr.get(), spawn_scratch.get());
    prof_end();
    HIP_OK(hipGetLastError());
    n_slots += mine;  // upper bound; kernels stop at the device-side count
    slots_added += mine;
    slots_added_total += mine;
    ghosts_present = true;  // (sources in the ring spawn ghosts)
    sorted = false;
    return 0;
  }

  // ---- Simulation::step, lib.rs:195-383 ----
  int step(double dt_seconds, cs_step_report* report) {
    border_on_aux = false;  // (set again below only if THIS step's border launch goes to the second stream)
    if (tile)
      if (int rc = flight_throttle()) return rc;
    peek_poll();
    if (poisoned) {
      error = poison_error;
      return 1;
    }
    if (int rc = upload_sinks()) return rc;
    if (int rc = upload_groups()) return rc;
    const bool has_sinks = n_live_sinks > 0;
    if (tile && has_sinks && !spawn_committed) {
      error = "tile engine with source-sinks: run cs_spawn_probe / cs_spawn_commit before cs_step";
      return 6;
    }
    // a tile's slot count changes with every halo exchange: the host re-reads it each step
    // lib.rs:299-302: the update loop fails on an agent the index never took (`limbo`).  The spawn phase has run by
    // then (lib.rs:199-254) and its agents stay, so the step is taken as usual and fails where an agent that left
    // the grid fails it: nothing of phase B is committed, this step's spawns are.
    const bool limbo_fail = !limbo.empty();
    const bool need_host = has_sinks || any_callback_hlp || any_callback_lp || report != nullptr || tile || limbo_fail;

    bool spawn_ran = false;  // the spawn kernels reset n_spawned and the occupancy marks themselves

    // ---- Phase A: spawn (lib.rs:199-254) ----
    uint32_t n_want = 0;
    bool spawn_events_done = false;
    // nobody needs the host this step: source-sinks without listeners / host planners / report
    // ... or a tile without source-sinks: its slot count (owned + ghosts) stays a host-side upper
    // bound for a few steps; every kernel stops at the device-side count
    const bool fire_and_forget =
        !limbo_fail && !record_events && !any_callback_hlp && !any_callback_lp && report == nullptr && !peek_errors() &&
        ((has_sinks && !tile && async_steps + 1 < kWantRing) ||
         (tile && (!has_sinks || spawn_on_device) && async_steps + 1 < kTileAsync));
    if (has_sinks && !tile) {
      uint32_t* want = want_host.get() + (size_t)want_ring * std::max<size_t>(sinks.size(), 1);
      want_ring = (want_ring + 1) % kWantRing;  // a slot is reused only after a host sync
      n_want = eval_generators(dt_seconds, want);
      if (n_want) {
        if (int rc = ids_room(n_want, (uint64_t)async_steps * sinks.size())) return rc;
        if (int rc = reserve((uint64_t)n_slots + n_want)) return rc;
        if (int rc = mark_occupancy()) return rc;  // no-op right after a step
        if (int rc = recount()) return rc;         // no-op right after a step
        // generators that ask for the same sinks every step (MonotonicCrowd) need no new upload
        if (want_on_device.size() != sinks.size() ||
            std::memcmp(want_on_device.data(), want, sinks.size() * sizeof(uint32_t)) != 0) {
          HIP_OK(hipMemcpyAsync(want_dev.get(), want, sinks.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                stream));
          want_on_device.assign(want, want + sinks.size());
        }
        spawn_ran = true;
        spawn_first_slot = n_slots;  // the k-th spawn of this step lands in slot n_slots + k
        if (any_route_hlp)
          if (int rc = flush_route_tables()) return rc;
        prof_begin(CS_K_SPAWN);
        {
          const uint32_t nb = ((uint32_t)sinks.size() + SPAWN_BLOCK - 1u) / SPAWN_BLOCK;
          hipLaunchKernelGGL(k_spawn_count, dim3(nb), dim3(SPAWN_BLOCK), 0, stream, sinks_dev.get(), want_dev.get(),
                             (uint32_t)sinks.size(), src_occupied.get(), ctr.get(), spawn_scratch.get());
          hipLaunchKernelGGL(k_spawn_apply, dim3(nb), dim3(SPAWN_BLOCK), 0, stream, view(cur), n_slots,
                             (uint32_t)cap, sinks_dev.get(), want_dev.get(), (uint32_t)sinks.size(), n_want, src_occupied.get(),
                             cell_count.get(), spawned_slots_dev.get(), ctr.get(), spawn_scratch.get());
        }
        prof_end();
        HIP_OK(hipGetLastError());
        n_slots += n_want;
        sorted = false;
        if (any_callback_hlp) {
          // a host planner must see set_target(new agent) BEFORE this step asks it for a velocity
          // (lib.rs:236-250 runs before the update loop): read the spawn result back now
          Counters c0;
          if (int rc = read_counters(&c0)) return rc;
          if (int rc = finish_spawn_events(c0.n_spawned, (uint64_t)c0.next_id - c0.n_spawned)) return rc;
          if (int rc = flush_route_pending()) return rc;  // before the re-sort moves the new agents
          spawn_events_done = true;
        }
      }
    }

    if (has_sinks && !spawn_ran && !(tile && spawn_on_device))  // n_spawned (n_halo_overflow is sticky)
      HIP_OK(hipMemsetAsync(&ctr.get()->n_spawned, 0, sizeof(uint32_t), stream));

    // ---- index for this step (location_hash_2d.rs:126-149) ----
    const bool rebuilt = !sorted;
    if (!rebuilt)  // no re-sort this step: the scan is what normally zeroes the step counters
      HIP_OK(hipMemsetAsync(&ctr.get()->n_destroyed, 0, 6 * sizeof(uint32_t), stream));
    // the form of the neighbour kernel is known before the sort: LDS-tiled strips when the crowd
    // is large enough to fill them; its band windows are then built in the scatter launch
    const uint64_t n_rows = ncells / std::max<uint64_t>(nx, 1);
    const int h = max_eyesight > 0.0 ? (int)std::ceil(max_eyesight / grid.cell_size - 1e-6) : 0;
    bool tiled = n_slots >= 2048 && h >= 1 && 2 * h + 1 <= TILE_MAX_ROWS && nx >= (uint64_t)(3 * h + 2);
    if (flags & CS_CFG_FORCE_GATHER) tiled = false;
    if ((flags & CS_CFG_FORCE_TILED) && h >= 1 && 2 * h + 1 <= TILE_MAX_ROWS) tiled = true;
    const uint32_t own_rows = gdev.own_x1 - gdev.own_x0;
    const uint32_t n_bands = tile_rows > 1 ? (own_rows + tile_rows - 1u) / tile_rows : 0u;
    // staged agents a window may have: the builder keeps windows within it (95 %: the ghost rows
    // are only estimated there)
    uint32_t agents_cap_now = tiled ? tile_agents_cap(h) : 0u;
    // (a tile's slot count moves with every exchange, and the LDS slots a window may stage follow the crowd's mean
    // occupancy in steps of 64: a kept list, and the builders' context, must not change with every such step.  While
    // the figure stays within 1/16 of the one the kept list was cut for, that one is used.)
    if (windows_valid && kept_agents_cap && agents_cap_now + kept_agents_cap / 16u >= kept_agents_cap &&
        agents_cap_now <= kept_agents_cap + kept_agents_cap / 16u)
      agents_cap_now = kept_agents_cap;
    const uint32_t stage_cap = tile_stage_cap ? tile_stage_cap : agents_cap_now - agents_cap_now / 20u;
    // The most band windows the builder can make (build_band's budget summed over the bands): two
    // consecutive windows cut by the agent bound hold more than tile_target owned agents, two cut by
    // the staging bound stage more than stage_cap (every row is staged by (rb + 2h) / rb bands), plus
    // the windows cut by the column bound of the fixed-point range and one odd window per bound and
    // band.  The step kernel's launch and the descriptor array are sized by it.
    // the window builder off the critical path (see windows_shadow): a small crowd steps on the windows of the step before
    // (a tile's slot count is an upper bound that runs ahead of its agents by up to kFlight + 1 exchanges' capacities: the
    //  size limit, which is about AGENTS, allows for that; without it a 250,000-agent tile, configs[2]'s share on four
    //  GPUs, fell out of the kept windows: 92.9 -> 86.5 us per step, profiles/r05/kept_windows_tile_limit.txt)
    uint64_t keep_limit = windows_keep_max_agents;
    if (tile)
      for (int d = 0; d < 8; ++d)
        if (halo[d].recv) keep_limit += (uint64_t)halo[d].cap * (kFlight + 2u);
    const bool want_keep = tiled && tile_rows > 1 && windows_shadow && n_slots <= keep_limit &&
                           (gdev.own_y1 - gdev.own_y0) <= BAND_LDS_COLS && !tile_windows_cap && split_margin() == 0u;
    const uint32_t band_target = want_keep ? tile_target - tile_target * std::min(windows_slack_pct, 50u) / 100u : tile_target;
    uint32_t band_windows_max = 0;
    if (tiled && tile_rows > 1) {
      const uint32_t rb = tile_rows;
      band_windows_max = 2u * (n_slots / band_target) +
                         n_bands * (2u + (gdev.own_y1 - gdev.own_y0) / tile_max_cols((uint32_t)h)) + 1u +
                         (uint32_t)(2ull * ((uint64_t)n_slots * (rb + 2u * (uint32_t)h) / rb) / std::max(stage_cap, 1u));
      // (cover mode: at most one filler in front of every window, one behind the last of a band, and those a long empty
      // stretch is cut into)
      if (want_keep) band_windows_max = 2u * band_windows_max + n_bands * (2u + (gdev.own_y1 - gdev.own_y0) / tile_max_cols((uint32_t)h));
      if (tile_windows_cap) band_windows_max = std::min(band_windows_max, tile_windows_cap);
      const uint64_t need = (uint64_t)band_windows_max * (split_margin() ? 2u : 1u);  // (split: two lists share the array)
      if (need > blk_desc_cap) {
        HIP_OK(hipStreamSynchronize(stream));
        if (int rc = alloc_window_arrays((uint32_t)std::min<uint64_t>(need + need / 4u, 0x7FFFFFFFull))) return rc;
      }
    }
    bool keep_now = false;
    if (want_keep) {
      WindowsKey key;
      std::memset(&key, 0, sizeof key);
      key.ncells = gdev.ncells; key.nx = gdev.nx;
      key.own_x0 = gdev.own_x0; key.own_x1 = gdev.own_x1; key.own_y0 = gdev.own_y0; key.own_y1 = gdev.own_y1;
      key.org_x = gdev.org_x; key.org_y = gdev.org_y;
      key.h = (uint32_t)h; key.desc_cap = blk_desc_cap; key.rows = tile_rows; key.target = band_target;
      key.stage_cap = stage_cap; key.split = split_margin();
      key.desc = blk_desc.get() < blk_desc_back.get() ? blk_desc.get() : blk_desc_back.get();  // (the pair; the two swap every step)
      keep_now = windows_valid && key == windows_key && n_slots != 0u;
      if (keep_now) n_steps_on_kept_windows += 1;
      windows_key = key;
    }
    // (set again below once windows for the next step really exist: a cover build in this step's own launches, or kept
    // windows with their builder workgroups; an empty crowd builds nothing)
    const bool had_windows = windows_valid;
    windows_valid = false;
    bool cover_built_late = false;  // (the builder ran as a launch of its own: no sort was due this step)
    // (windows built to be stepped on a step later get room in what they stage as well as in what they own)
    const uint32_t build_stage_cap = want_keep ? stage_cap - stage_cap * std::min(windows_slack_pct, 50u) / 200u : stage_cap;
    if (int rc = rebuild(tiled && !keep_now ? n_bands : 0u, tile_rows, (uint32_t)h, build_stage_cap, keep_now, want_keep && !keep_now,
                         band_target))
      return rc;

    // ---- HighLevelPlanner callbacks (slow path) ----
    if (any_velocity_callback)
      if (int rc = eval_callback_hlps()) return rc;
    // ---- field planners: on the device, behind that upload (it writes the whole of pref), nothing waited for ----
    if (any_field_hlp)
      if (int rc = hlp_field_eval(this)) return rc;
    if (any_route_hlp)
      if (int rc = flush_route_tables()) return rc;

    // ---- Phases B + C: per-agent update and commit (lib.rs:259-359) ----
    if (has_sinks && !spawn_ran)
      HIP_OK(hipMemsetAsync(src_occupied.get(), 0, std::max<size_t>(sinks.size(), 1) * sizeof(uint32_t), stream));
    // cell_count is all zero here: the scan clears it while reading (k_scan_apply)
    if (tile && n_slots && !bands_built)  // ghosts get no thread: their output slots must read "dead"
      HIP_OK(hipMemsetAsync(buf[cur ^ 1].cell, 0xFF, (size_t)n_slots * sizeof(uint32_t), stream));  // (else the scatter did)
    StepParams P;
    P.g = gdev;
    P.dt = (float)dt_seconds;
    P.n = n_slots;
    P.has_sinks = has_sinks ? 1u : 0u;
    P.n_src_cells = 0;
    P.halo_late_check = 0;
    P.peek_seq = 0;
    if (tile) {
      if (!peek_host.get()) {
        HIP_OK(peek_host.alloc(3));
        peek_host.get()[0] = peek_host.get()[1] = peek_host.get()[2] = 0ull;
      }
      P.peek_seq = peek_next();
    }
    EpilogueCtx E;
    memset(&E, 0, sizeof(E));  // (compared bytewise below)
    E.out = view(cur ^ 1);
    E.cell_count = cell_count.get();
    E.ctr = ctr.get();
    E.groups = groups_dev.get();
    E.sinks = sinks_dev.get();
    E.waypoints = waypoints_dev.get();
    E.grid_off_x = grid.offset_x;
    E.grid_off_y = grid.offset_y;
    E.cell_size = grid.cell_size;
    E.destroyed = destroyed.get();
    E.destroyed_cap = destroyed_cap;
    E.wp_events = wp_events.get();
    E.wp_events_cap = wp_events_cap;
    E.src_cell_start = src_cell_start.get();
    E.src_sorted = src_sorted.get();
    E.src_occupied = src_occupied.get();
    E.route_desc = route_desc_dev.get();
    E.route_xy = route_xy_dev.get();
    E.route_book = any_route_hlp ? route_book_dev.get() : nullptr;
    E.route_book_mask = route_book_size ? route_book_size - 1u : 0u;
    E.hlp_route_scale = hlp_scale_dev.get();
    if (any_callback_lp && n_slots && !lp_vel.get()) {
      HIP_OK(lp_vel.alloc(cap));
      HIP_OK(hipMemsetAsync(lp_vel.get(), 0, cap * sizeof(float2), stream));
    }
    E.lp_vel = any_callback_lp ? lp_vel.get() : nullptr;
    E.peek = tile ? peek_host.get() : nullptr;
    // (keep_now: this step runs on the windows of the step before and cuts its own, for the next one, in the
    // neighbour kernel's launch.  Also where no sort was due, a query or a read between two steps having sorted already:
    // that sort's scan zeroed the owned count with nobody behind it to count again, which the builders do as they go;
    // the scan of a step's own sort clears the other array's window count, here it is cleared by hand)
    const uint32_t builders = (keep_now && n_slots) ? n_bands : 0u;
    if (builders && !rebuilt) HIP_OK(hipMemsetAsync(n_blocks_back.get(), 0, 2 * sizeof(uint32_t), stream));
    if (builders) {
      const bool front_low = blk_desc.get() < blk_desc_back.get();  // (address order: the same context every step)
      E.build_desc[0] = front_low ? blk_desc.get() : blk_desc_back.get();
      E.build_desc[1] = front_low ? blk_desc_back.get() : blk_desc.get();
      E.build_n_blocks[0] = front_low ? n_blocks_dev.get() : n_blocks_back.get();
      E.build_n_blocks[1] = front_low ? n_blocks_back.get() : n_blocks_dev.get();
      E.build_prefix = band_prefix.get();
      E.build_first = 0u;
      E.build_bands = builders;
      E.build_rows = tile_rows;
      E.build_target = band_target;
      E.build_stage_cap = build_stage_cap;
      E.build_max_cols = tile_max_cols((uint32_t)h);
      E.build_desc_cap = blk_desc_cap;
      E.build_g_h = (uint32_t)h;
      E.build_g = gdev;
    }
    bool fuse_pack = false;
    if (tile && halo_one_phase && halo_fuse) {
      for (int d = 0; d < 8; ++d) {
        E.halo_send.p[d] = halo[d].send;
        E.halo_send.cap[d] = halo[d].cap;
        fuse_pack = fuse_pack || halo[d].send;
      }
      if (fuse_pack) {
        E.halo_band = 2u * halo_cells;
        if (!halo_all_clean)  // no unpack since the buffers were last filled: reset the record counts
          for (int d = 0; d < 8; ++d)
            if (halo[d].send) HIP_OK(hipMemsetAsync(halo[d].send, 0, sizeof(uint32_t), stream));  // (word 1 stays: the mesh's failure word)
      }
    }
    // The step kernels read the context from device memory (one copy per output buffer); it is
    // written again only when something in it changed (a table was reallocated, sinks were added),
    // by a one-wave kernel that carries the new value as its argument: in stream order, without
    // a host synchronisation.  (The kernel's other arguments stayed by-value: moving the input
    // arrays and the tile configuration here as well cost 5 %, they are read in the hot loops.)
    const int epi_slot = cur ^ 1;
    if (!epi_dev.get()) {
      HIP_OK(epi_dev.alloc(2));
      epi_host = new EpilogueCtx[2];
      epi_valid[0] = epi_valid[1] = false;
    }
    if (!epi_valid[epi_slot] || memcmp(&epi_host[epi_slot], &E, sizeof(E)) != 0) {
      memcpy(&epi_host[epi_slot], &E, sizeof(E));
      hipLaunchKernelGGL(k_store_ctx, dim3(1), dim3(64), 0, stream, E, &epi_dev.get()[epi_slot]);
      HIP_OK(hipGetLastError());
      epi_valid[epi_slot] = true;
    }
    const EpilogueCtx* Ep = &epi_dev.get()[epi_slot];
    // ---- LocalPlanner callbacks (slow path, local_planner.rs:7-18 at lib.rs:276-291) ----
    if (any_callback_lp && n_slots)
      if (int rc = lp_callbacks_eval(this, P, Ep)) return rc;
    if (tiled) {
      TileCfg cfg;
      cfg.h = h;
      cfg.debug = (flags >> 8) & 0xFFu;
      // LDS budget per workgroup: staged agents (20 B each, ~(2h+1) strips of 256 + halo ends),
      // the cell table and the per-thread neighbour lists; sized so that `tile_blocks_per_cu`
      // workgroups fit in the 160 KiB of a CU
      const uint32_t rb = tile_rows;
      cfg.agents_cap = agents_cap_now;
      cfg.table_cap = 1024u * (uint32_t)(h > 1 ? 2 : 1);
      const size_t entry = 2u;  // a list entry is an LDS slot (u16)
      // A workgroup's share of the CU's 160 KiB: staged records, cell table, list rows + the spare
      // row, the kernel's static arrays, rounded up to the allocation unit.  The unit is 1,280 B
      // (160 KiB / 128), found with a probe kernel that counts resident workgroups per CU: 4 up
      // to 40,960 B, 3 up to 53,760 B; a 512 B unit would let a fourth / third one in where the
      // hardware does not (32-bit entries, 26 rows: 30 % slower than 24).
      const size_t fixed = (size_t)cfg.agents_cap * 20u + (size_t)cfg.table_cap * 2u + TILE_LIST_SPARE * TILE_THREADS * entry +
                           (builders ? tile_static_lds_builders : tile_static_lds);
      auto share = [&](uint32_t rows) {
        return (fixed + (size_t)rows * TILE_THREADS * entry + 1279u) / 1280u * 1280u;
      };
      // rows worth having before occupancy: about the neighbours a lane holds (what does not fit
      // is spilled to global memory); workgroups per CU: as configured, fewer while that many
      // rows do not fit (wide cells: a large staged tile)
      const double k_mean = (double)n_slots / (double)std::max<uint64_t>(ncells, 1) * 3.14159265 *
                            (max_eyesight / grid.cell_size) * (max_eyesight / grid.cell_size);
      // (measured: with 16-bit entries 58 rows at 3 per CU beat 32 at 4 (cell 4 m), 64 at 2 beat 24
      // at 3 by 30 % (cell 8 m); with 32-bit entries, a row costing 1 KiB, occupancy won every time)
      uint32_t want_rows = tile_min_rows ? tile_min_rows
                           : (uint32_t)std::min(40.0, std::max(16.0, k_mean * 1.25));
      want_rows = std::min(64u, (want_rows + 1u) & ~1u);
      uint32_t per_cu = std::max(1u, tile_blocks_per_cu);
      while (per_cu > 1u && share(want_rows) > (size_t)(160u * 1024u) / per_cu) --per_cu;
      while (per_cu > 1u && share(16u) > (size_t)(160u * 1024u) / per_cu) --per_cu;
      cfg.list_cap = tile_list_cap;
      if (!cfg.list_cap) {  // then as many (an even number of) rows as the share holds
        cfg.list_cap = 16u;
        while (cfg.list_cap + 2u <= 64u && share(cfg.list_cap + 2u) <= (size_t)(160u * 1024u) / per_cu)
          cfg.list_cap += 2u;
      }
      cfg.list_cap = std::min(cfg.list_cap, 64u);
      // (the staging ids borrow the list area: agents_cap * 4 bytes must fit; with agents_cap <= TILE_AGENTS_MAX that
      // is at most 48 rows, so the bound of 64 entries the lean time-to-collision pass walks is never passed)
      static_assert((size_t)TILE_AGENTS_MAX * 4u <= (size_t)64u * TILE_THREADS * 2u, "the staging ids must fit 64 list rows");
      while ((size_t)cfg.list_cap * TILE_THREADS * entry < (size_t)cfg.agents_cap * 4u && cfg.list_cap + 8u <= 64u) cfg.list_cap += 8u;
      if (getenv("CS_TILE_PRINT")) {
        static int once = 0;
        if (once++ < 2)
          fprintf(stderr, "crowdstep tile cfg: h %d agents_cap %u table %u list_cap %u per_cu %u want_rows %u split %u fuse %d\n", h,
                  cfg.agents_cap, cfg.table_cap, cfg.list_cap, per_cu, want_rows, split_margin(), (int)fuse_pack);
      }
      size_t lds = (size_t)cfg.agents_cap * 20u + (size_t)(cfg.list_cap + TILE_LIST_SPARE) * TILE_THREADS * entry +
                   (size_t)cfg.table_cap * 2u;
      if (builders) lds = std::max<size_t>(lds, BAND_SCRATCH_BYTES);  // (the builder workgroups' arrays live there)
      uint32_t grid_blocks;
      if (rb <= 1) {
        hipLaunchKernelGGL(k_build_blocks, dim3(1), dim3(1024), 0, stream, gdev, cell_start.get(), blk_desc.get(),
                           blk_desc_cap, n_blocks_dev.get(), ctr.get());
        grid_blocks = (n_slots + TILE_THREADS - 1u) / TILE_THREADS + (uint32_t)std::min<uint64_t>(n_rows, n_slots);
      } else {
        if (!bands_built && !keep_now) {  // (kept windows tile the bands whether or not a sort was due)
          if (!rebuilt) HIP_OK(hipMemsetAsync(n_blocks_dev.get(), 0, 2 * sizeof(uint32_t), stream));  // else the scan did
          hipLaunchKernelGGL(k_build_bands, dim3(n_bands), dim3(256), 0, stream, gdev, cell_start.get(), rb,
                             band_target, (uint32_t)h, build_stage_cap, tile_max_cols((uint32_t)h), split_margin(), want_keep ? 1u : 0u,
                             band_prefix.get(), blk_desc.get(), blk_desc_cap, n_blocks_dev.get(), ctr.get());
          cover_built_late = want_keep;
        }
        // two consecutive greedy windows of a band hold more than tile_target agents together
        // (+ the windows a band is cut into by the column bound of the fixed-point range)
        grid_blocks = tile_windows_cap ? band_windows_max : std::max(band_windows_max, (n_slots + TILE_THREADS - 1u) / TILE_THREADS);
        // (kept windows were cut for the crowd of the step before: a tile that has lost agents since, or an engine whose
        // slots were compacted, may hold more windows than this step's own bound)
        if (keep_now) grid_blocks = std::max(grid_blocks, windows_bound);
      }
      // spilled list rows: up to 64 entries per lane in all, or 128 for crowds announced as dense
      // (CS_CFG_DENSE: the second right-of-way mask); the scratch is sized for the most workgroups
      // the launch can have
      cfg.list_cap &= ~1u;
      // ... or whose mean occupancy says so: neighbours in sight ~ agents per cell x pi r^2 / cell^2
      const double k_est = (double)n_slots / (double)std::max<uint64_t>(ncells, 1) * 3.14159265 *
                           (max_eyesight / grid.cell_size) * (max_eyesight / grid.cell_size);
      const uint32_t all_cap = ((flags & CS_CFG_DENSE) || k_est > 44.0) ? 128u : 64u;
      cfg.spill_rows = tile_spill_rows >= 0 ? (uint32_t)tile_spill_rows : all_cap - std::min(cfg.list_cap, all_cap);
      cfg.spill_rows = std::min(cfg.spill_rows, all_cap - std::min(cfg.list_cap, all_cap));
      const bool split = rb > 1 && split_margin() != 0u;
      {
        // (a split step's two launches may run side by side: each has its own spill area)
        const uint64_t words = (uint64_t)grid_blocks * cfg.spill_rows * TILE_THREADS * (split ? 2u : 1u);
        if (words > tile_spill.count()) {
          HIP_OK(hipStreamSynchronize(stream));
          HIP_OK(tile_spill.alloc(words + words / 4));
        }
      }
      cfg.spill = tile_spill.get();
      cfg.part = 0;
      cfg.desc_cap = blk_desc_cap;
      cfg.split = split ? 1u : 0u;
      cfg.build_sel = (builders && blk_desc.get() < blk_desc_back.get()) ? 1u : 0u;  // (the back array's place in the context)
      // (crowds whose agents all run the waypoint test keep the context in registers: k_step_tiled)
      // (CS_DEBUG_CTX_BY_VALUE=1, measurement only: a plain crowd through the instantiation with 146 spilled scalars,
      //  profiles/K4_LEVERS.md round 5)
      const bool ctx_by_value = has_sinks || any_route_hlp || debug_ctx_by_value;
      // (windows that stage at most TILE_XF_ROWS rows, owned rows + h on either side, keep x as an exact float: k_step_tiled, XF)
      const bool x_float = rb + 2u * (uint32_t)h <= (uint32_t)TILE_XF_ROWS;
      auto launch_tiled_as = [&](auto xf_tag, hipStream_t s, const StepParams& Pl, const TileCfg& c) {
        constexpr bool XF = decltype(xf_tag)::value;
        const dim3 grid(grid_blocks + builders), block(TILE_THREADS);
        const EpilogueCore& Ec = static_cast<const EpilogueCore&>(E);
        if (ctx_by_value && builders)
          hipLaunchKernelGGL((k_step_tiled<true, true, false, XF>), grid, block, lds, s, Pl, view(cur), Ep, Ec, cell_start.get(), pref.get(), blk_desc.get(), n_blocks_dev.get(), c);
        else if (ctx_by_value)
          hipLaunchKernelGGL((k_step_tiled<true, false, false, XF>), grid, block, lds, s, Pl, view(cur), Ep, Ec, cell_start.get(), pref.get(), blk_desc.get(), n_blocks_dev.get(), c);
        else if (builders)
          hipLaunchKernelGGL((k_step_tiled<false, true, false, XF>), grid, block, lds, s, Pl, view(cur), Ep, Ec, cell_start.get(), pref.get(), blk_desc.get(), n_blocks_dev.get(), c);
        else
          hipLaunchKernelGGL((k_step_tiled<false, false, false, XF>), grid, block, lds, s, Pl, view(cur), Ep, Ec, cell_start.get(), pref.get(), blk_desc.get(), n_blocks_dev.get(), c);
      };
      auto launch_tiled = [&](hipStream_t s, const StepParams& Pl, const TileCfg& c) {
        if (x_float) launch_tiled_as(std::true_type{}, s, Pl, c);
        else launch_tiled_as(std::false_type{}, s, Pl, c);
      };
      if (check_windows && n_slots && rb > 1 && !split)
        if (int rc = check_window_list(blk_desc.get(), n_blocks_dev.get(), rb, n_bands, tile_max_cols((uint32_t)h), want_keep, grid_blocks)) return rc;
      if (n_slots && P.peek_seq) flight_launched(P.peek_seq);
      prof_begin(CS_K_NEIGHBOUR_FORCE);
      early_pending = false;
      if (n_slots && split && overlap_ready && overlap_early && (!need_host || fire_and_forget)) {
        // "Early exchange": ONE launch, the border windows in its first workgroups (the dispatcher starts those first);
        // the last of them to finish publishes this launch's number, and the exchange of the next step goes out on the
        // second stream behind a one-wave kernel that waits for that (cs_tile_step_rccl), while the interior windows
        // still run.  No split-launch cost: the chip is filled by one launch as in the plain schedule.
        if (int rc = ensure_aux()) return rc;
        TileCfg c2 = cfg;
        c2.split = 2u;
        if (++early_seq == 0u) early_seq = 1u;
        c2.flag_seq = early_seq;
        StepParams Pc = P;
        Pc.halo_late_check = fuse_pack ? 1u : 0u;  // (the interior windows' check; the border windows skip it themselves)
        {
          const dim3 grid(grid_blocks), block(TILE_THREADS);  // (no builder workgroups: kept windows and a split exclude each other)
          const EpilogueCore& Ec = static_cast<const EpilogueCore&>(E);
          if (ctx_by_value && x_float)
            hipLaunchKernelGGL((k_step_tiled<true, false, true, true>), grid, block, lds, stream, Pc, view(cur), Ep, Ec, cell_start.get(), pref.get(), blk_desc.get(), n_blocks_dev.get(), c2);
          else if (ctx_by_value)
            hipLaunchKernelGGL((k_step_tiled<true, false, true>), grid, block, lds, stream, Pc, view(cur), Ep, Ec, cell_start.get(), pref.get(), blk_desc.get(), n_blocks_dev.get(), c2);
          else if (x_float)
            hipLaunchKernelGGL((k_step_tiled<false, false, true, true>), grid, block, lds, stream, Pc, view(cur), Ep, Ec, cell_start.get(), pref.get(), blk_desc.get(), n_blocks_dev.get(), c2);
          else
            hipLaunchKernelGGL((k_step_tiled<false, false, true>), grid, block, lds, stream, Pc, view(cur), Ep, Ec, cell_start.get(), pref.get(), blk_desc.get(), n_blocks_dev.get(), c2);
        }
        border_on_aux = true;
        early_pending = true;
      } else if (n_slots && split) {
        // The windows along the tile's edges first, as a launch of their own: they pack the next
        // step's halo records (fuse_pack), so the exchange can start when THEY are done, while the
        // interior windows still run.  With overlap_ready (cs_tile_step_rccl) they go to a second
        // stream, which the caller then hands the exchange to.
        TileCfg cfg_b = cfg;
        cfg_b.part = 1;
        cfg_b.spill = tile_spill.get() + (uint64_t)grid_blocks * cfg.spill_rows * TILE_THREADS;
        hipStream_t sb = stream;
        border_on_aux = false;
        if (overlap_ready && (!need_host || fire_and_forget)) {
          if (int rc = ensure_aux()) return rc;
          HIP_OK(hipEventRecord(ev_sorted, stream));
          HIP_OK(hipStreamWaitEvent(aux_stream, ev_sorted, 0));
          sb = aux_stream;
          border_on_aux = true;
        }
        const int tb = prof_open_on(CS_K_STEP_BORDER, sb);
        launch_tiled(sb, P, cfg_b);
        prof_close_on(tb, sb);
        if (border_on_aux) HIP_OK(hipEventRecord(ev_border, aux_stream));
        StepParams Pi = P;
        Pi.halo_late_check = fuse_pack ? 1u : 0u;
        const int ti = prof_open_on(CS_K_STEP_INTERIOR, stream);
        launch_tiled(stream, Pi, cfg);
        prof_close_on(ti, stream);
        // everything that follows on the engine's stream comes after both launches
        if (border_on_aux) HIP_OK(hipStreamWaitEvent(stream, ev_border, 0));
      } else if (n_slots) {
        launch_tiled(stream, P, cfg);
      }
      prof_end();
    } else {
      if (tile)  // owned count + slot count of the step output
        hipLaunchKernelGGL(k_build_blocks, dim3(1), dim3(1024), 0, stream, gdev, cell_start.get(), blk_desc.get(),
                           blk_desc_cap, n_blocks_dev.get(), ctr.get());
      if (n_slots && P.peek_seq) flight_launched(P.peek_seq);
      prof_begin(CS_K_NEIGHBOUR_FORCE);
      if (n_slots)
        hipLaunchKernelGGL(k_step_gather, dim3((n_slots + 255) / 256), dim3(256), 0, stream, P, view(cur),
                           Ep, cell_start.get(), pref.get());
      prof_end();
    }
    HIP_OK(hipGetLastError());
    last_windows_count = (tiled && n_slots) ? n_blocks_dev.get() : nullptr;  // (CS_STAT_WINDOWS_LISTED; before the swap below)
    if (builders && check_windows)
      if (int rc = check_window_list(blk_desc_back.get(), n_blocks_back.get(), tile_rows, n_bands, tile_max_cols((uint32_t)h), true, 0xFFFFFFFFu)) return rc;
    if (builders) {  // the launch above has cut the next step's windows into the other array
      std::swap(blk_desc, blk_desc_back);
      std::swap(n_blocks_dev, n_blocks_back);
    }
    // windows a later step may run on exist if this step cut them in cover mode (in the scatter's launch or by builder
    // workgroups), or ran on kept ones without a sort being due (they are still there)
    windows_valid = want_keep && n_slots != 0u && tiled && (builders != 0u || (keep_now && had_windows) || (!keep_now && bands_built) || cover_built_late);
    if (windows_valid && (builders != 0u || !keep_now)) windows_bound = band_windows_max;  // (cut this step)
    if (windows_valid) kept_agents_cap = agents_cap_now;
    if (fuse_pack) {
      halo_prepacked = true;
      halo_all_clean = false;
      halo_counts_clean[0] = halo_counts_clean[1] = false;
    }

    if (!need_host || fire_and_forget) {
      // fire and forget: an out-of-bounds agent poisons the engine at the next sync.  With
      // source-sinks n_slots stays an upper bound (the gap reads "dead") until refresh_counts().
      cur ^= 1;
      sorted = false;
      hist_valid = true;
      occ_valid = has_sinks;
      if (has_sinks || tile) {
        counts_stale = true;
        ++async_steps;
      }
      errors_stale = true;
      spawn_committed = false;
      committed_spawns = 0;
      slots_added = 0;
      ghosts_present = false;  // the step wrote the agents this tile holds, nothing else
      return 0;
    }

    Counters c;
    if (int rc = read_counters(&c)) return rc;
    counts_stale = false;
    errors_stale = false;
    async_steps = 0;
    if (has_sinks && (!tile || spawn_on_device)) next_id = c.next_id;
    const uint64_t first_spawn_id = (uint64_t)c.next_id - c.n_spawned;
    if (c.n_scan_stalled) {  // (the sort this step ran on was garbage: whatever else the counters say follows from that)
      poisoned = true;
      error = poison_error = kScanStalled;
      return 7;
    }
    if (c.n_out_of_bounds || limbo_fail) {
      // "Index out of bounds" (location_hash_2d.rs:61-63 via lib.rs:299-302): nothing is
      // committed; the pre-step state (including this step's spawns) stays current.
      HIP_OK(hipMemsetAsync(&ctr.get()->n_out_of_bounds, 0, sizeof(uint32_t), stream));
      HIP_OK(hipMemsetAsync(cell_count.get(), 0, (ncells + 1) * sizeof(uint32_t), stream));  // partial histogram
      hist_valid = false;
      occ_valid = false;
      halo_invalidate();  // (records of a step that did not happen)
      n_alive_host = c.n_alive;
      n_slots = c.n_alive;
      if (!spawn_events_done) finish_spawn_events(c.n_spawned, first_spawn_id);
      error = "Index out of bounds";
      return 1;
    }
    if (c.n_win_dropped) {  // agents of the dropped windows were not stepped: nothing to roll back to
      poisoned = true;
      error = poison_error = kWindowsDropped;
      return 7;
    }
    if (c.n_early_stalled) {
      poisoned = true;
      error = poison_error = kEarlyStalled;
      return 7;
    }
    if (c.n_halo_late) {  // the neighbours' ghost rings are already missing this agent: nothing to roll back to
      poisoned = true;
      error = poison_error = "an agent of an interior window landed in the halo band within one step (it moved more than a cell, or its position became NaN and was binned to cell 0): it would miss the overlapped exchange";
      return 7;
    }
    cur ^= 1;
    sorted = false;
    hist_valid = true;
    occ_valid = has_sinks;
    n_slots = c.n_alive;  // the step wrote exactly the live population
    slots_added = 0;
    ghosts_present = false;
    if (!spawn_events_done)
      if (int rc = finish_spawn_events(c.n_spawned, first_spawn_id)) return rc;
    if (int rc = finish_destroy_events(c)) return rc;
    if (int rc = flush_route_pending()) return rc;  // set_target of this step's waypoint advances
    n_alive_host = tile ? (uint64_t)c.n_owned - c.n_destroyed : (uint64_t)c.n_alive - c.n_destroyed;
    if (c.n_halo_overflow) {
      error = "halo buffer overflow: raise capacity_records of cs_halo_set_buffers";
      poisoned = true;
      return 7;
    }
    if (report) {
      report->n_agents = n_alive_host;
      report->n_spawned = (tile && !spawn_on_device) ? committed_spawns : c.n_spawned;
      report->n_destroyed = c.n_destroyed;
      report->n_waypoint_hits = c.n_waypoint_hits;
      report->n_tti_zero = c.n_tti_zero;
      report->n_nonfinite = c.n_nonfinite;
      report->n_clamped = c.n_clamped;
    }
    spawn_committed = false;
    committed_spawns = 0;
    return 0;
  }

  // SPAWNED events + set_target for this step's spawns (lib.rs:151-153,236-250),
  // in ascending sink order.
  int finish_spawn_events(uint32_t n_spawned, uint64_t first_id) {
    if (!n_spawned) return 0;
    if (!record_events && !any_callback_hlp) return 0;  // nobody listens: nothing to read back
    std::vector<uint32_t> slots(n_spawned);
    HIP_OK(hipMemcpy(slots.data(), spawned_slots_dev.get(), n_spawned * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < n_spawned; ++k) {
      const HostSink& h = sinks[slots[k]];
      cs_event ev;
      ev.kind = CS_EVENT_SPAWNED;
      ev.source_sink = slots[k];
      ev.id = ext_id(first_id + k);
      ev.x = h.d.source_x;
      ev.y = h.d.source_y;
      if (record_events) events.push_back(ev);
      const cs_hlp_desc& p = hlps[h.d.hlp];
      if (p.kind == CS_HLP_CALLBACK && p.set_target && !h.waypoints.empty())
        p.set_target(p.user, ev.id, ev.x, ev.y, h.waypoints[0], h.waypoints[1], h.d.radius_sink,
                     h.d.radius_sink);
      // (a sink whose spawn route is known had its agent_cache entry written by the spawn kernel)
      if (p.kind == CS_HLP_ROUTE && !h.waypoints.empty() && h.spawn_route == 0) {
        const uint32_t st = route_set_target(h.d.hlp, spawn_first_slot + k, ev.x, ev.y, h.waypoints[0], h.waypoints[1]);
        // the same (source, first waypoint) pair for every later spawn of this sink: from now
        // on the spawn kernel writes the agent_cache entry itself
        if (st && sinks[slots[k]].spawn_route != st) {
          sinks[slots[k]].spawn_route = st;
          sinks_dirty = true;
          groups_dirty = true;
        }
      }
    }
    return 0;
  }

  // waypoint set_target callbacks (lib.rs:325-333) and DESTROYED events in
  // ascending id (lib.rs:378-380, canonical order).
  int finish_destroy_events(const Counters& c) {
    // (a field planner's groups are CS_HLP_CALLBACK groups to the step kernel, which lists their waypoint advances too:
    // nobody listens to those, and the scan zeroes the count before the next step appends)
    if (c.n_wp_events && (any_callback_hlp || any_route_hlp)) {
      uint32_t m = std::min(c.n_wp_events, wp_events_cap);
      std::vector<WpEvent> w(m);
      HIP_OK(hipMemcpy(w.data(), wp_events.get(), m * sizeof(WpEvent), hipMemcpyDeviceToHost));
      std::sort(w.begin(), w.end(), [](const WpEvent& a, const WpEvent& b) { return a.id < b.id; });
      for (const WpEvent& ev : w) {  // ascending id = the canonical visiting order
        const HostGroup& g = groups[ev.group];
        const cs_hlp_desc& p = hlps[g.hlp];
        if (g.sink < 0) continue;
        const bool cb = p.kind == CS_HLP_CALLBACK && p.set_target;
        if (!cb && p.kind != CS_HLP_ROUTE) continue;
        const HostSink& h = sinks[g.sink];
        if (2 * (size_t)ev.next_wp + 1 >= h.waypoints.size()) continue;
        double px, py;
        to_global(ev.cell, ev.ox, ev.oy, &px, &py);
        if (cb)
          p.set_target(p.user, ext_id(ev.id), px, py, h.waypoints[2 * ev.next_wp], h.waypoints[2 * ev.next_wp + 1],
                       h.d.radius_sink, h.d.radius_sink);
        else if (tile)
          route_misses.push_back(cs_route_miss{ext_id(ev.id), g.hlp, ev.slot, px, py, h.waypoints[2 * ev.next_wp],
                                               h.waypoints[2 * ev.next_wp + 1]});
        else
          route_set_target(g.hlp, ev.slot, px, py, h.waypoints[2 * ev.next_wp], h.waypoints[2 * ev.next_wp + 1]);
      }
    }
    if (c.n_destroyed && (record_events || any_callback_hlp)) {
      uint32_t m = std::min(c.n_destroyed, destroyed_cap);
      std::vector<uint2> d(m);
      HIP_OK(hipMemcpy(d.data(), destroyed.get(), m * sizeof(uint2), hipMemcpyDeviceToHost));
      std::sort(d.begin(), d.end(), [](const uint2& a, const uint2& b) { return a.x < b.x; });
      for (auto& it : d) {
        const HostGroup& g = groups[meta_group(gdev, it.y)];
        const cs_hlp_desc& p = hlps[g.hlp];
        const uint64_t id = ext_id(it.x);
        if (p.kind == CS_HLP_CALLBACK && p.remove_agent) p.remove_agent(p.user, id);
        cs_event ev;
        ev.kind = CS_EVENT_DESTROYED;
        ev.source_sink = g.sink >= 0 ? (uint32_t)g.sink : UINT32_MAX;
        ev.id = id;
        ev.x = ev.y = 0;
        if (record_events) events.push_back(ev);
      }
    }
    return 0;
  }

  // ---- tiles: pack / unpack one axis of the halo exchange ----
  int halo_pack(uint32_t axis) {
    if (poisoned) {
      error = poison_error;
      return 1;
    }
    if (int rc = recount()) return rc;  // ranks of appended records extend this histogram
    if (int rc = routes_for_halo()) return rc;
    halo_one_phase = false;  // the two-phase schedule packs per axis, with forwarding
    halo_invalidate();
    HaloDir& lo = halo[axis * 2];
    HaloDir& hi = halo[axis * 2 + 1];
    HaloDir& other_lo = halo[(axis ^ 1u) * 2];
    HaloDir& other_hi = halo[(axis ^ 1u) * 2 + 1];
    // record counts: the previous pack of the other axis has reset them, except the first time
    if (!halo_counts_clean[axis]) {
      if (lo.send) HIP_OK(hipMemsetAsync(lo.send, 0, sizeof(HaloRecord), stream));
      if (hi.send) HIP_OK(hipMemsetAsync(hi.send, 0, sizeof(HaloRecord), stream));
    }
    halo_counts_clean[axis] = false;  // about to be filled
    if ((lo.send || hi.send) && n_slots) {
      prof_begin(CS_K_HALO);
      hipLaunchKernelGGL(k_halo_pack, dim3((n_slots + 255) / 256), dim3(256), 0, stream, gdev, view(cur),
                         n_slots, axis, 2u * halo_cells, lo.send, hi.send,
                         std::max(lo.cap, hi.cap), ctr.get(), other_lo.send, other_hi.send);
      prof_end();
      halo_counts_clean[axis ^ 1u] = true;
    }
    HIP_OK(hipGetLastError());
    return 0;
  }
  int halo_unpack(uint32_t axis) {
    HaloDir& a = halo[axis * 2];
    HaloDir& b = halo[axis * 2 + 1];
    if (!a.recv && !b.recv) return 0;
    const uint32_t dcap = std::max(a.cap, b.cap);
    const uint32_t add = (a.recv ? a.cap : 0u) + (b.recv ? b.cap : 0u);
    if ((uint64_t)n_slots + add > cap)  // the tile's population grew: reallocate (rare)
      if (int rc = reserve((uint64_t)n_slots + add)) return rc;
    const uint32_t blocks = (dcap + 255u) / 256u;
    prof_begin(CS_K_HALO);
    hipLaunchKernelGGL(k_halo_unpack, dim3(2u * blocks), dim3(256), 0, stream, gdev, view(cur), (uint32_t)cap,
                       a.recv, b.recv, dcap, blocks, cell_count.get(), ctr.get());
    prof_end();
    n_slots += add;  // upper bound; kernels stop at the device-side count
    slots_added += add;
    slots_added_total += add;
    ghosts_present = true;
    sorted = false;
    occ_valid = false;
    HIP_OK(hipGetLastError());
    return 0;
  }

  // ---- one-phase form: all eight neighbours ----
  int halo_pack_all() {
    if (poisoned) {
      error = poison_error;
      return 1;
    }
    if (int rc = recount()) return rc;
    if (int rc = routes_for_halo()) return rc;
    halo_one_phase = true;
    if (halo_prepacked) {  // the step kernel packed what it moved, and nothing has changed since
      halo_prepacked = false;
      return 0;
    }
    HaloBuffers8 send;
    uint32_t hcap = 0;
    bool any = false;
    for (int d = 0; d < 8; ++d) {
      send.p[d] = halo[d].send;
      send.cap[d] = halo[d].cap;
      hcap = std::max(hcap, halo[d].cap);
      any = any || halo[d].send;
      if (halo[d].send && !halo_all_clean) HIP_OK(hipMemsetAsync(halo[d].send, 0, sizeof(uint32_t), stream));  // (word 1 stays)
    }
    halo_all_clean = false;
    halo_counts_clean[0] = halo_counts_clean[1] = false;
    if (any && n_slots) {
      prof_begin(CS_K_HALO_PACK);
      hipLaunchKernelGGL(k_halo_pack_all, dim3((n_slots + 255) / 256), dim3(256), 0, stream, gdev, view(cur),
                         n_slots, 2u * halo_cells, send, ctr.get());
      prof_end();
    }
    HIP_OK(hipGetLastError());
    return 0;
  }
  int halo_unpack_all() {
    HaloBuffers8 recv, send;
    uint32_t hcap = 0, add = 0;
    bool any = false;
    for (int d = 0; d < 8; ++d) {
      recv.p[d] = halo[d].recv;
      send.p[d] = halo[d].send;
      recv.cap[d] = send.cap[d] = halo[d].cap;
      if (halo[d].recv) {
        hcap = std::max(hcap, halo[d].cap);
        add += halo[d].cap;
        any = true;
      }
    }
    if (!any) return 0;
    peek_poll();
    if ((uint64_t)n_slots + add > cap)  // the tile's population grew: reallocate (rare)
      if (int rc = reserve((uint64_t)n_slots + add)) return rc;
    const uint32_t blocks = (hcap + 255u) / 256u;
    prof_begin(CS_K_HALO_UNPACK);
    hipLaunchKernelGGL(k_halo_unpack_all, dim3(8u * blocks), dim3(256), 0, stream, gdev, view(cur), (uint32_t)cap,
                       recv, send, blocks, cell_count.get(), ctr.get(), mesh_step_tag);
    prof_end();
    halo_all_clean = true;  // the kernel reset the send counts
    n_slots += add;  // upper bound; kernels stop at the device-side count
    slots_added += add;
    slots_added_total += add;
    ghosts_present = true;
    sorted = false;
    occ_valid = false;
    HIP_OK(hipGetLastError());
    return 0;
  }

  // The local grid of this engine: the whole grid, or (tile) the owned rectangle [cx0, cx1) x
  // [cy0, cy1) of global cells plus a ghost ring of H cells.  (Re)allocates the per-cell tables.
  int set_geometry(bool is_tile, uint32_t cx0, uint32_t cx1, uint32_t cy0, uint32_t cy1, uint32_t H) {
    nx = gnx;
    ny = gny;
    uint32_t ox0 = 0, ox1 = (uint32_t)gny, oy0 = 0, oy1 = (uint32_t)gnx, org_x = 0, org_y = 0;
    tile = is_tile;
    if (is_tile) {
      if (cx0 >= cx1 || cy0 >= cy1 || cx1 > gny || cy1 > gnx || H == 0) {
        error = "bad tile rectangle / halo_cells";
        return 3;
      }
      halo_cells = H;
      const uint32_t lx0 = cx0 > H ? cx0 - H : 0, ly0 = cy0 > H ? cy0 - H : 0;
      const uint32_t lx1 = (uint32_t)std::min<uint64_t>(gny, (uint64_t)cx1 + H);
      const uint32_t ly1 = (uint32_t)std::min<uint64_t>(gnx, (uint64_t)cy1 + H);
      ny = lx1 - lx0;
      nx = ly1 - ly0;
      org_x = lx0;
      org_y = ly0;
      ox0 = cx0 - lx0;
      ox1 = cx1 - lx0;
      oy0 = cy0 - ly0;
      oy1 = cy1 - ly0;
    }
    ncells = nx * ny;
    gdev.nx = (uint32_t)nx;
    gdev.ny = (uint32_t)ny;
    gdev.ncells = (uint32_t)ncells;
    gdev.tile = tile ? 1u : 0u;
    gdev.own_x0 = ox0;
    gdev.own_x1 = ox1;
    gdev.own_y0 = oy0;
    gdev.own_y1 = oy1;
    gdev.org_x = org_x;
    gdev.org_y = org_y;
    cell_count.release(); cell_start.release(); block_totals.release(); band_prefix.release(); src_cell_start.release();
    n_scan_blocks = (uint32_t)std::max<uint64_t>(1, (ncells + SCAN_TILE - 1) / SCAN_TILE);
    HIP_OK(cell_count.alloc(ncells + 1));
    HIP_OK(cell_start.alloc(ncells + 1));
    HIP_OK(block_totals.alloc(n_scan_blocks));
    HIP_OK(band_prefix.alloc(ncells + 1));
    HIP_OK(hipMemset(cell_count.get(), 0, (ncells + 1) * sizeof(uint32_t)));
    HIP_OK(hipMemset(cell_start.get(), 0, (ncells + 1) * sizeof(uint32_t)));
    return 0;
  }

  // ---- re-cutting a running mesh: export everything owned, take a new rectangle, import ----
  int tile_histogram(uint64_t* rows, uint64_t* cols) {
    if (int rc = refresh_counts()) return rc;
    DevBuf<uint32_t> rows_mem, cols_mem;
    HIP_OK(rows_mem.alloc(gny));
    HIP_OK(cols_mem.alloc(gnx));
    uint32_t *d_rows = rows_mem.get(), *d_cols = cols_mem.get();
    HIP_OK(hipMemsetAsync(d_rows, 0, gny * sizeof(uint32_t), stream));
    HIP_OK(hipMemsetAsync(d_cols, 0, gnx * sizeof(uint32_t), stream));
    if (n_slots)
      hipLaunchKernelGGL(k_tile_histogram, dim3((n_slots + 255u) / 256u), dim3(256), 0, stream, gdev, view(cur), n_slots, ctr.get(),
                         (tile && ghosts_present) ? 1u : 0u, d_rows, d_cols);
    std::vector<uint32_t> hr(gny), hc(gnx);
    HIP_OK(hipMemcpyAsync(hr.data(), d_rows, gny * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(hc.data(), d_cols, gnx * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    for (uint64_t k = 0; k < gny; ++k) rows[k] += hr[k];
    for (uint64_t k = 0; k < gnx; ++k) cols[k] += hc[k];
    return 0;
  }
  // returns the number of owned agents; writes min(that, cap) records
  long long tile_export(HaloRecord* out, size_t cap_records) {
    if (refresh_counts() != 0) return -1;
    DevBuf<HaloRecord> out_mem;
    DevBuf<uint32_t> count_mem;
    const uint32_t cap_dev = (uint32_t)std::min<size_t>(std::max<size_t>(cap_records, 1), n_slots + 1u);
    if (out_mem.alloc(cap_dev) != hipSuccess || count_mem.alloc(1) != hipSuccess) {
      error = "HIP error while exporting a tile";
      return -1;
    }
    HaloRecord* d_out = out_mem.get();
    uint32_t* d_count = count_mem.get();
    uint32_t count = 0;
    bool ok = hipMemsetAsync(d_count, 0, sizeof(uint32_t), stream) == hipSuccess;
    if (n_slots)
      hipLaunchKernelGGL(k_tile_export, dim3((n_slots + 255u) / 256u), dim3(256), 0, stream, gdev, view(cur), n_slots, ctr.get(),
                         (tile && ghosts_present) ? 1u : 0u, d_out, cap_dev, d_count);
    ok = ok && hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipStreamSynchronize(stream) == hipSuccess;
    const size_t m = std::min<size_t>(std::min<size_t>(count, cap_dev), cap_records);
    if (ok && m && out) ok = hipMemcpy(out, d_out, m * sizeof(HaloRecord), hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) {
      error = "HIP error while exporting a tile";
      return -1;
    }
    return (long long)count;
  }
  int tile_retile(uint32_t cx0, uint32_t cx1, uint32_t cy0, uint32_t cy1) {
    if (!tile) {
      error = "cs_tile_retile needs a tile engine";
      return 3;
    }
    if (int rc = refresh_counts()) return rc;
    HIP_OK(hipStreamSynchronize(stream));
    if (int rc = set_geometry(true, cx0, cx1, cy0, cy1, halo_cells)) return rc;
    // nobody lives here until cs_tile_import; planners, groups, source-sinks, ids and routes stay
    n_slots = 0;
    n_alive_host = 0;
    slots_added = 0;
    ghosts_present = false;
    sorted = true;
    hist_valid = false;
    occ_valid = false;
    halo_invalidate();
    counts_stale = errors_stale = false;
    async_steps = 0;
    spawn_committed = false;
    {
      Counters c;
      HIP_OK(hipMemcpy(&c, ctr.get(), sizeof c, hipMemcpyDeviceToHost));
      c.n_alive = c.n_owned = c.n_pending = c.n_spawned = c.n_destroyed = 0;
      HIP_OK(hipMemcpy(ctr.get(), &c, sizeof c, hipMemcpyHostToDevice));
    }
    for (auto& h : halo) h = HaloDir{};  // the caller sets buffers for the new neighbours' edges
    halo_all_clean = false;
    halo_counts_clean[0] = halo_counts_clean[1] = false;
    sinks_dirty = true;  // the sources are binned in local cells
    if (int rc = alloc_window_arrays((uint32_t)(cap / 32 + ncells / std::max<uint64_t>(nx, 1) + 8))) return rc;
    return upload_sinks();
  }
  int tile_import(const HaloRecord* rec, size_t n) {
    halo_invalidate();
    if (!tile) {
      error = "cs_tile_import needs a tile engine";
      return 3;
    }
    if (n == 0) return 0;
    for (size_t k = 0; k < n; ++k)  // (host memory: records somebody else made; the kernels read the right of way
      if (rec[k].id >= id_limit) {  //  from the sign of an id difference, which needs ids below 2^31)
        error = "cs_tile_import: a record's agent id is beyond the device's 31-bit id space";
        return 3;
      }
    if (int rc = upload_groups()) return rc;
    if (int rc = recount()) return rc;
    if (int rc = reserve((uint64_t)n_slots + n)) return rc;
    DevBuf<HaloRecord> rec_mem;
    DevBuf<uint32_t> kept_mem;
    HIP_OK(rec_mem.alloc(n));
    HIP_OK(kept_mem.alloc(1));
    HaloRecord* d_rec = rec_mem.get();
    uint32_t* d_kept = kept_mem.get();
    HIP_OK(hipMemcpy(d_rec, rec, n * sizeof(HaloRecord), hipMemcpyHostToDevice));
    HIP_OK(hipMemsetAsync(d_kept, 0, sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_tile_import, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, stream, gdev, view(cur), (uint32_t)cap,
                       d_rec, (uint32_t)n, cell_count.get(), ctr.get(), d_kept);
    uint32_t kept = 0;
    HIP_OK(hipMemcpyAsync(&kept, d_kept, sizeof kept, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    n_slots += kept;
    slots_added_total += kept;
    n_alive_host += kept;
    if (kept) sorted = false;
    occ_valid = false;
    halo_invalidate();
    return 0;
  }

  // device memory the engine holds, by what it grows with (cs_device_bytes)
  uint64_t device_bytes() const {
    uint64_t b = 0;
    b += 2ull * cap * (2 * sizeof(float2) + 5 * sizeof(uint32_t));                    // the two agent buffers
    b += cap * sizeof(float2) + (uint64_t)destroyed_cap * sizeof(uint2) + (uint64_t)wp_events_cap * sizeof(WpEvent);
    b += (uint64_t)blk_desc_cap * sizeof(BlockDesc) + tile_spill.bytes();
    b += 4ull * (ncells + 1) * sizeof(uint32_t) + (uint64_t)n_scan_blocks * sizeof(uint32_t);  // cell tables
    b += sinks.size() * (sizeof(SinkDev) + 5 * sizeof(uint32_t)) + spawn_rec_dev.bytes();
    b += route_desc_dev.bytes() + route_xy_dev.bytes() + (uint64_t)route_book_size * sizeof(RouteBookEntry) +
         hlp_scale_dev.bytes() + route_pending_dev.bytes();
    for (const Snapshot& sn : snap) b += sn.cap * sizeof(cs_snapshot_record);
    b += write_scratch.bytes();  // the batches of the by-id calls (write, read, remove) and the selections' lists
    b += sel_groups_dev.bytes();
    b += field_scratch.bytes();  // the raster of the last cs_agent_field (cs_field.hip.inc)
    b += hlp_field_bytes();    // the field planners' samples and their table (cs_hlp_field.hip.inc)
    b += flow_scratch.bytes();  // the rasters of the last cs_flow_field_solve (cs_flow_solve.hip.inc)
    b += pairs_scratch.bytes();  // the kept part of the lists of the distance queries, at most 16 MiB (cs_near.hip.inc)
    return b;
  }

  // make buf[cur] sorted for queries between steps
  int ensure_index() {
    if (sorted) return 0;
    return rebuild();
  }
};
