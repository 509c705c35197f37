// cs_device_types.hip.inc — device-side tables, the arithmetic of the neighbour pass (TTC, Zanlungo force), re-binning, source marks
// Part of the single translation unit crowdstep_hip.hip (included there, in order).

// ---------------------------------------------------------------------------
// device-side tables
// ---------------------------------------------------------------------------
struct GridDev {
  uint32_t nx;      // row stride AND number of x rows: (width / cell) as usize
  uint32_t ny;      // (height / cell) as usize
  uint32_t ncells;  // nx * ny
  float cs;         // cell size, f32
  float cs_lo;      // cell_size - (double)cs, second word for exact re-basing
  float inv_cs;
  // tile mode (one engine per GPU): the local grid is the owned cell rectangle
  // [own_x0, own_x1) x [own_y0, own_y1) (local cell coordinates) plus its ghost ring; local
  // cell (0,0) is global cell (org_x, org_y).  Not a tile: tile = 0 and the owned rectangle
  // is the whole grid.
  uint32_t tile;
  uint32_t own_x0, own_x1, own_y0, own_y1;
  uint32_t org_x, org_y;
  // Relative positions of the neighbour pass are formed in fixed point (fix_rel below): one unit =
  // 1 / fix_scale metres (cell / 2^23 rounded to a power of two), cs_fix = the cell size in those units.
  int32_t cs_fix;
  float fix_scale, fix_inv;
  // AgentArrays::meta = planner group (low grp_bits bits) | next_waypoint (the rest).  16 / 16 until an engine
  // has more than 65,535 groups (every source-sink is one), then 20 / 12 (cs_engine::widen_groups)
  uint32_t grp_bits;
};
__host__ __device__ inline uint32_t meta_group(const GridDev& g, uint32_t meta) { return meta & ((1u << g.grp_bits) - 1u); }
__host__ __device__ inline uint32_t meta_waypoint(const GridDev& g, uint32_t meta) { return meta >> g.grp_bits; }
__host__ __device__ inline uint32_t meta_make(const GridDev& g, uint32_t group, uint32_t waypoint) {
  return group | (waypoint << g.grp_bits);
}

// ---------------------------------------------------------------------------
// Relative position of two agents, p_j - p_i, from cell-relative offsets.  Offsets are rounded
// once to fixed point (fix_coord: 2^-22 m for cells of (1, 2] m, i.e. cell / 2^23), the difference (offset_j + whole cells) - offset_i is then EXACT
// integer arithmetic, converted back to f32 once.  Exact integer differences do not depend on
// the origin they are measured from, so the LDS-tiled kernel can keep its staged agents in
// window-relative coordinates (one subtraction per pair, no per-cell shift) and still produce the
// bits of the gather kernel and of any tile mesh.  Offsets beyond +-FIX_LIM units (agents the
// reference has clamped far outside the grid) do not fit: the gather path takes such a pair in
// f32, the tiled kernel stages such an agent at FIX_FAR, where nothing sees it (it is at least
// 64 cells from its cell's origin, the tile reaches at most 8).
// ---------------------------------------------------------------------------
#define FIX_LIM 0x20000000  /* 2^29 */
#define FIX_FAR 0x40000000  /* 2^30 */
__device__ __forceinline__ bool fix_ok(float off, const GridDev& g) {
  return fabsf(off * g.fix_scale) < (float)FIX_LIM;  // false for NaN
}
__device__ __forceinline__ int fix_coord(float off, const GridDev& g) {
  return __float2int_rn(off * g.fix_scale);
}
// p_j - p_i in fixed units as floats (fx, fy) for a neighbour whose cell lies (sx, sy) cells from
// the own one; rp = (fx, fy) * g.fix_inv.  The radius test is fx^2 + fy^2 < (r * fix_scale)^2.
__device__ __forceinline__ void fix_rel(const GridDev& g, float2 oi, float2 oj, int sx, int sy, float& fx,
                                        float& fy) {
  if (fix_ok(oi.x, g) && fix_ok(oi.y, g) && fix_ok(oj.x, g) && fix_ok(oj.y, g) && abs(sx) <= 32 && abs(sy) <= 32) {
    fx = (float)(fix_coord(oj.x, g) - fix_coord(oi.x, g) + sx * g.cs_fix);
    fy = (float)(fix_coord(oj.y, g) - fix_coord(oi.y, g) + sy * g.cs_fix);
  } else {  // out of the fixed-point range: plain f32 (never reached by the tiled kernel)
    fx = ((oj.x + (float)sx * g.cs) - oi.x) * g.fix_scale;
    fy = ((oj.y + (float)sy * g.cs) - oi.y) * g.fix_scale;
  }
}

// One group per add_agents call / per source-sink: the reference passes the
// planners and the eyesight per call (lib.rs:119-125, source_sink.rs:46-59).
struct GroupDev {
  float eyesight;
  uint32_t lp_kind;  // 0 = NoLocalPlan, 1 = Zanlungo, 2 = a host LocalPlanner (its answer is read from EpilogueCore::lp_vel)
  float A, D, inv_mass, R;
  uint32_t hlp_kind;  // CS_HLP_*
  float hvx, hvy;
  int32_t sink;  // owning source-sink slot or -1
  uint32_t hlp;  // planner handle (the route book is kept per planner)
  // |fut|^2 in fixed units from which every forward force term is exactly +0 (zanlungo_forward_vanishes), set by the
  // host (cs_engine::upload_groups); NaN: never
  float vanish2;
};

// What a selection asks of an agent's planner group (cs_select.hip.inc): the owning source-sink as the HOST group knows it
// (kept after the sink was removed; 0xFFFFFFFF: no sink, cs_add_agents) and the two planner handles.  A table of its
// own, so that GroupDev, which the step kernels read, stays as it is.
struct SelGroupDev {
  uint32_t sink, hlp, lp;
};

struct SinkDev {
  double src_x, src_y;  // global, for events
  uint32_t src_cell;    // stored cell of the source point (or CS_INVALID_CELL)
  // tile engines: the source lies in the ghost ring (another tile owns it).  Its spawns are
  // appended here as ghosts in the step they happen: the halo exchange of that step ran before
  // the spawn phase, and the reference's new agent is a neighbour from its first step on.
  uint32_t ghost_cell;
  float src_ox, src_oy;
  float radius_sink;
  uint32_t wp_begin, wp_count;  // into the waypoint array (global f64 pairs)
  uint32_t loop_forever;
  uint32_t group;
  float eyesight;
  // CS_HLP_ROUTE: route_state value of an agent spawned here ((route + 1), waypoint 0) once the
  // route from the source to the first waypoint is in the route book; 0 = ask the host
  uint32_t spawn_route;
};

struct Counters {
  // persistent
  uint32_t n_alive;          // written by the scan: total of the histogram
  uint32_t n_out_of_bounds;  // cumulative: any non-zero value poisons the engine
  uint32_t n_owned;          // agents in the owned rectangle (tile mode; else = n_alive)
  uint32_t n_pending;        // slots in use in the unsorted buffer (halo unpack appends)
  uint32_t next_id;          // last_alloc_agent_id (lib.rs:83): the spawn kernel allocates from it
  // written before the re-sort of a step (zeroed by the host when sinks / tiles exist)
  uint32_t n_spawned;
  uint32_t n_halo_overflow;
  // written by the step kernel (zeroed by the scan of the same step)
  uint32_t n_destroyed;
  uint32_t n_waypoint_hits;
  uint32_t n_tti_zero;
  uint32_t n_nonfinite;
  uint32_t n_clamped;
  uint32_t n_wp_events;
  uint32_t n_halo_late;  // cumulative (like n_out_of_bounds): an interior agent reached the halo band in one step
  // cumulative diagnostics of the tiled kernel (cs_kernel_stat): windows that left the LDS path, windows walked in chunks
  uint32_t n_win_off_lds, n_win_chunked;
  // cumulative (like n_out_of_bounds): band windows the builder could not list, or the step kernel's launch could not
  // hold (the launch and the descriptor array are sized by a bound on the builder's output, cs_engine: band_windows_max):
  // their agents were not stepped, so any non-zero value poisons the engine
  uint32_t n_win_dropped;
  // cumulative: a tile of the one-launch cell scan gave up waiting for the totals of the tiles before it (k_scan_onepass:
  // cannot happen while the dispatcher starts workgroups in order; the wait is bounded all the same): the sort of that
  // step is garbage, the engine is poisoned
  uint32_t n_scan_stalled;
  // A mesh's failure word (cs_mesh, "a step that fails on one tile"): 0, or 1 + the index of the mesh step in whose halo
  // unpack the EARLIEST failure known to this tile was first seen by the tile it happened on.  Formed in k_halo_unpack_all
  // from this tile's own cumulative error counters and from word 1 of the headers of the halo buffers it has just
  // received (the smallest non-zero value wins), and written into word 1 of its own send headers: the word spreads one
  // tile per step through messages that travel anyway.  Never reset.
  uint32_t mesh_fail_step;
  // CS_CFG_TILE_OVERLAP, "early exchange" (k_step_tiled, TileCfg::split == 2): the border windows of a launch count
  // themselves off here; the last one publishes the launch's sequence number in border_flag, which the one-wave kernel in
  // front of the next step's exchange on the second stream waits for (k_wait_border).  n_early_stalled: cumulative, that
  // wait gave up (the two streams share a hardware queue, or the launch never ran): the exchange would have gone out before
  // the border windows had packed, so the engine is poisoned.
  uint32_t border_done, border_flag, n_early_stalled;
#ifdef CS_TILE_TRIPS  // diagnostic build (tools/trip_counts.sh): per-wave loop trips of the tiled kernel, cs_kernel_stat(100 + i)
  uint32_t dbg[20];
#endif
};

struct AgentArrays {
  float2* off;
  float2* vel;
  uint32_t* id;
  uint32_t* cell;  // stored flat cell (reference's location_to_index), or CS_INVALID_CELL
  uint32_t* meta;  // planner group | next_waypoint (meta_group / meta_waypoint: 16 / 16 bits, or 20 / 12)
  uint32_t* rank;  // arrival rank inside `cell` for the next scatter
  // CS_HLP_ROUTE: RMFPlanner's agent_cache entry of this agent, (route + 1) | waypoint << 22, 0 = no
  // route (rmf/mod.rs:86).  Travels with the agent through the scatter and the halo records.  The
  // kernels get a null pointer here while no route planner exists (nothing is read or copied).
  uint32_t* route;
};

// ---------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ float f_inf() { return __builtin_huge_valf(); }
__device__ __forceinline__ float f_nan() { return __builtin_nanf(""); }

// ---------------------------------------------------------------------------
// Arithmetic of the neighbour pass.  One definition, used by both neighbour
// kernels, so their results are bitwise equal.  Divisions, square roots and the
// exponential use the 1-ulp hardware forms (v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 /
// v_exp_f32): the IEEE-exact expansions cost ~10 VALU each and this kernel is
// VALU-issue bound (profiles/), while the fp32 tolerance of the path is 1e-4.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fast_rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Zanlungo::time_to_collision, zanlungo.rs:49-74 (collision distance is R, not 2R).
// With bh = b/2 the quadratic reads t = (-bh -+ sqrt(bh^2 - a c)) / a: the same values as
// the reference's (-b -+ sqrt(b^2 - 4ac)) / 2a, the factors of two being exact.  For a > 0
// the roots are ordered (t0 <= t1), which folds the reference's case analysis into
//   disc < 0 -> inf;  t0 > 0 -> t0;  t1 > 0 -> (t0 < 0 ? 0 : t1);  else inf.
// f32 has 1/8 of f64's exponent range: |rel_vel|^2 underflows near 1e-19 m/s where the
// reference's f64 does not, and a flushed `a` with b != 0 would read as "colliding now"
// (t0 = NaN or -inf, t1 = +inf -> 0 through v_max).  Two measures:
//  * ttc_select lets a NaN t0 fall through to t1, so that a pair which does NOT overlap and whose
//    |rel_vel|^2 has left the range comes out as +inf from the plain quadratic (ttc_core_c_f32): the
//    reference computes a collision years ahead for it, whose force term is below 1e-17 N;
//  * a pair that DOES overlap (0 < d2 <= R2: "colliding now" whatever the velocities, unless they are equal)
//    takes the guarded form (ttc_f32): tiny relative velocities scaled by 2^48 first
//    (t(s*rv) = t(rv)/s exactly), what still underflows in the a -> 0 limit of the same quadratic,
//    which is what f64 computes there (ttc_tiny_f32).  d2 = |rp|^2.
// ttc_pair_f32 is the two together.  (Until round 3 every pair with 0 < |rel_vel| < 1e-12 m/s took the
// guarded form, and a wave that met one repeated its whole pass: in a crowd whose forces are real, velocity
// components that differ by 1e-45 .. 1e-12 m/s are common (a force term that has all but underflowed
// perturbs a velocity component that was exactly equal), and nearly every wave paid for the pass twice.)
//
// UNITS.  Both forms are homogeneous in the relative position: called with rp, d2 and R2 in the
// neighbour pass's FIXED units (rp' = S rp with S = GridDev::fix_scale, a power of two, d2' = |rp'|^2,
// R2' = (S R)^2) they return T' = S T with the mantissa bits T would have had: every intermediate is
// the metre-valued one times a power of two.  The step kernels do exactly that: p_j - p_i comes out of
// the fixed-point subtraction as an integer number of units, and converting it to metres per pair
// (a multiplication by the scalar 1/S, which issues at half the rate of a plain v_mul on this chip:
// tools/valu_ceiling.hip) is saved; t_i is converted once per agent (make_force_ctx).

// the reference's case analysis (zanlungo.rs:61-73) for ordered roots t0 <= t1:
//   t1 > 0 ? (t0 > 0 ? t0 : (t0 < 0 ? 0 : t1)) : inf       (NaN roots fail every test: inf)
// The middle test is written "t0 neither below nor above 0" (one v_cmp_nlg_f32): a NaN t0 falls through to t1
// like an exact 0.  t0 alone is NaN only when |rel_vel|^2 has underflowed to 0 (0 * rcp(0), see ttc_pair_f32);
// t1 is then +-inf or NaN and the pair reads as "no collision" instead of v_max's "colliding now".
__device__ __forceinline__ float ttc_select(float t0, float t1) {
  float t = fmaxf(t0, 0.0f);                    // t0 > 0 -> t0, t0 < 0 -> 0
  t = !(t0 < 0.0f || t0 > 0.0f) ? t1 : t;       // "t0 == 0 exactly falls through to t1"
  return (t1 > 0.0f) ? t : f_inf();
}

// (tscale: 2^48 for tiny relative velocities, 2^-40 for huge ones, see ttc_f32)
__device__ __noinline__ float ttc_tiny_f32(float rvx, float rvy, float rpx, float rpy, float d2,
                                           float R2, float tscale) {
  rvx *= tscale;
  rvy *= tscale;
  const float a = __builtin_fmaf(rvx, rvx, rvy * rvy);
  const float bh = __builtin_fmaf(rvx, rpx, rvy * rpy);
  const float c = d2 - R2;
  if (a < 1e-30f) {
    if (bh == 0.0f) return f_inf();  // equal velocities: 0/0 = NaN fails every comparison
    if (c < 0.0f) return 0.0f;       // already inside R: t0 < 0 < t1
    return bh < 0.0f ? (-c / (2.0f * bh)) * tscale : f_inf();
  }
  const float disc = __builtin_fmaf(bh, bh, -(a * c));
  const float root = fast_sqrt(disc);
  const float ia = fast_rcp(a) * tscale;
  const float t0 = (-bh - root) * ia;
  const float t1 = (-bh + root) * ia;
  return (disc < 0.0f) ? f_inf() : ttc_select(t0, t1);
}

// The quadratic proper.  No test of the discriminant: disc < 0 makes the root NaN, both t0 and t1 NaN,
// every comparison false and the result +inf, which is the reference's answer.  Equal velocities
// (rv == 0 exactly) give a = bh = 0, t0 = t1 = 0 * inf = NaN -> +inf as well (the reference: 0/0 = NaN
// fails every comparison).  c = d2 - R2.
// Where |rel_vel|^2 leaves f32's range (|rel_vel| < ~1e-19 m/s; the reference's f64 gets there at 1e-162)
// rcp(a) is +inf and a pair that does not overlap (c > 0) comes out as +inf whichever way it moves: the
// collision the reference would compute lies more than 2^51 fixed units of time (years) ahead, and the
// force term it would set is below 1e-17 N.  Overlapping pairs do not go through here alone: ttc_pair_f32.
__device__ __forceinline__ float ttc_core_c_f32(float rvx, float rvy, float rpx, float rpy, float c) {
  const float a = __builtin_fmaf(rvx, rvx, rvy * rvy);
  const float bh = __builtin_fmaf(rvx, rpx, rvy * rpy);
  const float disc = __builtin_fmaf(bh, bh, -(a * c));
  const float root = fast_sqrt(disc);
  const float ia = fast_rcp(a);
  const float t0 = (-bh - root) * ia;
  const float t1 = (-bh + root) * ia;
  return ttc_select(t0, t1);
}
__device__ __forceinline__ float ttc_core_f32(float rvx, float rvy, float rpx, float rpy, float d2,
                                              float R2) {
  return ttc_core_c_f32(rvx, rvy, rpx, rpy, d2 - R2);
}

// ttc_core_c_f32 up to its discriminant, for a pass that finishes only the pairs whose result can be finite (the lean
// time-to-collision pass of k_step_tiled; DESIGN.md section 4 has the proof).  The SIGN BIT of the key is set only if
//   disc < 0   or   disc == 0 and bh == 0,
// and for exactly these ttc_core_c_f32 returns +inf whatever the 1-ulp v_sqrt_f32 / v_rcp_f32 return: the root of a
// negative number is NaN, so t0 and t1 are NaN; the root of +-0 is +-0, so t1 = (-bh + root) * ia is +-0 or NaN; either
// way `t1 > 0` fails.  Same a, bh and disc as there, operation for operation.  s = disc + |bh| is negative only for
// disc < -|bh| <= 0 and zero only for disc = -|bh| (a +0 then: |bh| is never -0), so s <= 0 implies the above; bits(s) - 1
// turns "s < 0 or s == +0" into one sign bit (+0 wraps around to 0xFFFFFFFF).  The test is
// conservative: a pair with -|bh| < disc < 0 is finished although it would come out as +inf.  A NaN counts by its sign
// bit: with a NaN discriminant the root is NaN and the result +inf like for a negative one.
__device__ __forceinline__ uint32_t ttc_skip_key(float rvx, float rvy, float rpx, float rpy, float c) {
  const float a = __builtin_fmaf(rvx, rvx, rvy * rvy);
  const float bh = __builtin_fmaf(rvx, rpx, rvy * rpy);
  const float disc = __builtin_fmaf(bh, bh, -(a * c));
  return __float_as_uint(disc + __builtin_fabsf(bh)) - 1u;
}

// max(|rvx|, |rvy|) as ordered bits minus one: < TTC_TINY_KEY exactly when 0 < |rv|_max < 1e-12,
// the range that takes ttc_tiny_f32 in the guarded form (zero wraps around to the largest key).
#define TTC_TINY_KEY (0x2B8CBCCCu - 1u) /* bits of 1e-12f, minus one */
__device__ __forceinline__ uint32_t ttc_tiny_key(float rvx, float rvy) {
  return __float_as_uint(fmaxf(fabsf(rvx), fabsf(rvy))) - 1u;
}

// HUGE relative velocities: positions are in fixed units (|rp'| up to 2^25), so bh = rv . rp' leaves f32's range
// in bh^2 from |rel_vel| ~ 5e11 m/s on, where the metre-valued quadratic of the reference has room up to 2e18.  The
// model's own clamp throws agents at 1e15 m/s (zanlungo.rs:165-167), and whoever sees such an agent in the next
// step has a time to collision of 1e-15 s with it: the reference's cascade.  Such pairs are scaled DOWN by 2^-40
// (the same exact rescaling as the tiny ones).  Threshold 2^32 m/s per component.
#define TTC_HUGE_SPEED 0x1p32f
__device__ __forceinline__ bool ttc_huge(float rvx, float rvy) { return fmaxf(fabsf(rvx), fabsf(rvy)) >= TTC_HUGE_SPEED; }

// the guarded form: tiny relative velocities rescaled up (what still underflows: the a -> 0 limit), huge ones down
__device__ __forceinline__ float ttc_f32(float rvx, float rvy, float rpx, float rpy, float d2,
                                         float R2) {
  if (__builtin_expect(ttc_tiny_key(rvx, rvy) < TTC_TINY_KEY, 0))
    return ttc_tiny_f32(rvx, rvy, rpx, rpy, d2, R2, 0x1p48f);
  if (__builtin_expect(ttc_huge(rvx, rvy), 0)) return ttc_tiny_f32(rvx, rvy, rpx, rpy, d2, R2, 0x1p-40f);
  return ttc_core_f32(rvx, rvy, rpx, rpy, d2, R2);
}

// THE time to collision of a pair, in every neighbour kernel: the plain quadratic, and the guarded form
// for pairs that overlap (0 < d2 <= R2), whose answer ("colliding now", t = 0: zanlungo.rs:61-73 with
// t0 < 0 < t1) must not depend on whether |rel_vel|^2 is representable, and for pairs whose relative velocity is
// huge (an agent the model has thrown: ttc_huge), whose bh^2 would overflow in fixed units.  (d2 == 0, two agents in one
// place, stays with the plain form: the tiled kernel keeps the agent itself on its list, and the plain
// form answers 0 for any |rel_vel| above 1e-19 m/s.)  The hot loops compute the plain form for every
// pair and collect the smallest overlap key; an agent (a wave) that saw an overlapping pair repeats its
// pass with this function, which gives the other pairs the values they had.
// overlap key: the bits of d2 minus one, as an ordered integer: < bits(R2) exactly when 0 < d2 <= R2
// (zero wraps around to the largest key; NaN is larger than any R2).
__device__ __forceinline__ uint32_t ttc_overlap_key(float d2) { return __float_as_uint(d2) - 1u; }
__device__ __forceinline__ float ttc_pair_f32(float rvx, float rvy, float rpx, float rpy, float d2,
                                              float R2) {
  if (__builtin_expect(ttc_overlap_key(d2) < __float_as_uint(R2) || ttc_huge(rvx, rvy), 0))
    return ttc_f32(rvx, rvy, rpx, rpy, d2, R2);
  return ttc_core_c_f32(rvx, rvy, rpx, rpy, d2 - R2);
}

// What every force term of one agent shares (zanlungo.rs:93-170 with weight = 2):
//   fut = v_i * t_i,  mag = min(1e15, 2 * A * |v_i| / t_i),  k = log2(e) / D
// Lengths in FIXED units (see UNITS above): fut' = S fut, two_R' = S 2R, k_exp' = k_exp / S.
struct ForceCtx {
  float vix, viy, futx, futy, mag, two_R, k_exp;
};

// Ts = S t_i, as the time-to-collision functions return it for positions in fixed units
__device__ __forceinline__ ForceCtx make_force_ctx(float vix, float viy, float Ts, const GroupDev& grp, const GridDev& g) {
  ForceCtx c;
  c.vix = vix;
  c.viy = viy;
  c.futx = vix * Ts;
  c.futy = viy * Ts;
  const float T = Ts * g.fix_inv;  // seconds (exact: a power of two)
  // weight * agent_scale * |my_vel - other_vel| / t_i with weight 2, other_vel 0; once per agent,
  // so the exact division is kept (t_i == 0 -> +inf -> clamped, zanlungo.rs:165-167)
  float speed = sqrtf(__builtin_fmaf(vix, vix, viy * viy));
  // t_i == 0 divides by zero: +-inf (clamped) for any speed but 0, NaN for 0.  Below 1e-19 m/s the squares
  // underflow in f32 where the reference's f64 still has a speed; only "zero or not" matters there.
  if (Ts == 0.0f && speed == 0.0f) speed = fmaxf(fabsf(vix), fabsf(viy));
  float mag = 2.0f * grp.A * speed / T;
  c.mag = (mag >= 1e15f) ? 1e15f : mag;
  c.two_R = grp.R * 2.0f * g.fix_scale;
  c.k_exp = 1.44269504088896341f / grp.D * g.fix_inv;
  return c;
}

// The radius test of the neighbour pass on p_j - p_i = (ax, ay) in fixed units, nr2 = -(S eyesight)^2:
// in sight (strict `<`, location_hash_2d.rs:251) exactly when the result is negative.  The result is
// never -0 (ax, ay are integers) and not NaN unless the eyesight is; the LDS-tiled kernel reads its
// sign bit, the others compare with 0.
__device__ __forceinline__ float sight_margin(float ax, float ay, float nr2) {
  return __builtin_fmaf(ax, ax, __builtin_fmaf(ay, ay, nr2));
}

// "some active lane": one compare and a scalar test (HIP's __any goes through a select and a second compare)
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
// a wave-uniform value held in a vector register (see the fast form of k_step_tiled)
__device__ __forceinline__ uint32_t in_vgpr(uint32_t x) {
  uint32_t v;
  asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
  return v;
}

// LDS addresses as plain 32-bit integers (the tiled kernel's list entries ARE such addresses, and its
// hot loops advance them with full-rate v_add_u32 instead of the compiler's v_lshl_add / v_mad)
#define CS_LDS __attribute__((address_space(3)))
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(CS_LDS const char*)p; }
typedef int cs_v4i __attribute__((ext_vector_type(4)));
typedef int cs_v2i __attribute__((ext_vector_type(2)));
typedef float cs_v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int4 lds_ld_i4(uint32_t a) {
  const cs_v4i v = *(CS_LDS const cs_v4i*)(uintptr_t)a;
  return make_int4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ int2 lds_ld_i2(uint32_t a) {
  const cs_v2i v = *(CS_LDS const cs_v2i*)(uintptr_t)a;
  return make_int2(v.x, v.y);
}
__device__ __forceinline__ float2 lds_ld_f2(uint32_t a) {
  const cs_v2f v = *(CS_LDS const cs_v2f*)(uintptr_t)a;
  return make_float2(v.x, v.y);
}
__device__ __forceinline__ uint32_t lds_ld_u32(uint32_t a) { return *(CS_LDS const uint32_t*)(uintptr_t)a; }
__device__ __forceinline__ uint32_t lds_ld_u16(uint32_t a) { return *(CS_LDS const unsigned short*)(uintptr_t)a; }
__device__ __forceinline__ void lds_st_u16(uint32_t a, uint32_t v) { *(CS_LDS unsigned short*)(uintptr_t)a = (unsigned short)v; }

// Force on agent i from a neighbour j with the LARGER id (weight = 2 branch of
// compute_agent_force, zanlungo.rs:93-170, with right_of_way_vel :173-198 and slerp :23-28
// folded for the state the reference actually produces: a neighbour's preferred_vel is
// always (0,0) (lib.rs:140,261,271: it is set on the per-iteration clone only), so
// other_vel = v_j + 1*(0 - v_j) = 0 and the "stationary" branch :119-125 is the live one;
// slerp(1, d, perp, s) = d*(sin(0)/s) + perp*(sin(asin s)/s) = d*0 + perp*1 for s > 0 and NaN
// for s == 0, and the normalize() that follows removes the factor sin(asin s)/s = 1 +- 1 ulp).
// |perp| = |rp|, so the unit vector is perp * rsqrt(d2).   rp = p_j - p_i, d2 = |rp|^2, both in the
// fixed units of the context (the factors S cancel: perp' rsqrt(d2') = perp rsqrt(d2)).
__device__ __forceinline__ void zanlungo_forward_force(float rpx, float rpy, float d2,
                                                       const ForceCtx& c, float& fx, float& fy) {
  const float dx = c.futx - rpx, dy = c.futy - rpy;  // (p_i + v_i T) - (p_j + 0 T)
  const float dist = fast_sqrt(__builtin_fmaf(dx, dx, dy * dy));
  float px = rpy, py = -rpx;  // perp of q = p_i - p_j = -rp: (-q.y, q.x)
  const bool flip = __builtin_fmaf(px, c.vix, py * c.viy) < 0.0f;
  px = flip ? -px : px;
  py = flip ? -py : py;
  const float s = fabsf(__builtin_fmaf(px, dy, -(py * dx)));
  // s > 1 clamps to 1 and drops out; s == 0 or NaN poisons the direction (0/0)
  const float inv_n = (s > 0.0f) ? fast_rsq(d2) : f_nan();
  const float scale = c.mag * fast_exp2((c.two_R - dist) * c.k_exp) * inv_n;
  fx = __builtin_fmaf(px, scale, fx);
  fy = __builtin_fmaf(py, scale, fy);
}

// v_exp_f32 (fast_exp2) returns +0 for every input at or below -ZAN_EXP2_ZERO.  It flushes results below 2^-126 to +0 in
// the kernels' denormal mode (the engine is built without -ffast-math: f32 denormals on); an exhaustive sweep on gfx950
// found +0 for every input below -126 and the smallest non-zero result at -126 (tools/exp2_underflow.hip).  160 keeps
// the test right even for an exp2 that returned denormals: 2^-160 lies far below half the smallest one, 2^-150.
#define ZAN_EXP2_ZERO 160.0f

// The force pass's pre-test (k_step_tiled): true when every forward term of this agent whose direction is not NaN has
// fast_exp2(...) == +0 in zanlungo_forward_force, for any neighbour the lean filter can list (|rp| < |rs|, rs = S
// eyesight).  The kernel's per-entry check (forward_terms_vanish) takes the agent off the fast path if any forward entry
// has the NaN direction (s = +-0 or NaN), so the argument below may assume rp != 0 for every forward entry: rp is then a
// non-zero integer vector, |rp| >= 1.  Ts is the agent's t_i in fixed units, c its context, vanish2 the group's bound.
//   * The argument: dist >= Z / k_exp + max(two_R, 0) (Z = ZAN_EXP2_ZERO) with a relative margin of a few ulps gives
//     (two_R - dist) * k_exp <= -Z after both roundings (the subtraction and the product, 2^-24 each), for k_exp > 0
//     finite and normal and two_R finite.  An infinite dist (d2 overflowed) gives -inf, and exp2(-inf) = +0 too.
//   * dist >= |fut - rp| (1 - 2^-21): dx, dy (2^-24 each), dy * dy and the fma (2^-24 each), v_sqrt_f32 (1 ulp, 2^-23).
//     Nothing underflows: |fut - rp| >= 2^-12 |fut| >= 2^-12 (below, and |fut| > |rp| >= 1).
//   * |fut - rp| >= |fut| - |rp|, and a listed neighbour has |rp| < |rs| (1 + 2^-24) (sight_margin < 0 with nr2 rounded
//     once; the fmas only round the sign-correct result).
// So |fut| >= (|rs| + max(two_R, 0) + Z / k_exp) (1 + 2^-20) suffices.  The host computes b = that sum with rs, two_R
// and k_exp formed exactly as make_force_ctx forms them, in double, times (1 + 2^-10), and stores b^2 rounded up
// (GroupDev::vanish2; NaN unless k_exp is normal and finite, rs and two_R finite, and b^2 fits).  The kernel's one
// rounding, |fut|^2 (the product and the fma, under 2^-23), leaves whatever passes a margin of at least 2^-11.  fut is
// the very (futx, futy) the force reads, so its own rounding does not enter.  mag must be finite (mag * 0 = +-0), and
// 0 < t_i < inf.  A NaN anywhere fails a comparison: the agent is no candidate.
__device__ __forceinline__ bool zanlungo_forward_vanishes(const ForceCtx& c, float Ts, float vanish2) {
  const float fut2 = __builtin_fmaf(c.futx, c.futx, c.futy * c.futy);
  return Ts > 0.0f && Ts < f_inf() && fabsf(c.mag) < f_inf() && fut2 >= vanish2;
}
// GroupDev::vanish2 for a Zanlungo group (host side of zanlungo_forward_vanishes)
inline float zanlungo_vanish2(float eyesight, float R, float D, const GridDev& g) {
  const float k_exp = 1.44269504088896341f / D * g.fix_inv;  // as make_force_ctx
  const float rs = eyesight * g.fix_scale, two_R = R * 2.0f * g.fix_scale;
  if (!(k_exp >= 0x1p-126f && k_exp < HUGE_VALF && std::fabs(rs) < HUGE_VALF && std::fabs(two_R) < HUGE_VALF))
    return std::nanf("");
  const double b = ((double)std::fabs(rs) + std::max((double)two_R, 0.0) + (double)ZAN_EXP2_ZERO / (double)k_exp) *
                   (1.0 + 0x1p-10);
  const float b2 = std::nextafter((float)(b * b), HUGE_VALF);  // (rounded up)
  return b2 < HUGE_VALF ? b2 : std::nanf("");
}

// RMFPlanner::route_plans_by_location (rmf/mod.rs:90) on the device: an open-addressing table of
// (planner, SpatialHash(start), SpatialHash(goal)) -> route + 1, built on the host whenever a route
// is added (the host plans: A* is its business), searched by the step kernel when an agent reaches
// a waypoint of its source-sink (set_target, lib.rs:325-333 -> rmf/mod.rs:217-222).
struct RouteBookEntry {
  long long sx, sy, gx, gy;
  uint32_t hlp, route1;  // route1 == 0: empty slot
};
__host__ __device__ inline long long route_spatial_hash(double v, double res) {  // SpatialHash::new, rmf/mod.rs:70-77
  const double r = round(v / res);
  if (r != r) return 0;
  if (r >= 9.2e18) return 0x7FFFFFFFFFFFFFFFll;
  if (r <= -9.2e18) return (long long)0x8000000000000000ull;
  return (long long)r;
}
__host__ __device__ inline uint32_t route_book_slot(uint32_t hlp, long long sx, long long sy, long long gx, long long gy) {
  unsigned long long h = 0x9E3779B97F4A7C15ull * (unsigned long long)(hlp + 1u);
  h = (h ^ (unsigned long long)sx) * 0xBF58476D1CE4E5B9ull;
  h = (h ^ (unsigned long long)sy) * 0x94D049BB133111EBull;
  h = (h ^ (unsigned long long)gx) * 0xBF58476D1CE4E5B9ull;
  h = (h ^ (unsigned long long)gy) * 0x94D049BB133111EBull;
  return (uint32_t)(h >> 32);
}
__device__ __forceinline__ uint32_t route_book_find(const RouteBookEntry* __restrict__ book, uint32_t mask,
                                                    uint32_t hlp, long long sx, long long sy, long long gx,
                                                    long long gy) {
  if (!book) return 0u;
  uint32_t k = route_book_slot(hlp, sx, sy, gx, gy) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const RouteBookEntry e = book[k];
    if (e.route1 == 0u) return 0u;
    if (e.hlp == hlp && e.sx == sx && e.sy == sy && e.gx == gx && e.gy == gy) return e.route1;
    k = (k + 1u) & mask;
  }
  return 0u;
}

struct StepParams {
  GridDev g;
  float dt;
  uint32_t n;  // slots in the sorted arrays (upper bound of alive)
  uint32_t has_sinks;
  uint32_t n_src_cells;  // 0 when no sources are binned
  // The windows along a tile's edges ran as a launch of their own and the halo exchange may already
  // be reading what they packed: an agent of THIS (interior) launch that lands in the halo band
  // came from more than a cell away and would miss the exchange (counted in n_halo_late, an error)
  uint32_t halo_late_check;
  // tile engines: the number of this step, stored with n_alive in pinned host memory by the step
  // kernel's first thread (EpilogueCtx::peek): the host's slot bound follows without a copy or a wait
  uint32_t peek_seq;
};

// Re-bin after integration: the reference's location_to_index
// (location_hash_2d.rs:54-66) on a cell-relative position.  Negative
// coordinates saturate to row/column 0, y beyond the stride aliases into the
// next row, flat >= len is "Index out of bounds".
__device__ __forceinline__ uint32_t rebin(const GridDev& g, uint32_t gx, uint32_t gy, float& ox,
                                          float& oy, Counters* ctr) {
  float kxf = floorf(ox * g.inv_cs), kyf = floorf(oy * g.inv_cs);
  if (kxf == 0.0f && kyf == 0.0f) return gx * g.nx + gy;  // fast path: same cell
  bool nanx = !(ox == ox), nany = !(oy == oy);
  // NaN as usize = 0 (saturating cast): binned into row/column 0, offset stays NaN
  long long cx = nanx ? 0 : (long long)gx + (long long)fminf(fmaxf(kxf, -4e9f), 4e9f);
  long long cy = nany ? 0 : (long long)gy + (long long)fminf(fmaxf(kyf, -4e9f), 4e9f);
  bool clamp_x = false, clamp_y = false;
  if (cx < 0) {
    cx = 0;
    clamp_x = !nanx;
  }
  if (cy < 0) {
    cy = 0;
    clamp_y = !nany;
  }
  if (clamp_x || clamp_y) atomicAdd(&ctr->n_clamped, 1u);
  unsigned long long flat = (unsigned long long)cx * g.nx + (unsigned long long)cy;
  // A tile has real neighbours behind its shared edges: what leaves the local rectangle there (more than a
  // ghost ring in one step) is an error.  Along the DOMAIN's own low edges (local row / column 0 is global
  // row / column 0: org == 0) the reference's saturating cast applies as on a single engine (location_hash_2d.rs:
  // 54-66): the agent is binned into row / column 0 and keeps its exact position.  The alias of y beyond the
  // stride (a move into another x row, i.e. generally another tile) stays an error on a tile.
  const bool tile_strict = g.tile && ((clamp_x && g.org_x != 0u) || (clamp_y && g.org_y != 0u) || cy >= (long long)g.nx);
  if (flat >= g.ncells || tile_strict) {
    atomicAdd(&ctr->n_out_of_bounds, 1u);
    return CS_INVALID_CELL;
  }
  // geometric coordinates of the STORED cell (differ from (cx,cy) when aliased)
  uint32_t sx = (uint32_t)cx, sy = (uint32_t)cy;
  if (cy >= g.nx) {
    sx = (uint32_t)(flat / g.nx);
    sy = (uint32_t)(flat % g.nx);
  }
  float mx = (float)((long long)sx - (long long)gx), my = (float)((long long)sy - (long long)gy);
  ox = (ox - mx * g.cs) - mx * g.cs_lo;
  oy = (oy - my * g.cs) - my * g.cs_lo;
  return (uint32_t)flat;
}

// Source occupancy for the next spawn phase: the reference asks the index for
// agents within 0.4 of each source (lib.rs:212-217); here every agent marks the
// sources it blocks.  Sources are binned once on the host (src_cell_start /
// src_sorted, same cell order as the agents).
__device__ __forceinline__ void mark_sources(const GridDev& g, const SinkDev* __restrict__ sinks,
                                             const uint32_t* __restrict__ src_cell_start,
                                             const uint32_t* __restrict__ src_sorted,
                                             uint32_t* __restrict__ src_occupied, uint32_t cell,
                                             float ox, float oy) {
  const float r = (float)CS_SPAWN_OCCUPANCY_RADIUS;
  if (!(fabsf(ox) < 1e6f * g.cs && fabsf(oy) < 1e6f * g.cs)) return;  // NaN / far outside
  const uint32_t sx = cell / g.nx, sy = cell - sx * g.nx;
  long long lx = (long long)sx + (long long)floorf((ox - r) * g.inv_cs - 1e-4f);
  long long hx = (long long)sx + (long long)floorf((ox + r) * g.inv_cs + 1e-4f);
  long long ly = (long long)sy + (long long)floorf((oy - r) * g.inv_cs - 1e-4f);
  long long hy = (long long)sy + (long long)floorf((oy + r) * g.inv_cs + 1e-4f);
  lx = max(lx, 0ll); ly = max(ly, 0ll);
  // get_bounds / signed_idx_to_data_idx (location_hash_2d.rs:74-122) clamp nothing: negative
  // indices and flat >= len are rejected, that is all.  x runs over the grid's rows (len / stride of
  // them: more than the stride on a grid taller than wide), y over one row's cells; y beyond the
  // stride would alias into the next row, where the distance test below rejects everything.
  const long long x_last = (long long)(g.ncells / g.nx) - 1;
  hx = min(hx, x_last); hy = min(hy, (long long)g.nx - 1);
  for (long long cx = lx; cx <= hx; ++cx) {
    for (long long cy = ly; cy <= hy; ++cy) {
      unsigned long long flat = (unsigned long long)cx * g.nx + (unsigned long long)cy;
      if (flat >= g.ncells) continue;
      uint32_t b = src_cell_start[flat], e = src_cell_start[flat + 1];
      for (uint32_t k = b; k < e; ++k) {
        uint32_t slot = src_sorted[k];
        float qx = (float)(cx - (long long)sx) * g.cs + (sinks[slot].src_ox - ox);
        float qy = (float)(cy - (long long)sy) * g.cs + (sinks[slot].src_oy - oy);
        if (sqrtf(qx * qx + qy * qy) < r) src_occupied[slot] = 1u;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Halo records of a tile (K7, DESIGN.md "Tiles").  A record is what a neighbour tile needs to see
// an agent: cell-relative state + its GLOBAL cell.  Ownership is decided by cell alone, so
// migrants and ghosts travel the same way: everything within 2*halo cells of a shared edge (the
// ghost ring itself holds the agents that just walked out) is sent.
// Buffer layout: record 0 is the header (word 0 = record count, word 1 = the sender's Counters::mesh_fail_step), records follow.
// ---------------------------------------------------------------------------
struct HaloRecord {
  float ox, oy, vx, vy;
  uint32_t id, meta, gcx, gcy;
  uint32_t route, reserved;  // CS_HLP_ROUTE: the agent_cache entry (route + 1 | waypoint << 22) travels along
};
static_assert(sizeof(HaloRecord) == CS_HALO_RECORD_BYTES, "halo record layout");

__device__ __forceinline__ void halo_append(HaloRecord* __restrict__ buf, uint32_t cap, const HaloRecord& r,
                                            Counters* ctr) {
  uint32_t k = atomicAdd(reinterpret_cast<uint32_t*>(buf), 1u);
  if (k < cap) buf[k + 1] = r;
  else atomicAdd(&ctr->n_halo_overflow, 1u);
}

// One-phase exchange: all eight neighbours at once.  dir: 0 XLO, 1 XHI, 2 YLO, 3 YHI, 4 XLO_YLO,
// 5 XLO_YHI, 6 XHI_YLO, 7 XHI_YHI.
struct HaloBuffers8 {
  HaloRecord* p[8];
  uint32_t cap[8];  // records each buffer holds (edges are long, corners a handful of cells)
};


// cell c of the local grid lies within `band` cells of an edge
__device__ __forceinline__ bool halo_in_band(const GridDev& g, uint32_t band, uint32_t c) {
  const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
  const uint32_t rows = g.ncells / g.nx;
  return cx < band || cx + band >= rows || cy < band || cy + band >= g.nx;
}

// ... of an edge BEHIND WHICH A NEIGHBOUR TILE LIVES (the check of the interior launch: along the
// domain's own edges nobody waits for records)
__device__ __forceinline__ bool halo_in_shared_band(const GridDev& g, uint32_t band, const HaloBuffers8& send, uint32_t c) {
  const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
  const uint32_t rows = g.ncells / g.nx;
  return (cx < band && send.p[0]) || (cx + band >= rows && send.p[1]) || (cy < band && send.p[2]) ||
         (cy + band >= g.nx && send.p[3]);
}

// One live agent -> the send buffers of the (up to three) neighbours whose ring or ownership its
// cell falls into.  Called by k_halo_pack_all for every agent of the unsorted arrays, and by the
// step kernels' epilogue for the agent they have just moved (then no pack launch is needed).
// The lanes of a wave that append to the same buffer share ONE atomic on its record count (a
// border window's agents all go to the same one or two buffers).  Every lane that calls this must
// do so at the same point of the program (ballots over the active lanes).
__device__ __forceinline__ void halo_pack_agent(const GridDev& g, uint32_t band, const HaloBuffers8& send,
                                                uint32_t c, float ox, float oy, float vx, float vy, uint32_t id,
                                                uint32_t meta, uint32_t route, Counters* ctr) {
  const uint32_t cx = c / g.nx, cy = c - cx * g.nx;
  const uint32_t rows = g.ncells / g.nx;
  const bool xl = cx < band, xh = cx + band >= rows, yl = cy < band, yh = cy + band >= g.nx;
  if (!__any(xl || xh || yl || yh)) return;
  HaloRecord r;
  r.ox = ox; r.oy = oy; r.vx = vx; r.vy = vy;
  r.id = id;
  r.meta = meta;
  r.gcx = g.org_x + cx;
  r.gcy = g.org_y + cy;
  r.route = route;
  r.reserved = 0u;
  const int lane = __lane_id();
  const bool want[8] = {xl, xh, yl, yh, xl && yl, xl && yh, xh && yl, xh && yh};
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    if (!send.p[d]) continue;  // no neighbour on that side (wave-uniform)
    const unsigned long long m = __ballot(want[d]);
    if (!m) continue;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(reinterpret_cast<uint32_t*>(send.p[d]), (uint32_t)__popcll(m));
    base = __shfl(base, leader, 64);
    if (want[d]) {
      const uint32_t k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (k < send.cap[d]) send.p[d][k + 1] = r;
      else atomicAdd(&ctr->n_halo_overflow, 1u);
    }
  }
}
