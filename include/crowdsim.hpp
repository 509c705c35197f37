// crowdsim.hpp — C++ host-side mirror of the reference's trait surface over the C ABI.
//
// Same names, argument order and error behaviour as rmf_crowdsim (paths relative to
// rmf_crowdsim/src in the reference tree); Result<_, String> becomes std::runtime_error(message).
//   Simulation            lib.rs:69-383            EventListener     lib.rs:22-33
//   HighLevelPlanner      highlevel_planners/highlevel_planners.rs:8-16
//   LocalPlanner / Zanlungo / NoLocalPlan   local_planners/{local_planner,zanlungo,no_local_plan}.rs
//   LocationHash2D        spatial_index/location_hash_2d.rs:33-51
//   SourceSink / CrowdGenerator / MonotonicCrowd / PoissonCrowd   source_sink/source_sink.rs:30-101
// Header-only; link against libcrowdstep_hip.so (the HIP engine).  There is no CPU path.
#ifndef CROWDSIM_HPP
#define CROWDSIM_HPP

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <map>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "crowdstep.h"
#include "crowdstep_state.h"

namespace rmf_crowdsim {

using AgentId = std::size_t;  // lib.rs:36
struct Vec2f {               // lib.rs:40-43 (nalgebra Vector2<f64>)
  double x = 0, y = 0;
};
using Point = Vec2f;

struct Agent {  // lib.rs:46-65
  AgentId agent_id = 0;
  Point position;
  double orientation = 0;
  Vec2f velocity;
  double angular_vel = 0;
  std::size_t next_waypoint = 0;
  double eyesight_range = 0;
};

// one record of write_agents (include/crowdstep_state.h): the fields of `a` that a write can set (eyesight_range is
// carried along and ignored; orientation and angular_vel are not writable)
inline cs_agent_view agent_view_of(const Agent& a) {
  cs_agent_view v{};
  v.id = a.agent_id;
  v.x = a.position.x;
  v.y = a.position.y;
  v.vx = a.velocity.x;
  v.vy = a.velocity.y;
  v.next_waypoint = a.next_waypoint;
  v.eyesight_range = a.eyesight_range;
  return v;
}
// ... and the Agent of one record that a read returned (cs_read_agents, cs_read_agents_by_id)
inline Agent agent_of_view(const cs_agent_view& v) {
  Agent a;
  a.agent_id = v.id;
  a.position = {v.x, v.y};
  a.velocity = {v.vx, v.vy};
  a.next_waypoint = v.next_waypoint;
  a.eyesight_range = v.eyesight_range;
  return a;
}
constexpr uint32_t kWriteAll = CS_WRITE_POSITION | CS_WRITE_VELOCITY | CS_WRITE_NEXT_WAYPOINT;

struct EventListener {  // lib.rs:22-33
  virtual ~EventListener() = default;
  virtual void agent_spawned(Vec2f position, AgentId agent) = 0;
  virtual void agent_destroyed(AgentId agent) = 0;
  virtual void waypoint_reached(Vec2f, AgentId) {}
};

struct LocationHash2D;
// trait SpatialIndex, spatial_index.rs:4-14: what Simulation<T: SpatialIndex> (lib.rs:69) is generic over.  On this
// backend the index IS the neighbour kernel (the engine keeps the agents in a LocationHash2D's cell order and answers the
// trait's four calls itself), so an index has to describe itself as such a grid: device_form() returns the LocationHash2D
// it is equivalent to, or null, in which case Simulation's constructor throws.  No host-side slow path for a foreign
// index exists (a per-agent host query per step would put the hot path on the CPU).
struct SpatialIndex {
  virtual ~SpatialIndex() = default;
  virtual const LocationHash2D* device_form() const { return nullptr; }
};
struct LocationHash2D : SpatialIndex {  // location_hash_2d.rs:33
  double width, height, cell_size;
  Point offset;
  LocationHash2D(double w, double h, double cell, Point off) : width(w), height(h), cell_size(cell), offset(off) {}
  const LocationHash2D* device_form() const override { return this; }
};

// highlevel_planners.rs:8-16.  Override get_desired_velocity for a host planner (batched
// callback, slow path), or use the data planners below, which the device evaluates.
struct HighLevelPlanner {
  virtual ~HighLevelPlanner() = default;
  virtual bool get_desired_velocity(const Agent&, std::chrono::duration<double>, Vec2f*) { return false; }
  virtual void set_target(const Agent&, Point, Vec2f) {}
  virtual void remove_agent_id(AgentId) {}
  virtual cs_hlp_desc describe() {
    cs_hlp_desc d{};
    d.kind = CS_HLP_CALLBACK;
    d.user = this;
    d.velocity = [](void* u, size_t n, const uint64_t* ids, const double* pos, const double* vel, double t,
                    double* out, uint8_t* some) {
      auto* self = static_cast<HighLevelPlanner*>(u);
      for (size_t i = 0; i < n; ++i) {
        Agent a;
        a.agent_id = ids[i];
        a.position = {pos[2 * i], pos[2 * i + 1]};
        a.velocity = {vel[2 * i], vel[2 * i + 1]};
        Vec2f v;
        some[i] = self->get_desired_velocity(a, std::chrono::duration<double>(t), &v) ? 1 : 0;
        out[2 * i] = v.x;
        out[2 * i + 1] = v.y;
      }
    };
    d.set_target = [](void* u, uint64_t id, double px, double py, double tx, double ty, double ox, double oy) {
      Agent a;
      a.agent_id = id;
      a.position = {px, py};
      static_cast<HighLevelPlanner*>(u)->set_target(a, {tx, ty}, {ox, oy});
    };
    d.remove_agent = [](void* u, uint64_t id) { static_cast<HighLevelPlanner*>(u)->remove_agent_id(id); };
    return d;
  }
  // how a Simulation / a TiledSimulation registers the planner: by its descriptor, unless the planner has a call of its own
  virtual uint32_t register_with(cs_engine* e) {
    cs_hlp_desc d = describe();
    return cs_register_hlp(e, &d);
  }
  virtual uint32_t register_with(cs_mesh* m) {
    cs_hlp_desc d = describe();
    return cs_mesh_register_hlp(m, &d);
  }
};
struct StubHighLevelPlan : HighLevelPlanner {  // lib.rs:391-420: Some(default_vel)
  Vec2f default_vel;
  explicit StubHighLevelPlan(Vec2f v) : default_vel(v) {}
  cs_hlp_desc describe() override {
    cs_hlp_desc d{};
    d.kind = CS_HLP_CONSTANT;
    d.vx = default_vel.x;
    d.vy = default_vel.y;
    return d;
  }
};
struct IdParityHighLevelPlan : StubHighLevelPlan {  // rmf_crowdsim_viz/src/main.rs:20-30
  using StubHighLevelPlan::StubHighLevelPlan;
  cs_hlp_desc describe() override {
    cs_hlp_desc d = StubHighLevelPlan::describe();
    d.kind = CS_HLP_ID_PARITY;
    return d;
  }
};
// One flow-field solve (cs_flow_field_solve, include/crowdstep_state.h, "Solving a flow field on the device"): goals and
// blocked hold nx * ny bytes (blocked may be empty: no walls), slowness nx * ny floats (empty: 1 everywhere), bin (ix, iy)
// at iy * nx + ix.  A step out of a bin costs its length times slowness * (1 + density_weight * the agents in the bin).
struct FlowProblem {
  cs_field_desc raster{};
  std::vector<uint8_t> goals, blocked;
  std::vector<float> slowness;
  double speed = 1.0, density_weight = 0.0;
  const cs_selection* density_filter = nullptr;
  cs_flow_desc desc() const {
    const std::size_t bins = (std::size_t)raster.nx * raster.ny;
    if (goals.size() != bins || (!blocked.empty() && blocked.size() != bins) || (!slowness.empty() && slowness.size() != bins))
      throw std::runtime_error("FlowProblem: goals, blocked and slowness hold nx * ny values (or none)");
    cs_flow_desc d{};
    d.raster = raster;
    d.goals = goals.data();
    d.blocked = blocked.empty() ? nullptr : blocked.data();
    d.slowness = slowness.empty() ? nullptr : slowness.data();
    d.speed = speed;
    d.density_weight = density_weight;
    d.density_filter = density_filter;
    return d;
  }
};
// ... and what it returns: the vectors (nx * ny pairs; NaN at blocked and unreachable bins) and the distances (+inf there),
// each empty unless asked for; the bins with a path to a goal; the rounds the device ran.
struct FlowField {
  uint32_t nx = 0, ny = 0;
  std::vector<float> vxy;
  std::vector<double> dist;
  uint64_t reached = 0;
  uint32_t rounds = 0;
};
template <class Handle, class Call, class Why>
inline FlowField flow_solve_call(Handle* h, Call call, Why why, const FlowProblem& p, uint32_t hlp, bool vectors, bool distance) {
  const cs_flow_desc d = p.desc();
  FlowField f;
  f.nx = p.raster.nx;
  f.ny = p.raster.ny;
  const std::size_t bins = (std::size_t)f.nx * f.ny;
  if (vectors) f.vxy.assign(2 * bins, 0.0f);
  if (distance) f.dist.assign(bins, 0.0);
  cs_flow_stats st{};
  if (call(h, &d, hlp, vectors ? f.vxy.data() : nullptr, distance ? f.dist.data() : nullptr, &st) != 0)
    throw std::runtime_error(why(h));
  f.reached = st.reached;
  f.rounds = st.rounds;
  return f;
}
// A navigation (flow) field: a raster of preferred velocities sampled at the agent's position ON THE DEVICE every step
// (cs_register_hlp_field, include/crowdstep_state.h: no host call and no wait in a step).  raster: the cs_field_desc of
// agent_field; vxy: nx * ny pairs (vx, vy), bin (ix, iy) at iy * nx + ix; a NaN bin is a wall.  update() replaces the
// values in every simulation the planner is registered with (they must still be alive); steps already queued keep the
// old ones.  get_desired_velocity restates the rule for a host that wants to ask the planner itself (bit for bit the
// device's when this header is compiled without floating-point contraction).
struct FieldPlanner : HighLevelPlanner {
  cs_field_desc raster;
  uint32_t sampling;
  std::vector<float> vxy;
  FieldPlanner(const cs_field_desc& r, std::vector<float> values, uint32_t how = CS_HLP_FIELD_NEAREST)
      : raster(r), sampling(how), vxy(std::move(values)) {
    if (vxy.size() != 2 * (std::size_t)r.nx * r.ny) throw std::runtime_error("FieldPlanner: vxy holds nx * ny pairs");
  }
  void update(const std::vector<float>& values) {
    if (values.size() != vxy.size()) throw std::runtime_error("FieldPlanner: update keeps the raster: nx * ny pairs");
    vxy = values;
    for (auto& b : engines_)
      if (cs_hlp_field_update(b.first, b.second, vxy.data()) != 0) throw std::runtime_error(cs_last_error(b.first));
    for (auto& b : meshes_)
      if (cs_mesh_hlp_field_update(b.first, b.second, vxy.data()) != 0) throw std::runtime_error(cs_mesh_last_error(b.first));
  }
  // Solve the flow field of `p` (whose raster is this planner's) on the device and write it into this planner's samples
  // in every simulation it is registered with: behind the steps already queued, in front of the next.  With vectors and
  // distance both false no raster crosses the bus.  The host's copy `vxy` follows when the vectors are asked for.
  FlowField solve(const FlowProblem& p, bool vectors = true, bool distance = false) {
    if (engines_.empty() && meshes_.empty()) throw std::runtime_error("FieldPlanner::solve: registered with no simulation yet");
    FlowField f;
    for (auto& b : engines_) f = flow_solve_call(b.first, cs_flow_field_solve, cs_last_error, p, b.second, vectors, distance);
    for (auto& b : meshes_) f = flow_solve_call(b.first, cs_mesh_flow_field_solve, cs_mesh_last_error, p, b.second, vectors, distance);
    if (vectors) vxy = f.vxy;
    return f;
  }
  // this planner's handle in an engine or a mesh, UINT32_MAX where it is not registered
  uint32_t handle_in(const cs_engine* e) const {
    for (auto& b : engines_)
      if (b.first == e) return b.second;
    return UINT32_MAX;
  }
  uint32_t handle_in(const cs_mesh* m) const {
    for (auto& b : meshes_)
      if (b.first == m) return b.second;
    return UINT32_MAX;
  }
  bool get_desired_velocity(const Agent& a, std::chrono::duration<double>, Vec2f* out) override {
    const cs_field_desc& d = raster;
    const double fx = (a.position.x - d.x0) / d.cell_w, fy = (a.position.y - d.y0) / d.cell_h;
    if (!(0.0 <= fx && fx < (double)d.nx && 0.0 <= fy && fy < (double)d.ny)) return false;
    const uint32_t ix = (uint32_t)fx, iy = (uint32_t)fy;
    auto sample = [&](uint32_t i, uint32_t j, int k) { return vxy[2 * ((std::size_t)j * d.nx + i) + k]; };
    auto nearest = [&]() {
      const float sx = sample(ix, iy, 0), sy = sample(ix, iy, 1);
      if (sx != sx || sy != sy) return false;
      *out = {(double)sx, (double)sy};
      return true;
    };
    if (sampling != CS_HLP_FIELD_BILINEAR) return nearest();
    auto axis = [](double f, uint32_t n, uint32_t* i0, uint32_t* i1, double* t) {
      const double ax = f - 0.5;
      if (ax < 0.0) {
        *i0 = *i1 = 0u;
        *t = 0.0;
        return;
      }
      *i0 = (uint32_t)ax;
      *t = ax - (double)*i0;
      *i1 = *i0 + 1u < n ? *i0 + 1u : n - 1u;
    };
    uint32_t i0, i1, j0, j1;
    double tx, ty, r[2];
    axis(fx, d.nx, &i0, &i1, &tx);
    axis(fy, d.ny, &j0, &j1, &ty);
    for (int k = 0; k < 2; ++k) {
      const double c00 = sample(i0, j0, k), c10 = sample(i1, j0, k), c01 = sample(i0, j1, k), c11 = sample(i1, j1, k);
      if (c00 != c00 || c10 != c10 || c01 != c01 || c11 != c11) return nearest();
      const double lo = c00 + (c10 - c00) * tx, hi = c01 + (c11 - c01) * tx;
      r[k] = (double)(float)(lo + (hi - lo) * ty);
    }
    *out = {r[0], r[1]};
    return true;
  }
  uint32_t register_with(cs_engine* e) override {
    const uint32_t h = cs_register_hlp_field(e, &raster, sampling, vxy.data());
    if (h == UINT32_MAX) throw std::runtime_error(cs_last_error(e));  // (refused: the raster or the sampling)
    engines_.emplace_back(e, h);
    return h;
  }
  uint32_t register_with(cs_mesh* m) override {
    const uint32_t h = cs_mesh_register_hlp_field(m, &raster, sampling, vxy.data());
    if (h != UINT32_MAX) meshes_.emplace_back(m, h);
    return h;
  }

 private:
  std::vector<std::pair<cs_engine*, uint32_t>> engines_;
  std::vector<std::pair<cs_mesh*, uint32_t>> meshes_;
};
// The follower half of RMFPlanner (rmf/mod.rs:195-242): override plan_route (the A* of
// rmf/mod.rs:160-192 is the host's business); it is asked once per new (start, goal) hash pair,
// following the route runs on the device.  An empty result = no contiguous path.
struct RouteFollower : HighLevelPlanner {
  double scale = 1.0, arrive = 0.1, speed = 1.0;
  virtual std::vector<Point> plan_route(Point start, Point goal) = 0;
  cs_hlp_desc describe() override {
    cs_hlp_desc d{};
    d.kind = CS_HLP_ROUTE;
    d.user = this;
    d.route_scale = scale;
    d.route_arrive = arrive;
    d.route_speed = speed;
    d.route_plan = [](void* u, double sx, double sy, double gx, double gy, double* out, size_t cap) -> size_t {
      const std::vector<Point> r = static_cast<RouteFollower*>(u)->plan_route({sx, sy}, {gx, gy});
      const size_t n = r.size() < cap ? r.size() : cap;
      for (size_t k = 0; k < n; ++k) {
        out[2 * k] = r[k].x;
        out[2 * k + 1] = r[k].y;
      }
      return n;
    };
    return d;
  }
};

// local_planner.rs:7-18.  The shipped planners (below) run on the device; any other subclass is host code:
// override get_desired_velocity and the engine evaluates it every step through its batched callback
// (cs_register_lp_callback: the slow path), with the agent and its neighbours as they were at the start of the step.
struct LocalPlanner {
  virtual ~LocalPlanner() = default;
  virtual Vec2f get_desired_velocity(const Agent& agent, const std::vector<Agent>& nearby_agents,
                                     Vec2f recommended_velocity) const {
    (void)agent; (void)nearby_agents;
    return recommended_velocity;
  }
  static int batch_thunk(void* u, size_t n, const cs_lp_agent* agents, const double* rec, const uint64_t* nb_begin,
                         const cs_lp_agent* nb, double* out) {
          try {
          const auto view = [](const cs_lp_agent& r) {
            Agent a{};
            a.agent_id = r.agent_id;
            a.position = {r.x, r.y};
            a.velocity = {r.vx, r.vy};
            a.next_waypoint = r.next_waypoint;
            a.eyesight_range = r.eyesight_range;
            return a;
          };
          const LocalPlanner* self = static_cast<const LocalPlanner*>(u);
          for (size_t k = 0; k < n; ++k) {
            std::vector<Agent> nearby;
            for (uint64_t q = nb_begin[k]; q < nb_begin[k + 1]; ++q) nearby.push_back(view(nb[q]));
            const Vec2f v = self->get_desired_velocity(view(agents[k]), nearby, Vec2f{rec[2 * k], rec[2 * k + 1]});
            out[2 * k] = v.x;
            out[2 * k + 1] = v.y;
          }
          } catch (...) {  // (nothing may unwind through the C frame: the step fails instead)
            return 1;
          }
          return 0;
  }
  virtual uint32_t register_with(cs_engine* e) { return cs_register_lp_callback(e, &LocalPlanner::batch_thunk, this); }
  // (a tile mesh evaluates planners on every tile: each tile asks for the agents it owns)
  virtual uint32_t register_with(cs_mesh* m) { return cs_mesh_register_lp_callback(m, &LocalPlanner::batch_thunk, this); }
};
struct NoLocalPlan : LocalPlanner {  // no_local_plan.rs:7-18
  uint32_t register_with(cs_engine* e) override { return cs_register_no_local_plan(e); }
  uint32_t register_with(cs_mesh* m) override { return cs_mesh_register_no_local_plan(m); }
};
struct Zanlungo : LocalPlanner {  // zanlungo.rs:31-48
  cs_zanlungo_params p;
  Zanlungo(double agent_scale, double obstacle_scale, double reaction_time, double force_distance,
           double agent_mass, double agent_radius)
      : p{agent_scale, obstacle_scale, reaction_time, force_distance, agent_mass, agent_radius} {}
  uint32_t register_with(cs_engine* e) override { return cs_register_zanlungo(e, &p); }
  uint32_t register_with(cs_mesh* m) override { return cs_mesh_register_zanlungo(m, &p); }
};

struct CrowdGenerator {  // source_sink.rs:30-33
  virtual ~CrowdGenerator() = default;
  virtual std::size_t get_number_to_spawn(std::chrono::duration<double> time_elapsed) const = 0;
  virtual void fill(cs_source_sink_desc* d) const {
    d->generator_kind = CS_GEN_CALLBACK;
    d->generator_user = const_cast<CrowdGenerator*>(this);
    d->generator = [](void* u, double dt) {
      return static_cast<const CrowdGenerator*>(u)->get_number_to_spawn(std::chrono::duration<double>(dt));
    };
  }
};
struct MonotonicCrowd : CrowdGenerator {  // source_sink.rs:85-101
  double rate;
  explicit MonotonicCrowd(double r) : rate(r) {}
  std::size_t get_number_to_spawn(std::chrono::duration<double> t) const override {
    double v = t.count() * rate;
    v = v < 0 ? 0 : (double)(long long)(v + 0.5);
    return (std::size_t)v;
  }
  void fill(cs_source_sink_desc* d) const override {
    d->generator_kind = CS_GEN_MONOTONIC;
    d->rate = rate;
  }
};

struct PoissonCrowd : CrowdGenerator {  // source_sink.rs:63-82: unseeded like the reference's thread_rng; host callback
  double rate;
  explicit PoissonCrowd(double r) : rate(r) {}
  std::size_t get_number_to_spawn(std::chrono::duration<double> t) const override {
    const double rt = t.count() * rate;
    if (!(rt > 0.0)) return 0;  // (the reference panics here: Poisson::new(rt).unwrap(), source_sink.rs:79; no exception may
                                //  cross the C ABI this is called through)
    thread_local std::mt19937_64 rng{std::random_device{}()};
    return (std::size_t)std::poisson_distribution<unsigned long long>(rt)(rng);
  }
};

struct SourceSink {  // source_sink.rs:36-60
  Vec2f source;
  double radius_sink;
  std::shared_ptr<CrowdGenerator> crowd_generator;
  std::shared_ptr<HighLevelPlanner> high_level_planner;
  std::shared_ptr<LocalPlanner> local_planner;
  std::vector<Vec2f> waypoints;
  bool loop_forever;
  double agent_eyesight_range;
};

// What agent_field returns: per bin (ix, iy) of the raster, at iy * nx + ix, the number of agents and (with velocity) the
// sums of their velocities; mean flow = sum / count.
struct AgentField {
  uint32_t nx = 0, ny = 0;
  std::vector<uint32_t> count;
  std::vector<double> sum_vx, sum_vy;  // empty unless velocities were asked for
};

// What close_pairs returns: `count` pairs of agents are closer than the distance; the first min(count, limit) of them,
// ascending by (a, b) with a < b, and the left-hand side dx * dx + dy * dy of each.
struct ClosePairs {
  uint64_t count = 0;
  std::vector<cs_id_pair> pairs;
  std::vector<double> d2;
};

// What agent_clusters returns: the members of the reported clusters ascending by id with the label of each (the smallest
// id of its cluster), and the clusters ascending by label (size, box and f64 sums of the members' positions).
struct AgentClusters {
  std::vector<uint64_t> ids, labels;
  std::vector<cs_cluster> clusters;
};
struct ClusterCounts {
  uint64_t clusters = 0, agents = 0;
};

class Simulation {  // Simulation<LocationHash2D>, lib.rs:69-383
 public:
  std::unordered_map<AgentId, Agent> agents;  // lib.rs:71, refreshed after every mutating call

  // Simulation<T: SpatialIndex>::new (lib.rs:103) for any index that describes itself as a grid
  explicit Simulation(const SpatialIndex& any_index, int device = 0) : Simulation(as_grid(any_index), device) {}
  static const LocationHash2D& as_grid(const SpatialIndex& index) {
    const LocationHash2D* grid = index.device_form();
    if (!grid)
      throw std::runtime_error("Simulation<T: SpatialIndex>: on this backend the spatial index is the neighbour kernel itself; "
                               "this index does not describe itself as a uniform grid (device_form() -> LocationHash2D)");
    return *grid;
  }
  explicit Simulation(const LocationHash2D& index, int device = 0) {  // lib.rs:103
    cs_grid_desc g{index.width, index.height, index.cell_size, index.offset.x, index.offset.y};
    cs_device_cfg cfg{};
    cfg.device_ordinal = device;
    engine_ = cs_create(&g, &cfg);
    if (!engine_) throw std::runtime_error(std::string("cs_create failed: ") + cs_last_error(nullptr));
  }
  ~Simulation() { cs_destroy(engine_); }
  Simulation(const Simulation&) = delete;
  Simulation& operator=(const Simulation&) = delete;

  std::vector<AgentId> add_agents(const std::vector<Point>& spawn_positions,  // lib.rs:119-156
                                  std::shared_ptr<HighLevelPlanner> hlp, std::shared_ptr<LocalPlanner> lp,
                                  double agent_eyesight_range) {
    std::vector<double> xy;
    for (const Point& p : spawn_positions) {
      xy.push_back(p.x);
      xy.push_back(p.y);
    }
    std::vector<uint64_t> ids(spawn_positions.size());
    int rc = cs_add_agents(engine_, xy.data(), ids.size(), handle(hlp), handle(lp), agent_eyesight_range,
                           ids.data());
    after_mutation();
    if (rc != 0) throw std::runtime_error(cs_last_error(engine_));
    return std::vector<AgentId>(ids.begin(), ids.end());
  }
  std::size_t add_source_sink(std::shared_ptr<SourceSink> s) {  // lib.rs:159-161
    cs_source_sink_desc d{};
    d.source_x = s->source.x;
    d.source_y = s->source.y;
    d.radius_sink = s->radius_sink;
    s->crowd_generator->fill(&d);
    d.hlp = handle(s->high_level_planner);
    d.lp = handle(s->local_planner);
    std::vector<double> wps;
    for (const Vec2f& w : s->waypoints) {
      wps.push_back(w.x);
      wps.push_back(w.y);
    }
    d.waypoints_xy = wps.data();
    d.n_waypoints = s->waypoints.size();
    d.loop_forever = s->loop_forever ? 1 : 0;
    d.agent_eyesight_range = s->agent_eyesight_range;
    sinks_.push_back(s);
    const uint32_t sink = cs_add_source_sink(engine_, &d);
    if (sink == UINT32_MAX) throw std::runtime_error(cs_last_error(engine_));
    return sink;
  }
  // lib.rs:164: the registry entry goes, the agents it spawned walk on; with_agents: they are removed first (events and
  // planner callbacks included), the reference's own TODO (lib.rs:165-166)
  void remove_source_sink(std::size_t id, bool with_agents = false) {
    if (with_agents) {
      cs_selection sel{};
      sel.terms = CS_SEL_SOURCE_SINK;
      sel.source_sink = (uint32_t)id;
      remove_selected(sel);
    }
    cs_remove_source_sink(engine_, (uint32_t)id);
  }
  std::size_t add_event_listener(std::shared_ptr<EventListener> l) {                        // lib.rs:171
    listeners_[next_listener_] = std::move(l);
    return next_listener_++;
  }
  void remove_agents(AgentId agent) {  // lib.rs:176-192 (unknown id throws instead of panicking)
    int rc = cs_remove_agent(engine_, agent);
    after_mutation();
    if (rc != 0) throw std::runtime_error(cs_last_error(engine_));
  }
  // agents.get_mut(&id) (lib.rs:71) for a batch, by id: the written fields (CS_WRITE_* bits) become the agents'
  // start-of-step state.  All or nothing: a refused batch throws and changes nothing.  Edit a copy of `agents` and
  // write it back: std::vector<Agent> edited = ...; sim.write_agents(edited, CS_WRITE_POSITION);
  void write_agents(const std::vector<cs_agent_view>& records, uint32_t fields = kWriteAll) {
    const int rc = cs_write_agents(engine_, records.data(), records.size(), fields);
    after_mutation();
    if (rc != 0) throw std::runtime_error(cs_last_error(engine_));
  }
  void write_agents(const std::vector<Agent>& edited, uint32_t fields = kWriteAll) {
    std::vector<cs_agent_view> v;
    for (const Agent& a : edited) v.push_back(agent_view_of(a));
    write_agents(v, fields);
  }
  // agents.get(&id) (lib.rs:71) for a batch: the agents with these ids, in the order asked, without reading the rest of
  // the crowd.  found == nullptr: an id that is not a live agent throws ("unknown agent id").  Otherwise (*found)[k]
  // says whether ids[k] is alive, and a missing agent's entry is zero except for its id.  A read changes nothing.
  std::vector<Agent> read_agents(const std::vector<AgentId>& ids, std::vector<uint8_t>* found = nullptr) {
    std::vector<cs_agent_view> v(ids.size());
    if (found) found->assign(ids.size(), 0);
    const int rc = cs_read_agents_by_id(engine_, ids.data(), ids.size(), v.data(), found ? found->data() : nullptr);
    if (rc != 0) throw std::runtime_error(cs_last_error(engine_));
    std::vector<Agent> out;
    for (const cs_agent_view& r : v) out.push_back(agent_of_view(r));
    return out;
  }
  // remove_agents (lib.rs:176-192) for a batch, in one pass over the crowd: the state, the events and the planner
  // callbacks of remove_agents(ids[0]) ... remove_agents(ids[n-1]).  All or nothing: an unknown id or an id given twice
  // throws and removes nothing.
  void remove_agents(const std::vector<AgentId>& ids) {
    const int rc = cs_remove_agents(engine_, ids.data(), ids.size());
    after_mutation();
    if (rc != 0) throw std::runtime_error(cs_last_error(engine_));
  }
  // planner.set_target(&agents[&id], goal, tolerance) (rmf/mod.rs:217-236) for a batch, in the order of the batch, on the
  // planner of each agent: a RouteFollower plans the first entry of every new (start, goal) hash pair and books it for the
  // rest, a host planner's set_target is called.  Returns one CS_TARGET_* status per entry.  All or nothing: an unknown id
  // or a non-finite goal throws, with no planner called.
  std::vector<uint8_t> set_targets(const std::vector<AgentId>& ids, const std::vector<Point>& goals, Vec2f tolerance = {}) {
    if (goals.size() != ids.size()) throw std::runtime_error("set_targets: one goal per id");
    std::vector<double> xy;
    for (const Point& g : goals) {
      xy.push_back(g.x);
      xy.push_back(g.y);
    }
    std::vector<uint8_t> status(ids.size(), 0);
    const int rc = cs_set_targets(engine_, ids.data(), xy.data(), ids.size(), tolerance.x, tolerance.y, status.data());
    if (rc != 0) throw std::runtime_error(cs_last_error(engine_));
    return status;
  }
  // sim.agents.values().filter(..) (lib.rs:71) on the device: the ids of the agents a cs_selection selects (an AND of
  // CS_SEL_* terms judged on the record `agents` holds, in f64; include/crowdstep_state.h), ascending, ready for
  // read_agents(ids) / remove_agents(ids) / set_targets.  `limit`: at most that many ids (the first ones).  Changes nothing.
  std::vector<AgentId> select_agents(const cs_selection& sel, std::size_t limit = SIZE_MAX) {
    std::vector<AgentId> ids(std::min(limit, cs_agent_count(engine_)));
    const std::size_t n = cs_select_agents(engine_, &sel, ids.data(), ids.size());
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    ids.resize(std::min(n, ids.size()));
    return ids;
  }
  // how many agents each of up to CS_SELECT_MAX selections selects, in one pass over the crowd
  std::vector<uint64_t> count_agents(const std::vector<cs_selection>& selections) {
    std::vector<uint64_t> counts(selections.size(), 0);
    if (cs_count_agents(engine_, selections.data(), selections.size(), counts.data()) != 0)
      throw std::runtime_error(cs_last_error(engine_));
    return counts;
  }
  // Where the crowd is and which way it flows, as a grid, in one pass over the agents on the device: the raster `desc`
  // (independent of the simulation's grid; include/crowdstep_state.h), only the agents `filter` selects when one is given.
  AgentField agent_field(const cs_field_desc& desc, bool velocity = false, const cs_selection* filter = nullptr) {
    AgentField f;
    const uint64_t bins = (uint64_t)desc.nx * desc.ny;
    if (bins >= 1 && bins <= CS_FIELD_MAX_CELLS) {  // (any other raster is refused below, before an output is touched)
      f.nx = desc.nx;
      f.ny = desc.ny;
      f.count.assign((std::size_t)bins, 0u);
      if (velocity) f.sum_vx.assign((std::size_t)bins, 0.0), f.sum_vy.assign((std::size_t)bins, 0.0);
    } else {
      f.count.assign(1, 0u);
      if (velocity) f.sum_vx.assign(1, 0.0), f.sum_vy.assign(1, 0.0);
    }
    if (cs_agent_field(engine_, &desc, filter, f.count.data(), velocity ? f.sum_vx.data() : nullptr,
        velocity ? f.sum_vy.data() : nullptr) != 0)
      throw std::runtime_error(cs_last_error(engine_));
    return f;
  }
  // Solve a flow field on the device (FlowProblem; include/crowdstep_state.h, "Solving a flow field on the device").
  // `planner`: a FieldPlanner of the problem's raster registered here, whose device samples take the vectors behind the
  // steps already queued.  The call waits for the device.
  FlowField solve_flow_field(const FlowProblem& p, FieldPlanner* planner = nullptr, bool vectors = true, bool distance = false) {
    uint32_t hlp = UINT32_MAX;
    if (planner && (hlp = planner->handle_in(engine_)) == UINT32_MAX)
      throw std::runtime_error("solve_flow_field: the planner is not registered with this simulation");
    FlowField f = flow_solve_call(engine_, cs_flow_field_solve, cs_last_error, p, hlp, vectors, distance);
    if (planner && vectors) planner->vxy = f.vxy;
    return f;
  }
  // The pairs of agents closer than `distance` on the device (include/crowdstep_state.h, "Pairs of agents between
  // steps"): judged in f64 on the positions `agents` holds, every pair once as (a, b) with a < b, ascending.  `a` / `b`:
  // the two roles of a pair (null: everyone), e.g. a = the robots' local planner, b = null.  `limit`: at most that many
  // pairs (the first ones); a listing of more than CS_PAIRS_MAX pairs throws, count_close_pairs has no limit.
  ClosePairs close_pairs(double distance, const cs_selection* a = nullptr, const cs_selection* b = nullptr,
                         std::size_t limit = SIZE_MAX) {
    ClosePairs out;
    out.count = count_close_pairs(distance, a, b);
    const std::size_t cap = (std::size_t)std::min<uint64_t>(out.count, limit);
    if (!cap) return out;
    out.pairs.resize(cap);
    out.d2.resize(cap);
    const std::size_t n = cs_close_pairs(engine_, distance, a, b, out.pairs.data(), out.d2.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    out.count = n;
    out.pairs.resize(std::min(n, cap));
    out.d2.resize(std::min(n, cap));
    return out;
  }
  uint64_t count_close_pairs(double distance, const cs_selection* a = nullptr, const cs_selection* b = nullptr) {
    const std::size_t n = cs_close_pairs(engine_, distance, a, b, nullptr, nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    return n;
  }
  // Which agents hang together (cs_agent_clusters, include/crowdstep_state.h "Clusters of agents between steps"): the
  // connected components of the members (`members`, null: everyone) under the links of close_pairs(distance, members,
  // members), labelled by their smallest id; only clusters of at least min_size members are reported.
  AgentClusters agent_clusters(double distance, const cs_selection* members = nullptr, uint64_t min_size = 1) {
    AgentClusters out;
    const ClusterCounts c = count_clusters(distance, members, min_size);
    out.ids.resize((std::size_t)c.agents);
    out.labels.resize((std::size_t)c.agents);
    out.clusters.resize((std::size_t)c.clusters);
    std::size_t na = 0, nc = 0;
    if (cs_agent_clusters(engine_, distance, members, min_size, out.ids.empty() ? nullptr : out.ids.data(),
                         out.ids.empty() ? nullptr : out.labels.data(), out.ids.size(), &na,
                         out.clusters.empty() ? nullptr : out.clusters.data(), out.clusters.size(), &nc))
      throw std::runtime_error(cs_last_error(engine_));
    out.ids.resize(std::min(na, out.ids.size()));
    out.labels.resize(out.ids.size());
    out.clusters.resize(std::min(nc, out.clusters.size()));
    return out;
  }
  ClusterCounts count_clusters(double distance, const cs_selection* members = nullptr, uint64_t min_size = 1) {
    std::size_t na = 0, nc = 0;
    if (cs_agent_clusters(engine_, distance, members, min_size, nullptr, nullptr, 0, &na, nullptr, 0, &nc))
      throw std::runtime_error(cs_last_error(engine_));
    ClusterCounts c;
    c.clusters = nc;
    c.agents = na;
    return c;
  }
  // What surrounds each agent (cs_agent_neighbours, include/crowdstep_state.h "Neighbours of each agent between steps"):
  // for every subject (`subjects`, null: everyone) the number of others (`others`, null: everyone; itself never) closer
  // than `distance` and the nearest of them (ties: the smallest id), ascending by id; only subjects with
  // count >= min_count are reported (0: all).  `limit`: at most that many rows (the first ones).
  std::vector<cs_neighbour_stat> agent_neighbours(double distance, const cs_selection* subjects = nullptr,
                                                  const cs_selection* others = nullptr, uint64_t min_count = 0,
                                                  std::size_t limit = SIZE_MAX) {
    std::vector<cs_neighbour_stat> out;
    const std::size_t cap = (std::size_t)std::min<uint64_t>(
        count_agents_with_neighbours(distance, subjects, others, min_count), limit);
    if (!cap) return out;
    out.resize(cap);
    const std::size_t n = cs_agent_neighbours(engine_, distance, subjects, others, min_count, out.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    out.resize(std::min(n, cap));
    return out;
  }
  uint64_t count_agents_with_neighbours(double distance, const cs_selection* subjects = nullptr,
                                        const cs_selection* others = nullptr, uint64_t min_count = 1) {
    const std::size_t n = cs_agent_neighbours(engine_, distance, subjects, others, min_count, nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    return n;
  }
  // Who comes close to whom in the near future (cs_encounters, include/crowdstep_state.h "Encounters between steps"): the
  // pairs now closer than `range` whose closest approach within `horizon`, both keeping their velocity, is closer than
  // `distance`: rows (a, b, t, d2) with a < b, ascending, t and d2 bit for bit.  `a`, `b`: the two roles (null:
  // everyone).  `limit`: at most that many rows (the first ones); a listing of more than CS_PAIRS_MAX rows throws,
  // count_encounters has no limit.
  std::vector<cs_encounter> encounters(double distance, double horizon, double range, const cs_selection* a = nullptr,
                                       const cs_selection* b = nullptr, std::size_t limit = SIZE_MAX) {
    std::vector<cs_encounter> out;
    const uint64_t count = count_encounters(distance, horizon, range, a, b);
    std::size_t cap = (std::size_t)std::min<uint64_t>(count, limit);
    if (!cap) return out;
    if (count > CS_PAIRS_MAX) cap = 1;  // (refused by the library, with its message: no room is made for it here)
    out.resize(cap);
    const std::size_t n = cs_encounters(engine_, distance, horizon, range, a, b, out.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    out.resize(std::min(n, cap));
    return out;
  }
  uint64_t count_encounters(double distance, double horizon, double range, const cs_selection* a = nullptr,
                            const cs_selection* b = nullptr) {
    const std::size_t n = cs_encounters(engine_, distance, horizon, range, a, b, nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    return n;
  }
  // What each ray hits first (cs_cast_rays, include/crowdstep_state.h "Rays against the crowd between steps"): every agent
  // is a disc of `radius`, row k of the answer is the first agent ray k enters and the parameter t where it does (the point
  // o + u * t, the direction as given), bit for bit; {CS_NO_HIT, +inf} for a ray that hits nobody.  `targets`: who can
  // be hit (null: everyone).  Line of sight from A to B: o = A, u = B - A, t_max = 1, ignore = A; visible iff the hit is B.
  std::vector<cs_ray_hit> cast_rays(const cs_ray* rays, std::size_t n, double radius, const cs_selection* targets = nullptr) {
    std::vector<cs_ray_hit> out(n);
    const std::size_t hits = cs_cast_rays(engine_, rays, n, radius, targets, out.data());
    if (hits == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    return out;
  }
  std::vector<cs_ray_hit> cast_rays(const std::vector<cs_ray>& rays, double radius, const cs_selection* targets = nullptr) {
    return cast_rays(rays.data(), rays.size(), radius, targets);
  }
  // the number of rays of cast_rays(...) that hit somebody; no rows are written
  std::size_t count_ray_hits(const std::vector<cs_ray>& rays, double radius, const cs_selection* targets = nullptr) {
    const std::size_t hits = cs_cast_rays(engine_, rays.data(), rays.size(), radius, targets, nullptr);
    if (hits == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    return hits;
  }
  // Who comes within `distance` of each timed leg first if the crowd keeps walking as it does now (cs_leg_conflicts,
  // include/crowdstep_state.h "Paths against the moving crowd between steps"): a leg is a probe at (x0, y0) at t0 moving
  // with (vx, vy) until t1, seconds from now ((0, 0): a wait); row k of the answer is the first agent slower than
  // speed_max to come within the distance of leg k and the seconds s after t0 at which it does, bit for bit;
  // {CS_NO_HIT, +inf} for a free leg.  `targets`: who can conflict (null: everyone).
  std::vector<cs_leg_hit> leg_conflicts(const cs_leg* legs, std::size_t n, double distance, double speed_max,
                                        const cs_selection* targets = nullptr) {
    std::vector<cs_leg_hit> out(n);
    const std::size_t hits = cs_leg_conflicts(engine_, legs, n, distance, speed_max, targets, out.data());
    if (hits == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    return out;
  }
  std::vector<cs_leg_hit> leg_conflicts(const std::vector<cs_leg>& legs, double distance, double speed_max,
                                        const cs_selection* targets = nullptr) {
    return leg_conflicts(legs.data(), legs.size(), distance, speed_max, targets);
  }
  // the number of legs of leg_conflicts(...) with a conflict; no rows are written
  std::size_t count_leg_conflicts(const std::vector<cs_leg>& legs, double distance, double speed_max,
                                  const cs_selection* targets = nullptr) {
    const std::size_t hits = cs_leg_conflicts(engine_, legs.data(), legs.size(), distance, speed_max, targets, nullptr);
    if (hits == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    return hits;
  }
  // Everybody who comes within `distance` of each timed leg, and when (cs_leg_intervals, include/crowdstep_state.h "Every
  // agent that enters a leg"): one row per (leg, agent) that conflicts by the rule of leg_conflicts, ascending by
  // (leg, id): the agent is within the distance from t0 + s_in to t0 + s_out, s_out at most t1 - t0, bit for bit.
  // `limit`: at most that many rows (the first ones); a listing of more than CS_PAIRS_MAX rows throws,
  // count_leg_intervals has no limit.
  std::vector<cs_leg_interval> leg_intervals(const std::vector<cs_leg>& legs, double distance, double speed_max,
                                             const cs_selection* targets = nullptr, std::size_t limit = SIZE_MAX) {
    std::vector<cs_leg_interval> out;
    const std::size_t count = cs_leg_intervals(engine_, legs.data(), legs.size(), distance, speed_max, targets, nullptr, nullptr, 0);
    if (count == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    std::size_t cap = std::min(count, limit);
    if (!cap) return out;
    if (count > CS_PAIRS_MAX) cap = 1;  // (refused by the library, with its message: no room is made for it here)
    out.resize(cap);
    const std::size_t n = cs_leg_intervals(engine_, legs.data(), legs.size(), distance, speed_max, targets, nullptr, out.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    out.resize(std::min(n, cap));
    return out;
  }
  // the number of rows of leg_intervals(...) per leg, from one pass that lists nothing, exact whatever its size
  std::vector<uint64_t> count_leg_intervals(const std::vector<cs_leg>& legs, double distance, double speed_max,
                                            const cs_selection* targets = nullptr) {
    std::vector<uint64_t> counts(legs.size());
    const std::size_t n = cs_leg_intervals(engine_, legs.data(), legs.size(), distance, speed_max, targets, counts.data(), nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    return counts;
  }
  // The agents inside each polygon zone (cs_zone_agents, include/crowdstep_state.h "Agents in polygon zones"): zones are
  // runs of `vertices_xy` (x0, y0, x1, y1, ...), one row (zone, id) per zone and agent inside it by the even-odd f64 rule of
  // the header, ascending by (zone, id); `filter`: a selection the agents must match too.  `limit`: at most that many
  // rows (the first ones); a listing of more than CS_PAIRS_MAX rows throws, count_zone_agents has no limit.
  std::vector<cs_zone_agent> zone_agents(const std::vector<cs_zone>& zones, const std::vector<double>& vertices_xy,
                                         const cs_selection* filter = nullptr, std::size_t limit = SIZE_MAX) {
    std::vector<cs_zone_agent> out;
    const std::size_t count = cs_zone_agents(engine_, zones.data(), zones.size(), vertices_xy.data(), vertices_xy.size() / 2, filter, nullptr, nullptr, 0);
    if (count == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    std::size_t cap = std::min(count, limit);
    if (!cap) return out;
    if (count > CS_PAIRS_MAX) cap = 1;  // (refused by the library, with its message: no room is made for it here)
    out.resize(cap);
    const std::size_t n = cs_zone_agents(engine_, zones.data(), zones.size(), vertices_xy.data(), vertices_xy.size() / 2, filter, nullptr, out.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    out.resize(std::min(n, cap));
    return out;
  }
  // the number of rows of zone_agents(...) per zone, from one pass that lists nothing, exact whatever its size
  std::vector<uint64_t> count_zone_agents(const std::vector<cs_zone>& zones, const std::vector<double>& vertices_xy,
                                          const cs_selection* filter = nullptr) {
    std::vector<uint64_t> counts(zones.size());
    const std::size_t n = cs_zone_agents(engine_, zones.data(), zones.size(), vertices_xy.data(), vertices_xy.size() / 2, filter, counts.data(), nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    return counts;
  }
  // Who walks through each gate within its window (cs_gate_crossings, include/crowdstep_state.h "Who crosses a line"): a
  // gate is the segment A -> B watched from t0 to t1; one row (gate, dir, id, s, u) per gate and agent that crosses it if
  // it keeps its velocity, ascending by (gate, id): at t0 + s, at A + u * (B - A), ending on the left (dir +1) or the
  // right (dir -1) of A -> B, bit for bit.  Agents at or above speed_max are not considered; `filter`: a selection the
  // agents must match too.  `limit`: at most that many rows (the first ones); a listing of more than CS_PAIRS_MAX rows
  // throws, count_gate_crossings has no limit.
  std::vector<cs_gate_crossing> gate_crossings(const std::vector<cs_gate>& gates, double speed_max,
                                               const cs_selection* filter = nullptr, std::size_t limit = SIZE_MAX) {
    std::vector<cs_gate_crossing> out;
    const std::size_t count = cs_gate_crossings(engine_, gates.data(), gates.size(), speed_max, filter, nullptr, nullptr, 0);
    if (count == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    std::size_t cap = std::min(count, limit);
    if (!cap) return out;
    if (count > CS_PAIRS_MAX) cap = 1;  // (refused by the library, with its message: no room is made for it here)
    out.resize(cap);
    const std::size_t n = cs_gate_crossings(engine_, gates.data(), gates.size(), speed_max, filter, nullptr, out.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    out.resize(std::min(n, cap));
    return out;
  }
  // the rows of gate_crossings(...) per gate and direction: [2k] dir +1, [2k + 1] dir -1; one pass that lists nothing
  std::vector<uint64_t> count_gate_crossings(const std::vector<cs_gate>& gates, double speed_max,
                                             const cs_selection* filter = nullptr) {
    std::vector<uint64_t> counts(2 * gates.size());
    const std::size_t n = cs_gate_crossings(engine_, gates.data(), gates.size(), speed_max, filter, counts.data(), nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    return counts;
  }
  // remove_agents(select_agents(sel)): the same events and planner callbacks, in ascending id; returns the removed ids
  std::vector<AgentId> remove_selected(const cs_selection& sel) {
    std::vector<AgentId> ids(cs_agent_count(engine_));
    const std::size_t n = cs_remove_selected(engine_, &sel, ids.data(), ids.size());
    after_mutation();
    if (n == SIZE_MAX) throw std::runtime_error(cs_last_error(engine_));
    ids.resize(std::min(n, ids.size()));
    return ids;
  }
  // the handle a planner was registered under, for cs_selection::hlp / lp (a planner never used here selects nobody)
  template <class P>
  uint32_t planner_handle(const std::shared_ptr<P>& p) const {
    auto it = handles_.find(p.get());
    return it != handles_.end() ? it->second : 0xFFFFFFFEu;
  }
  void step(std::chrono::duration<double> dur) {  // lib.rs:195-383
    cs_step_report rep;
    int rc = cs_step(engine_, dur.count(), &rep);
    after_mutation();
    if (rc != 0) throw std::runtime_error(cs_last_error(engine_));
  }
  // The same step without refreshing `agents` and without waiting for the device (an embedder
  // that renders from snapshots; listeners still get their events at the next step() / refresh).
  void step_no_readback(std::chrono::duration<double> dur) {
    if (cs_step(engine_, dur.count(), nullptr) != 0) throw std::runtime_error(cs_last_error(engine_));
  }
  // Streaming `agents` view (rmf_crowdsim_viz/src/main.rs:112-128): request a frame behind the
  // queued steps, pick it up later; the records stay valid until the second request from now.
  void request_snapshot() {
    if (cs_snapshot_request(engine_) != 0) throw std::runtime_error(cs_last_error(engine_));
  }
  struct Frame {
    const cs_snapshot_record* agents = nullptr;
    std::size_t count = 0;
    uint64_t step_index = 0;
    bool ready = false;
  };
  Frame snapshot(bool wait = true) {
    Frame f;
    int rc = cs_snapshot_acquire(engine_, wait ? 1 : 0, &f.agents, &f.count, &f.step_index);
    if (rc == 3) throw std::runtime_error(cs_last_error(engine_));
    f.ready = rc == 0;
    return f;
  }
  cs_engine* handle() { return engine_; }  // (for the calls of the C ABI this mirror does not wrap: cs_kernel_stat, ...)

 private:
  template <class P>
  uint32_t handle(const std::shared_ptr<P>& p) {
    auto it = handles_.find(p.get());
    if (it != handles_.end()) return it->second;
    uint32_t h = register_planner(p.get());
    handles_[p.get()] = h;
    keep_.push_back(p);
    return h;
  }
  uint32_t register_planner(HighLevelPlanner* p) { return p->register_with(engine_); }
  uint32_t register_planner(LocalPlanner* p) { return p->register_with(engine_); }

  void after_mutation() {
    cs_event ev[256];
    for (;;) {
      std::size_t n = cs_drain_events(engine_, ev, 256);
      for (std::size_t i = 0; i < n; ++i)
        for (auto& kv : listeners_) {
          if (ev[i].kind == CS_EVENT_SPAWNED) kv.second->agent_spawned({ev[i].x, ev[i].y}, ev[i].id);
          if (ev[i].kind == CS_EVENT_DESTROYED) kv.second->agent_destroyed(ev[i].id);
        }
      if (n < 256) break;
    }
    std::vector<cs_agent_view> v(cs_agent_count(engine_));
    std::size_t got = cs_read_agents(engine_, v.data(), v.size());
    agents.clear();
    for (std::size_t i = 0; i < got; ++i) {
      Agent a;
      a.agent_id = v[i].id;
      a.position = {v[i].x, v[i].y};
      a.velocity = {v[i].vx, v[i].vy};
      a.next_waypoint = v[i].next_waypoint;
      a.eyesight_range = v[i].eyesight_range;
      agents[a.agent_id] = a;
    }
  }

  cs_engine* engine_ = nullptr;
  std::map<const void*, uint32_t> handles_;
  std::vector<std::shared_ptr<void>> keep_;
  std::vector<std::shared_ptr<SourceSink>> sinks_;
  std::map<std::size_t, std::shared_ptr<EventListener>> listeners_;
  std::size_t next_listener_ = 0;
};

// The same `Simulation`, cut into tiles_x x tiles_y spatial tiles: one tile engine per tile behind
// the C ABI's mesh handle (cs_mesh_*: layout, halo exchange, spawn flags, route misses, re-cuts, merged queries all
// in the library).  With `rccl_unique_id` (CS_RCCL_UNIQUE_ID_BYTES from cs_rccl_unique_id on one rank) the
// distributed form: one tile per rank and GPU; a `host_transport` (three functions over MPI, sockets, ...:
// cs_mesh_host_transport) can stand in for RCCL or beside it.  In the distributed forms every call is collective and
// `agents`, re-cuts and the queries cover the whole crowd on every rank.  Results equal Simulation's bit for bit while nobody touches the
// domain's edges.
class TiledSimulation {
 public:
  std::unordered_map<AgentId, Agent> agents;  // lib.rs:71, refreshed after every mutating call

  TiledSimulation(const LocationHash2D& index, uint32_t tiles_x, uint32_t tiles_y, uint32_t halo_cells, int device = 0,
                  const uint8_t* rccl_unique_id = nullptr, int rank = 0, int n_ranks = 1, double density_per_cell = 16.0,
                  const cs_mesh_host_transport* host_transport = nullptr) {
    cs_grid_desc g{index.width, index.height, index.cell_size, index.offset.x, index.offset.y};
    cs_mesh_desc d{};
    d.tiles_x = tiles_x;
    d.tiles_y = tiles_y;
    d.halo_cells = halo_cells;
    d.device_ordinal = device;
    d.rank = rank;
    d.n_ranks = n_ranks;
    d.density_per_cell = density_per_cell;
    d.rccl_unique_id = rccl_unique_id;
    d.host_transport = host_transport;
    mesh_ = cs_mesh_create(&g, &d);
    if (!mesh_) throw std::runtime_error(std::string("cs_mesh_create failed: ") + cs_mesh_last_error(nullptr));
  }
  ~TiledSimulation() { cs_mesh_destroy(mesh_); }
  TiledSimulation(const TiledSimulation&) = delete;
  TiledSimulation& operator=(const TiledSimulation&) = delete;

  std::vector<AgentId> add_agents(const std::vector<Point>& spawn_positions, std::shared_ptr<HighLevelPlanner> hlp,
                                  std::shared_ptr<LocalPlanner> lp, double agent_eyesight_range) {  // lib.rs:119-156
    std::vector<double> xy;
    for (const Point& p : spawn_positions) {
      xy.push_back(p.x);
      xy.push_back(p.y);
    }
    std::vector<uint64_t> ids(spawn_positions.size());
    const int rc = cs_mesh_add_agents(mesh_, xy.data(), ids.size(), handle(hlp), handle(lp), agent_eyesight_range, ids.data());
    refresh();
    if (rc != 0) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return std::vector<AgentId>(ids.begin(), ids.end());
  }
  std::size_t add_source_sink(std::shared_ptr<SourceSink> s) {  // lib.rs:159-161
    cs_source_sink_desc d{};
    d.source_x = s->source.x;
    d.source_y = s->source.y;
    d.radius_sink = s->radius_sink;
    s->crowd_generator->fill(&d);
    d.hlp = handle(s->high_level_planner);
    d.lp = handle(s->local_planner);
    std::vector<double> wps;
    for (const Vec2f& w : s->waypoints) {
      wps.push_back(w.x);
      wps.push_back(w.y);
    }
    d.waypoints_xy = wps.data();
    d.n_waypoints = s->waypoints.size();
    d.loop_forever = s->loop_forever ? 1 : 0;
    d.agent_eyesight_range = s->agent_eyesight_range;
    keep_.push_back(s);
    const uint32_t sink = cs_mesh_add_source_sink(mesh_, &d);
    if (sink == UINT32_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return sink;
  }
  void remove_source_sink(std::size_t id, bool with_agents = false) {  // lib.rs:164 (Simulation::remove_source_sink)
    if (with_agents) {
      cs_selection sel{};
      sel.terms = CS_SEL_SOURCE_SINK;
      sel.source_sink = (uint32_t)id;
      remove_selected(sel);
    }
    cs_mesh_remove_source_sink(mesh_, (uint32_t)id);
  }
  std::size_t add_event_listener(std::shared_ptr<EventListener> l) {                           // lib.rs:171
    listeners_[next_listener_] = std::move(l);
    cs_mesh_event_recording(mesh_, 1);
    return next_listener_++;
  }
  void remove_agents(AgentId agent) {  // lib.rs:176-192
    const int rc = cs_mesh_remove_agent(mesh_, agent);
    refresh();
    if (rc != 0) throw std::runtime_error(cs_mesh_last_error(mesh_));
  }
  // Simulation::write_agents on the mesh: an agent written into a cell another tile owns moves there (collective in the
  // distributed forms: every rank passes the same batch)
  void write_agents(const std::vector<cs_agent_view>& records, uint32_t fields = kWriteAll) {
    const int rc = cs_mesh_write_agents(mesh_, records.data(), records.size(), fields);
    refresh();
    if (rc != 0) throw std::runtime_error(cs_mesh_last_error(mesh_));
  }
  void write_agents(const std::vector<Agent>& edited, uint32_t fields = kWriteAll) {
    std::vector<cs_agent_view> v;
    for (const Agent& a : edited) v.push_back(agent_view_of(a));
    write_agents(v, fields);
  }
  // Simulation::read_agents(ids) and remove_agents(ids) on the mesh (collective in the distributed forms: every rank
  // passes the same ids; the read returns the whole answer on every rank)
  std::vector<Agent> read_agents(const std::vector<AgentId>& ids, std::vector<uint8_t>* found = nullptr) {
    std::vector<cs_agent_view> v(ids.size());
    if (found) found->assign(ids.size(), 0);
    const int rc = cs_mesh_read_agents_by_id(mesh_, ids.data(), ids.size(), v.data(), found ? found->data() : nullptr);
    if (rc != 0) throw std::runtime_error(cs_mesh_last_error(mesh_));
    std::vector<Agent> out;
    for (const cs_agent_view& r : v) out.push_back(agent_of_view(r));
    return out;
  }
  void remove_agents(const std::vector<AgentId>& ids) {
    const int rc = cs_mesh_remove_agents(mesh_, ids.data(), ids.size());
    refresh();
    if (rc != 0) throw std::runtime_error(cs_mesh_last_error(mesh_));
  }
  // Simulation::set_targets on the mesh (collective in the distributed forms: every rank passes the same batch and gets
  // the same statuses; every tile books the routes of the whole batch, so that all tiles number routes alike)
  std::vector<uint8_t> set_targets(const std::vector<AgentId>& ids, const std::vector<Point>& goals, Vec2f tolerance = {}) {
    if (goals.size() != ids.size()) throw std::runtime_error("set_targets: one goal per id");
    std::vector<double> xy;
    for (const Point& g : goals) {
      xy.push_back(g.x);
      xy.push_back(g.y);
    }
    std::vector<uint8_t> status(ids.size(), 0);
    const int rc = cs_mesh_set_targets(mesh_, ids.data(), xy.data(), ids.size(), tolerance.x, tolerance.y, status.data());
    if (rc != 0) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return status;
  }
  // sim.agents.values().filter(..) (lib.rs:71) on the device: the ids of the agents a cs_selection selects (an AND of
  // CS_SEL_* terms judged on the record `agents` holds, in f64; include/crowdstep_state.h), ascending, ready for
  // read_agents(ids) / remove_agents(ids) / set_targets.  `limit`: at most that many ids (the first ones).  Changes nothing.
  std::vector<AgentId> select_agents(const cs_selection& sel, std::size_t limit = SIZE_MAX) {
    std::vector<AgentId> ids(std::min(limit, cs_mesh_agent_count(mesh_)));
    const std::size_t n = cs_mesh_select_agents(mesh_, &sel, ids.data(), ids.size());
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    ids.resize(std::min(n, ids.size()));
    return ids;
  }
  // how many agents each of up to CS_SELECT_MAX selections selects, in one pass over the crowd
  std::vector<uint64_t> count_agents(const std::vector<cs_selection>& selections) {
    std::vector<uint64_t> counts(selections.size(), 0);
    if (cs_mesh_count_agents(mesh_, selections.data(), selections.size(), counts.data()) != 0)
      throw std::runtime_error(cs_mesh_last_error(mesh_));
    return counts;
  }
  // Where the crowd is and which way it flows, as a grid, in one pass over the agents on the device: the raster `desc`
  // (independent of the simulation's grid; include/crowdstep_state.h), only the agents `filter` selects when one is given.
  AgentField agent_field(const cs_field_desc& desc, bool velocity = false, const cs_selection* filter = nullptr) {
    AgentField f;
    const uint64_t bins = (uint64_t)desc.nx * desc.ny;
    if (bins >= 1 && bins <= CS_FIELD_MAX_CELLS) {  // (any other raster is refused below, before an output is touched)
      f.nx = desc.nx;
      f.ny = desc.ny;
      f.count.assign((std::size_t)bins, 0u);
      if (velocity) f.sum_vx.assign((std::size_t)bins, 0.0), f.sum_vy.assign((std::size_t)bins, 0.0);
    } else {
      f.count.assign(1, 0u);
      if (velocity) f.sum_vx.assign(1, 0.0), f.sum_vy.assign(1, 0.0);
    }
    if (cs_mesh_agent_field(mesh_, &desc, filter, f.count.data(), velocity ? f.sum_vx.data() : nullptr,
        velocity ? f.sum_vy.data() : nullptr) != 0)
      throw std::runtime_error(cs_mesh_last_error(mesh_));
    return f;
  }
  // Solve a flow field on the device (FlowProblem; include/crowdstep_state.h, "Solving a flow field on the device").
  // `planner`: a FieldPlanner of the problem's raster registered here, whose device samples take the vectors behind the
  // steps already queued.  The call waits for the device.
  FlowField solve_flow_field(const FlowProblem& p, FieldPlanner* planner = nullptr, bool vectors = true, bool distance = false) {
    uint32_t hlp = UINT32_MAX;
    if (planner && (hlp = planner->handle_in(mesh_)) == UINT32_MAX)
      throw std::runtime_error("solve_flow_field: the planner is not registered with this simulation");
    FlowField f = flow_solve_call(mesh_, cs_mesh_flow_field_solve, cs_mesh_last_error, p, hlp, vectors, distance);
    if (planner && vectors) planner->vxy = f.vxy;
    return f;
  }
  // The pairs of agents closer than `distance` on the device (include/crowdstep_state.h, "Pairs of agents between
  // steps"): judged in f64 on the positions `agents` holds, every pair once as (a, b) with a < b, ascending.  `a` / `b`:
  // the two roles of a pair (null: everyone), e.g. a = the robots' local planner, b = null.  `limit`: at most that many
  // pairs (the first ones); a listing of more than CS_PAIRS_MAX pairs throws, count_close_pairs has no limit.
  ClosePairs close_pairs(double distance, const cs_selection* a = nullptr, const cs_selection* b = nullptr,
                         std::size_t limit = SIZE_MAX) {
    ClosePairs out;
    out.count = count_close_pairs(distance, a, b);
    const std::size_t cap = (std::size_t)std::min<uint64_t>(out.count, limit);
    if (!cap) return out;
    out.pairs.resize(cap);
    out.d2.resize(cap);
    const std::size_t n = cs_mesh_close_pairs(mesh_, distance, a, b, out.pairs.data(), out.d2.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    out.count = n;
    out.pairs.resize(std::min(n, cap));
    out.d2.resize(std::min(n, cap));
    return out;
  }
  uint64_t count_close_pairs(double distance, const cs_selection* a = nullptr, const cs_selection* b = nullptr) {
    const std::size_t n = cs_mesh_close_pairs(mesh_, distance, a, b, nullptr, nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return n;
  }
  // Which agents hang together (cs_agent_clusters, include/crowdstep_state.h "Clusters of agents between steps"): the
  // connected components of the members (`members`, null: everyone) under the links of close_pairs(distance, members,
  // members), labelled by their smallest id; only clusters of at least min_size members are reported.
  AgentClusters agent_clusters(double distance, const cs_selection* members = nullptr, uint64_t min_size = 1) {
    AgentClusters out;
    const ClusterCounts c = count_clusters(distance, members, min_size);
    out.ids.resize((std::size_t)c.agents);
    out.labels.resize((std::size_t)c.agents);
    out.clusters.resize((std::size_t)c.clusters);
    std::size_t na = 0, nc = 0;
    if (cs_mesh_agent_clusters(mesh_, distance, members, min_size, out.ids.empty() ? nullptr : out.ids.data(),
                              out.ids.empty() ? nullptr : out.labels.data(), out.ids.size(), &na,
                              out.clusters.empty() ? nullptr : out.clusters.data(), out.clusters.size(), &nc))
      throw std::runtime_error(cs_mesh_last_error(mesh_));
    out.ids.resize(std::min(na, out.ids.size()));
    out.labels.resize(out.ids.size());
    out.clusters.resize(std::min(nc, out.clusters.size()));
    return out;
  }
  ClusterCounts count_clusters(double distance, const cs_selection* members = nullptr, uint64_t min_size = 1) {
    std::size_t na = 0, nc = 0;
    if (cs_mesh_agent_clusters(mesh_, distance, members, min_size, nullptr, nullptr, 0, &na, nullptr, 0, &nc))
      throw std::runtime_error(cs_mesh_last_error(mesh_));
    ClusterCounts c;
    c.clusters = nc;
    c.agents = na;
    return c;
  }
  // What surrounds each agent (cs_mesh_agent_neighbours, include/crowdstep_state.h "Neighbours of each agent between steps"):
  // for every subject (`subjects`, null: everyone) the number of others (`others`, null: everyone; itself never) closer
  // than `distance` and the nearest of them (ties: the smallest id), ascending by id; only subjects with
  // count >= min_count are reported (0: all).  `limit`: at most that many rows (the first ones).
  std::vector<cs_neighbour_stat> agent_neighbours(double distance, const cs_selection* subjects = nullptr,
                                                  const cs_selection* others = nullptr, uint64_t min_count = 0,
                                                  std::size_t limit = SIZE_MAX) {
    std::vector<cs_neighbour_stat> out;
    const std::size_t cap = (std::size_t)std::min<uint64_t>(
        count_agents_with_neighbours(distance, subjects, others, min_count), limit);
    if (!cap) return out;
    out.resize(cap);
    const std::size_t n = cs_mesh_agent_neighbours(mesh_, distance, subjects, others, min_count, out.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    out.resize(std::min(n, cap));
    return out;
  }
  uint64_t count_agents_with_neighbours(double distance, const cs_selection* subjects = nullptr,
                                        const cs_selection* others = nullptr, uint64_t min_count = 1) {
    const std::size_t n = cs_mesh_agent_neighbours(mesh_, distance, subjects, others, min_count, nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return n;
  }
  // Who comes close to whom in the near future (cs_mesh_encounters, include/crowdstep_state.h "Encounters between steps"): the
  // pairs now closer than `range` whose closest approach within `horizon`, both keeping their velocity, is closer than
  // `distance`: rows (a, b, t, d2) with a < b, ascending, t and d2 bit for bit.  `a`, `b`: the two roles (null:
  // everyone).  `limit`: at most that many rows (the first ones); a listing of more than CS_PAIRS_MAX rows throws,
  // count_encounters has no limit.
  std::vector<cs_encounter> encounters(double distance, double horizon, double range, const cs_selection* a = nullptr,
                                       const cs_selection* b = nullptr, std::size_t limit = SIZE_MAX) {
    std::vector<cs_encounter> out;
    const uint64_t count = count_encounters(distance, horizon, range, a, b);
    std::size_t cap = (std::size_t)std::min<uint64_t>(count, limit);
    if (!cap) return out;
    if (count > CS_PAIRS_MAX) cap = 1;  // (refused by the library, with its message: no room is made for it here)
    out.resize(cap);
    const std::size_t n = cs_mesh_encounters(mesh_, distance, horizon, range, a, b, out.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    out.resize(std::min(n, cap));
    return out;
  }
  uint64_t count_encounters(double distance, double horizon, double range, const cs_selection* a = nullptr,
                            const cs_selection* b = nullptr) {
    const std::size_t n = cs_mesh_encounters(mesh_, distance, horizon, range, a, b, nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return n;
  }
  // What each ray hits first (cs_mesh_cast_rays, include/crowdstep_state.h "Rays against the crowd between steps"): every agent
  // is a disc of `radius`, row k of the answer is the first agent ray k enters and the parameter t where it does (the point
  // o + u * t, the direction as given), bit for bit; {CS_NO_HIT, +inf} for a ray that hits nobody.  `targets`: who can
  // be hit (null: everyone).  Line of sight from A to B: o = A, u = B - A, t_max = 1, ignore = A; visible iff the hit is B.
  std::vector<cs_ray_hit> cast_rays(const cs_ray* rays, std::size_t n, double radius, const cs_selection* targets = nullptr) {
    std::vector<cs_ray_hit> out(n);
    const std::size_t hits = cs_mesh_cast_rays(mesh_, rays, n, radius, targets, out.data());
    if (hits == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return out;
  }
  std::vector<cs_ray_hit> cast_rays(const std::vector<cs_ray>& rays, double radius, const cs_selection* targets = nullptr) {
    return cast_rays(rays.data(), rays.size(), radius, targets);
  }
  // the number of rays of cast_rays(...) that hit somebody; no rows are written
  std::size_t count_ray_hits(const std::vector<cs_ray>& rays, double radius, const cs_selection* targets = nullptr) {
    const std::size_t hits = cs_mesh_cast_rays(mesh_, rays.data(), rays.size(), radius, targets, nullptr);
    if (hits == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return hits;
  }
  // Who comes within `distance` of each timed leg first if the crowd keeps walking as it does now (cs_mesh_leg_conflicts,
  // include/crowdstep_state.h "Paths against the moving crowd between steps"): a leg is a probe at (x0, y0) at t0 moving
  // with (vx, vy) until t1, seconds from now ((0, 0): a wait); row k of the answer is the first agent slower than
  // speed_max to come within the distance of leg k and the seconds s after t0 at which it does, bit for bit;
  // {CS_NO_HIT, +inf} for a free leg.  `targets`: who can conflict (null: everyone).
  std::vector<cs_leg_hit> leg_conflicts(const cs_leg* legs, std::size_t n, double distance, double speed_max,
                                        const cs_selection* targets = nullptr) {
    std::vector<cs_leg_hit> out(n);
    const std::size_t hits = cs_mesh_leg_conflicts(mesh_, legs, n, distance, speed_max, targets, out.data());
    if (hits == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return out;
  }
  std::vector<cs_leg_hit> leg_conflicts(const std::vector<cs_leg>& legs, double distance, double speed_max,
                                        const cs_selection* targets = nullptr) {
    return leg_conflicts(legs.data(), legs.size(), distance, speed_max, targets);
  }
  // the number of legs of leg_conflicts(...) with a conflict; no rows are written
  std::size_t count_leg_conflicts(const std::vector<cs_leg>& legs, double distance, double speed_max,
                                  const cs_selection* targets = nullptr) {
    const std::size_t hits = cs_mesh_leg_conflicts(mesh_, legs.data(), legs.size(), distance, speed_max, targets, nullptr);
    if (hits == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return hits;
  }
  // Everybody who comes within `distance` of each timed leg, and when (cs_mesh_leg_intervals, include/crowdstep_state.h "Every
  // agent that enters a leg"): one row per (leg, agent) that conflicts by the rule of leg_conflicts, ascending by
  // (leg, id): the agent is within the distance from t0 + s_in to t0 + s_out, s_out at most t1 - t0, bit for bit.
  // `limit`: at most that many rows (the first ones); a listing of more than CS_PAIRS_MAX rows throws,
  // count_leg_intervals has no limit.
  std::vector<cs_leg_interval> leg_intervals(const std::vector<cs_leg>& legs, double distance, double speed_max,
                                             const cs_selection* targets = nullptr, std::size_t limit = SIZE_MAX) {
    std::vector<cs_leg_interval> out;
    const std::size_t count = cs_mesh_leg_intervals(mesh_, legs.data(), legs.size(), distance, speed_max, targets, nullptr, nullptr, 0);
    if (count == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    std::size_t cap = std::min(count, limit);
    if (!cap) return out;
    if (count > CS_PAIRS_MAX) cap = 1;  // (refused by the library, with its message: no room is made for it here)
    out.resize(cap);
    const std::size_t n = cs_mesh_leg_intervals(mesh_, legs.data(), legs.size(), distance, speed_max, targets, nullptr, out.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    out.resize(std::min(n, cap));
    return out;
  }
  // the number of rows of leg_intervals(...) per leg, from one pass that lists nothing, exact whatever its size
  std::vector<uint64_t> count_leg_intervals(const std::vector<cs_leg>& legs, double distance, double speed_max,
                                            const cs_selection* targets = nullptr) {
    std::vector<uint64_t> counts(legs.size());
    const std::size_t n = cs_mesh_leg_intervals(mesh_, legs.data(), legs.size(), distance, speed_max, targets, counts.data(), nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return counts;
  }
  // The agents inside each polygon zone (cs_mesh_zone_agents, include/crowdstep_state.h "Agents in polygon zones"): zones are
  // runs of `vertices_xy` (x0, y0, x1, y1, ...), one row (zone, id) per zone and agent inside it by the even-odd f64 rule of
  // the header, ascending by (zone, id); `filter`: a selection the agents must match too.  `limit`: at most that many
  // rows (the first ones); a listing of more than CS_PAIRS_MAX rows throws, count_zone_agents has no limit.
  std::vector<cs_zone_agent> zone_agents(const std::vector<cs_zone>& zones, const std::vector<double>& vertices_xy,
                                         const cs_selection* filter = nullptr, std::size_t limit = SIZE_MAX) {
    std::vector<cs_zone_agent> out;
    const std::size_t count = cs_mesh_zone_agents(mesh_, zones.data(), zones.size(), vertices_xy.data(), vertices_xy.size() / 2, filter, nullptr, nullptr, 0);
    if (count == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    std::size_t cap = std::min(count, limit);
    if (!cap) return out;
    if (count > CS_PAIRS_MAX) cap = 1;  // (refused by the library, with its message: no room is made for it here)
    out.resize(cap);
    const std::size_t n = cs_mesh_zone_agents(mesh_, zones.data(), zones.size(), vertices_xy.data(), vertices_xy.size() / 2, filter, nullptr, out.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    out.resize(std::min(n, cap));
    return out;
  }
  // the number of rows of zone_agents(...) per zone, from one pass that lists nothing, exact whatever its size
  std::vector<uint64_t> count_zone_agents(const std::vector<cs_zone>& zones, const std::vector<double>& vertices_xy,
                                          const cs_selection* filter = nullptr) {
    std::vector<uint64_t> counts(zones.size());
    const std::size_t n = cs_mesh_zone_agents(mesh_, zones.data(), zones.size(), vertices_xy.data(), vertices_xy.size() / 2, filter, counts.data(), nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return counts;
  }
  // Who walks through each gate within its window (cs_mesh_gate_crossings, include/crowdstep_state.h "Who crosses a
  // line"): one row (gate, dir, id, s, u) per gate and agent that crosses it, ascending by (gate, id), bit for bit the
  // single engine's.  `limit`: at most that many rows (the first ones); a listing of more than CS_PAIRS_MAX rows throws,
  // count_gate_crossings has no limit.
  std::vector<cs_gate_crossing> gate_crossings(const std::vector<cs_gate>& gates, double speed_max,
                                               const cs_selection* filter = nullptr, std::size_t limit = SIZE_MAX) {
    std::vector<cs_gate_crossing> out;
    const std::size_t count = cs_mesh_gate_crossings(mesh_, gates.data(), gates.size(), speed_max, filter, nullptr, nullptr, 0);
    if (count == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    std::size_t cap = std::min(count, limit);
    if (!cap) return out;
    if (count > CS_PAIRS_MAX) cap = 1;  // (refused by the library, with its message: no room is made for it here)
    out.resize(cap);
    const std::size_t n = cs_mesh_gate_crossings(mesh_, gates.data(), gates.size(), speed_max, filter, nullptr, out.data(), cap);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    out.resize(std::min(n, cap));
    return out;
  }
  // the rows of gate_crossings(...) per gate and direction: [2k] dir +1, [2k + 1] dir -1; one pass that lists nothing
  std::vector<uint64_t> count_gate_crossings(const std::vector<cs_gate>& gates, double speed_max,
                                             const cs_selection* filter = nullptr) {
    std::vector<uint64_t> counts(2 * gates.size());
    const std::size_t n = cs_mesh_gate_crossings(mesh_, gates.data(), gates.size(), speed_max, filter, counts.data(), nullptr, 0);
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    return counts;
  }
  // remove_agents(select_agents(sel)): the same events and planner callbacks, in ascending id; returns the removed ids
  std::vector<AgentId> remove_selected(const cs_selection& sel) {
    std::vector<AgentId> ids(cs_mesh_agent_count(mesh_));
    const std::size_t n = cs_mesh_remove_selected(mesh_, &sel, ids.data(), ids.size());
    refresh();
    if (n == SIZE_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    ids.resize(std::min(n, ids.size()));
    return ids;
  }
  // the handle a planner was registered under, for cs_selection::hlp / lp (a planner never used here selects nobody)
  template <class P>
  uint32_t planner_handle(const std::shared_ptr<P>& p) const {
    auto it = handles_.find(p.get());
    return it != handles_.end() ? it->second : 0xFFFFFFFEu;
  }
  void step(std::chrono::duration<double> dur) {  // lib.rs:195-383
    cs_step_report rep;
    const int rc = cs_mesh_step(mesh_, dur.count(), &rep);
    refresh();
    if (rc != 0) throw std::runtime_error(cs_mesh_last_error(mesh_));
  }
  void step_no_readback(std::chrono::duration<double> dur) {  // nothing waits for the device
    if (cs_mesh_step(mesh_, dur.count(), nullptr) != 0) throw std::runtime_error(cs_mesh_last_error(mesh_));
  }
  void recut() {  // cuts to the quantiles of where the crowd stands now (in-process form)
    if (cs_mesh_recut(mesh_) != 0) throw std::runtime_error(cs_mesh_last_error(mesh_));
  }
  cs_mesh* handle() { return mesh_; }

 private:
  template <class P>
  uint32_t handle(const std::shared_ptr<P>& p) {
    auto it = handles_.find(p.get());
    if (it != handles_.end()) return it->second;
    const uint32_t h = register_planner(p.get());
    if (h == UINT32_MAX) throw std::runtime_error(cs_mesh_last_error(mesh_));
    handles_[p.get()] = h;
    keep_.push_back(p);
    return h;
  }
  uint32_t register_planner(HighLevelPlanner* p) { return p->register_with(mesh_); }
  uint32_t register_planner(LocalPlanner* p) { return p->register_with(mesh_); }
  void refresh() {
    cs_event ev[256];
    for (;;) {
      const std::size_t n = cs_mesh_drain_events(mesh_, ev, 256);
      for (std::size_t i = 0; i < n; ++i)
        for (auto& kv : listeners_) {
          if (ev[i].kind == CS_EVENT_SPAWNED) kv.second->agent_spawned({ev[i].x, ev[i].y}, ev[i].id);
          if (ev[i].kind == CS_EVENT_DESTROYED) kv.second->agent_destroyed(ev[i].id);
        }
      if (n < 256) break;
    }
    std::vector<cs_agent_view> v(cs_mesh_agent_count(mesh_));
    const std::size_t got = cs_mesh_read_agents(mesh_, v.data(), v.size());
    agents.clear();
    for (std::size_t i = 0; i < got && got != SIZE_MAX; ++i) {
      Agent a;
      a.agent_id = v[i].id;
      a.position = {v[i].x, v[i].y};
      a.velocity = {v[i].vx, v[i].vy};
      a.next_waypoint = v[i].next_waypoint;
      a.eyesight_range = v[i].eyesight_range;
      agents[a.agent_id] = a;
    }
  }

  cs_mesh* mesh_ = nullptr;
  std::map<const void*, uint32_t> handles_;
  std::vector<std::shared_ptr<void>> keep_;
  std::map<std::size_t, std::shared_ptr<EventListener>> listeners_;
  std::size_t next_listener_ = 0;
};

}  // namespace rmf_crowdsim
#endif
