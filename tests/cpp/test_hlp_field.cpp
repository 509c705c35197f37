// The flow-field planner from C++ (include/crowdsim.hpp over include/crowdstep_state.h): crowdsim::FieldPlanner on a
// Simulation steps to the same bytes as a host planner that evaluates the same rule through the callback path, for both
// samplings, across an update(); a TiledSimulation (2 x 2) with the planner steps as the single engine does; a refused
// raster throws and leaves the simulation usable.
// Runs on an MI355X (tests/test_gpu_hlp_field_cpp.py builds and launches it).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "crowdsim.hpp"

using namespace rmf_crowdsim;

#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

// the same field through the host callback path: the comparison
struct HostField : HighLevelPlanner {
  std::shared_ptr<FieldPlanner> field;
  std::size_t calls = 0;
  explicit HostField(std::shared_ptr<FieldPlanner> f) : field(std::move(f)) {}
  bool get_desired_velocity(const Agent& a, std::chrono::duration<double> t, Vec2f* out) override {
    ++calls;
    return field->get_desired_velocity(a, t, out);
  }
};

// 11 x 9 bins of 3.1 x 2.7 from (14.3, 16.9): part of the crowd stands outside; a swirl, a wall of NaN bins in column 6
static std::vector<float> swirl(const cs_field_desc& d, double turn) {
  std::vector<float> v(2 * (std::size_t)d.nx * d.ny);
  for (uint32_t iy = 0; iy < d.ny; ++iy)
    for (uint32_t ix = 0; ix < d.nx; ++ix) {
      const double cx = ix + 0.5 - 0.5 * d.nx, cy = iy + 0.5 - 0.5 * d.ny;
      const std::size_t k = 2 * ((std::size_t)iy * d.nx + ix);
      v[k] = (float)(turn * -cy * 0.11 + 0.2);
      v[k + 1] = (float)(turn * cx * 0.09 - 0.1);
      if (ix == 6 && iy >= 2 && iy <= 6) v[k] = std::numeric_limits<float>::quiet_NaN();
    }
  return v;
}

template <class A, class B>
static std::size_t same_agents(const A& a, const B& b) {
  CHECK(a.size() == b.size());
  std::size_t moving = 0;
  for (const auto& kv : a) {
    const auto it = b.find(kv.first);
    CHECK(it != b.end());
    const Agent &p = kv.second, &q = it->second;
    CHECK(std::memcmp(&p.position, &q.position, sizeof p.position) == 0);
    CHECK(std::memcmp(&p.velocity, &q.velocity, sizeof p.velocity) == 0);
    if (p.velocity.x != 0.0 || p.velocity.y != 0.0) ++moving;
  }
  return moving;
}

int main() {
  const LocationHash2D grid(60.0, 60.0, 2.0, Point{0.0, 0.0});
  const cs_field_desc raster{14.3, 16.9, 3.1, 2.7, 11u, 9u};
  std::vector<Point> pts;
  for (int ix = 0; ix < 24; ++ix)
    for (int iy = 0; iy < 24; ++iy) pts.push_back(Point{12.0 + 1.5 * ix + 0.013 * iy, 13.0 + 1.4 * iy + 0.017 * ix});
  const auto step = std::chrono::duration<double>(0.1);

  for (uint32_t sampling : {CS_HLP_FIELD_NEAREST, CS_HLP_FIELD_BILINEAR}) {
    auto field = std::make_shared<FieldPlanner>(raster, swirl(raster, 1.0), sampling);
    auto host = std::make_shared<HostField>(field);
    auto zan = std::make_shared<Zanlungo>(1.0, 1.0, 0.0, 0.4, 2.0, 0.2);
    Simulation on_device(grid), on_host(grid);
    TiledSimulation mesh(grid, 2, 2, 1);
    on_device.add_agents(pts, field, zan, 2.0);
    on_host.add_agents(pts, host, zan, 2.0);
    mesh.add_agents(pts, field, zan, 2.0);
    std::size_t moving = 0;
    for (int k = 0; k < 12; ++k) {
      if (k == 6) field->update(swirl(raster, -0.7));  // (the engine, every tile of the mesh, and the host's copy)
      on_device.step(step);
      on_host.step(step);
      mesh.step(step);
      moving = same_agents(on_device.agents, on_host.agents);
      same_agents(mesh.agents, on_device.agents);
    }
    CHECK(host->calls >= 12u * pts.size());
    CHECK(moving > 100 && moving < pts.size());  // (some stand outside the raster or on the wall: None)
    CHECK(cs_kernel_stat(on_device.handle(), CS_STAT_HLP_FIELD_LAUNCHES) == 12u);
    CHECK(cs_kernel_stat(on_host.handle(), CS_STAT_HLP_FIELD_LAUNCHES) == 0u);
    // steps that wait for nothing, then the agents
    for (int k = 0; k < 5; ++k) on_device.step_no_readback(step);
    for (int k = 0; k < 5; ++k) on_host.step(step);
    on_device.step(step);
    on_host.step(step);
    same_agents(on_device.agents, on_host.agents);
  }

  // a refused raster throws, says why, and the simulation goes on
  Simulation sim(grid);
  auto zan = std::make_shared<Zanlungo>(1.0, 1.0, 0.0, 0.4, 2.0, 0.2);
  cs_field_desc bad = raster;
  bad.cell_w = 0.0;
  int threw = 0;
  try {
    sim.add_agents(pts, std::make_shared<FieldPlanner>(bad, swirl(bad, 1.0)), zan, 2.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "hlp_field") != nullptr;
  }
  try {
    sim.add_agents(pts, std::make_shared<FieldPlanner>(raster, swirl(raster, 1.0), 7u), zan, 2.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "sampling") != nullptr;
  }
  try {
    FieldPlanner(raster, std::vector<float>(5));
  } catch (const std::runtime_error&) {
    ++threw;
  }
  CHECK(threw == 3 && sim.agents.empty());
  sim.add_agents(pts, std::make_shared<FieldPlanner>(raster, swirl(raster, 1.0)), zan, 2.0);
  sim.step(step);
  CHECK(sim.agents.size() == pts.size());
  std::printf("hlp field: passed\n");
  return 0;
}
