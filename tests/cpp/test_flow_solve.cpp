// Solving a flow field from C++ (include/crowdsim.hpp over include/crowdstep_state.h): Simulation::solve_flow_field on a
// maze, and FieldPlanner::solve with the crowd's density on a Simulation and a 2 x 2 TiledSimulation, against the bytes the
// Python restatement of the rule wrote (tests/flow_solve_reference.py); a refused problem throws and leaves the
// simulation usable.
// Runs on an MI355X (tests/test_gpu_flow_solve_cpp.py writes the cases, builds and launches it: argv[1] = the case file).
//
// The case file, little endian: u32 n_cases, then per case
//   u32 nx, ny, has_blocked, n_agents; f64 x0, y0, cell_w, cell_h, speed, density_weight; u64 reached
//   u8 goals[nx * ny]; u8 blocked[nx * ny] (if has_blocked); f64 agents[n_agents][2]
//   f32 vxy[nx * ny][2]; f64 dist[nx * ny]
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

template <class T>
static std::vector<T> take(std::FILE* f, std::size_t n) {
  std::vector<T> v(n);
  CHECK(n == 0 || std::fread(v.data(), sizeof(T), n, f) == n);
  return v;
}

static void same(const FlowField& got, const std::vector<float>& vxy, const std::vector<double>& dist, uint64_t reached) {
  CHECK(got.vxy.size() == vxy.size() && got.dist.size() == dist.size());
  CHECK(std::memcmp(got.vxy.data(), vxy.data(), vxy.size() * sizeof(float)) == 0);
  CHECK(std::memcmp(got.dist.data(), dist.data(), dist.size() * sizeof(double)) == 0);
  CHECK(got.reached == reached && got.rounds >= 1u);
}

int main(int argc, char** argv) {
  CHECK(argc == 2);
  std::FILE* f = std::fopen(argv[1], "rb");
  CHECK(f != nullptr);
  const uint32_t n_cases = take<uint32_t>(f, 1)[0];
  CHECK(n_cases >= 2u);
  const LocationHash2D grid(64.0, 64.0, 2.0, Point{0.0, 0.0});
  const auto step = std::chrono::duration<double>(0.05);
  uint32_t with_agents = 0;
  for (uint32_t c = 0; c < n_cases; ++c) {
    const auto head = take<uint32_t>(f, 4);
    const auto real = take<double>(f, 6);
    const uint64_t reached = take<uint64_t>(f, 1)[0];
    FlowProblem p;
    p.raster = cs_field_desc{real[0], real[1], real[2], real[3], head[0], head[1]};
    p.speed = real[4];
    p.density_weight = real[5];
    const std::size_t bins = (std::size_t)head[0] * head[1];
    p.goals = take<uint8_t>(f, bins);
    if (head[2]) p.blocked = take<uint8_t>(f, bins);
    const auto xy = take<double>(f, 2 * (std::size_t)head[3]);
    const auto vxy = take<float>(f, 2 * bins);
    const auto dist = take<double>(f, bins);
    std::vector<Point> pts;
    for (std::size_t k = 0; k < head[3]; ++k) pts.push_back(Point{xy[2 * k], xy[2 * k + 1]});

    Simulation sim(grid);
    if (pts.empty()) {  // no crowd, no planner: the rasters come back
      same(sim.solve_flow_field(p, nullptr, true, true), vxy, dist, reached);
      const FlowField only = sim.solve_flow_field(p, nullptr, false, true);
      CHECK(only.vxy.empty() && only.reached == reached);
      continue;
    }
    ++with_agents;
    auto field = std::make_shared<FieldPlanner>(p.raster, std::vector<float>(2 * bins, 0.0f));
    auto zan = std::make_shared<Zanlungo>(1.0, 1.0, 0.0, 0.4, 2.0, 0.2);
    TiledSimulation mesh(grid, 2, 2, 1);
    sim.add_agents(pts, field, zan, 2.0);
    mesh.add_agents(pts, field, zan, 2.0);
    same(sim.solve_flow_field(p, field.get(), true, true), vxy, dist, reached);
    CHECK(std::memcmp(field->vxy.data(), vxy.data(), vxy.size() * sizeof(float)) == 0);
    same(mesh.solve_flow_field(p, field.get(), true, true), vxy, dist, reached);
    same(field->solve(p, true, true), vxy, dist, reached);  // (the engine, then every tile of the mesh: the mesh's answer)
    const FlowField quiet = field->solve(p, false, false);  // (nothing comes back but the statistics)
    CHECK(quiet.vxy.empty() && quiet.dist.empty() && quiet.reached == reached);
    // the crowd follows the solved field on both, to the same bytes
    for (int k = 0; k < 4; ++k) {
      sim.step(step);
      mesh.step(step);
    }
    CHECK(sim.agents.size() == mesh.agents.size());
    std::size_t moving = 0;
    for (const auto& kv : sim.agents) {
      const auto it = mesh.agents.find(kv.first);
      CHECK(it != mesh.agents.end());
      CHECK(std::memcmp(&kv.second.position, &it->second.position, sizeof kv.second.position) == 0);
      if (kv.second.velocity.x != 0.0 || kv.second.velocity.y != 0.0) ++moving;
    }
    CHECK(moving > pts.size() / 2);

    // refusals throw, say why, and change nothing
    FlowProblem bad = p;
    bad.speed = -1.0;
    int threw = 0;
    try {
      sim.solve_flow_field(bad, field.get());
    } catch (const std::runtime_error& e) {
      threw += std::strstr(e.what(), "speed") != nullptr;
    }
    bad = p;
    bad.raster.x0 += 1.0;  // (not the planner's raster)
    try {
      sim.solve_flow_field(bad, field.get());
    } catch (const std::runtime_error& e) {
      threw += std::strstr(e.what(), "raster") != nullptr;
    }
    bad = p;
    bad.goals.pop_back();
    try {
      sim.solve_flow_field(bad);
    } catch (const std::runtime_error&) {
      ++threw;
    }
    try {
      sim.solve_flow_field(p, nullptr, false, false);  // (nothing to write to)
    } catch (const std::runtime_error& e) {
      threw += std::strstr(e.what(), "nothing to write") != nullptr;
    }
    CHECK(threw == 4);
    sim.step(step);
    CHECK(sim.agents.size() == pts.size());
  }
  CHECK(with_agents >= 1u);
  std::fclose(f);
  std::printf("flow solve: passed\n");
  return 0;
}
