// Rasterising the crowd from C++ (include/crowdsim.hpp over include/crowdstep_state.h): agent_field on one engine and on a
// 2 x 2 mesh against a brute-force loop over `agents` by the rule the header writes: counts equal, sums within
// n * 2^-52 * sum|v| (equal where a bin holds one agent or none), with and without a filter, and a refused raster throws.
// Runs on an MI355X (tests/test_gpu_field_cpp.py builds and launches it).
#include <cmath>
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

template <class Sim>
static void steps(Sim& s, int n) {
  for (int k = 0; k < n; ++k) s.step(std::chrono::duration<double>(0.05));
}

struct Brute {
  std::vector<uint32_t> count;
  std::vector<long double> vx, vy, ax, ay;  // sums and sums of magnitudes (x87 extended: the reference of the bound)
};

// the rule of the header on every entry of `agents` (volatile: one subtraction, one division, each rounded once)
template <class Map>
static Brute brute(const Map& agents, const cs_field_desc& d, const cs_selection* rect) {
  Brute b;
  const std::size_t bins = (std::size_t)d.nx * d.ny;
  b.count.assign(bins, 0u);
  b.vx.assign(bins, 0.0L); b.vy.assign(bins, 0.0L); b.ax.assign(bins, 0.0L); b.ay.assign(bins, 0.0L);
  for (const auto& kv : agents) {
    const Agent& a = kv.second;
    const double x = a.position.x, y = a.position.y;
    if (rect && !(rect->x0 <= x && x < rect->x1 && rect->y0 <= y && y < rect->y1)) continue;
    volatile double dx = x - d.x0, dy = y - d.y0;
    volatile double fx = dx / d.cell_w, fy = dy / d.cell_h;
    if (!(0.0 <= fx && fx < (double)d.nx && 0.0 <= fy && fy < (double)d.ny)) continue;
    const std::size_t bin = (std::size_t)(uint32_t)fy * d.nx + (uint32_t)fx;
    b.count[bin] += 1u;
    b.vx[bin] += (long double)a.velocity.x; b.vy[bin] += (long double)a.velocity.y;
    b.ax[bin] += std::fabs((long double)a.velocity.x); b.ay[bin] += std::fabs((long double)a.velocity.y);
  }
  return b;
}

// -> the number of bins with two agents or more
static std::size_t agree(const AgentField& f, const Brute& b, bool velocity) {
  CHECK(f.count == b.count);
  std::size_t crowded = 0;
  for (std::size_t k = 0; k < b.count.size(); ++k) {
    if (b.count[k] >= 2u) ++crowded;
    if (!velocity) continue;
    const long double n = (long double)b.count[k];
    if (b.count[k] <= 1u) {
      CHECK(f.sum_vx[k] == (double)b.vx[k] && f.sum_vy[k] == (double)b.vy[k]);
      if (!b.count[k]) CHECK(!std::signbit(f.sum_vx[k]) && !std::signbit(f.sum_vy[k]));
    } else {
      CHECK(std::fabs((long double)f.sum_vx[k] - b.vx[k]) <= n * 0x1p-52L * b.ax[k]);
      CHECK(std::fabs((long double)f.sum_vy[k] - b.vy[k]) <= n * 0x1p-52L * b.ay[k]);
    }
  }
  if (!velocity) CHECK(f.sum_vx.empty() && f.sum_vy.empty());
  return crowded;
}

int main() {
  const LocationHash2D grid(60.0, 60.0, 2.0, Point{0.0, 0.0});
  auto east = std::make_shared<StubHighLevelPlan>(Vec2f{0.3, 0.2});
  auto west = std::make_shared<StubHighLevelPlan>(Vec2f{-0.6, 0.1});
  auto zan = std::make_shared<Zanlungo>(1.0, 1.0, 0.0, 0.4, 2.0, 0.2);
  std::vector<Point> pts_e, pts_w;
  for (int ix = 0; ix < 20; ++ix)
    for (int iy = 0; iy < 20; ++iy)
      ((ix + iy) % 2 ? pts_e : pts_w).push_back(Point{18.0 + 1.1 * ix + 0.01 * iy, 17.0 + 1.2 * iy + 0.02 * ix});

  Simulation one(grid);
  TiledSimulation mesh(grid, 2, 2, 1);
  one.add_agents(pts_e, east, zan, 2.0);
  mesh.add_agents(pts_e, east, zan, 2.0);
  one.add_agents(pts_w, west, zan, 2.0);
  mesh.add_agents(pts_w, west, zan, 2.0);
  steps(one, 20);
  steps(mesh, 20);

  cs_selection box{};
  box.terms = CS_SEL_RECT;
  box.x0 = 24.0; box.y0 = 22.5; box.x1 = 37.25; box.y1 = 36.0;  // across both cuts of the mesh (30 m)
  const cs_field_desc rasters[] = {
      {0.0, 0.0, 60.0, 60.0, 1u, 1u},      // one bin
      {15.0, 15.0, 4.0, 4.0, 8u, 8u},      // coarse, over the crowd and across the cuts
      {0.0, 0.0, 2.0, 2.0, 30u, 30u},      // the simulation's cells
      {20.0, 18.0, 0.25, 0.4, 96u, 64u},   // fine, non-square bins, part of the crowd outside
      {31.0, 31.0, 1.0, 1.0, 12u, 12u},    // inside one tile of the mesh
      {100.0, 100.0, 1.0, 1.0, 16u, 16u},  // nobody
  };
  std::size_t crowded = 0;
  for (const cs_field_desc& d : rasters)
    for (const cs_selection* filter : {(const cs_selection*)nullptr, (const cs_selection*)&box})
      for (bool velocity : {false, true}) {
        const Brute want = brute(one.agents, d, filter);
        crowded += agree(one.agent_field(d, velocity, filter), want, velocity);
        const AgentField on_mesh = mesh.agent_field(d, velocity, filter);
        CHECK(on_mesh.nx == d.nx && on_mesh.ny == d.ny);
        agree(on_mesh, brute(mesh.agents, d, filter), velocity);
        CHECK(on_mesh.count == want.count);  // (the mesh steps as one engine)
      }
  CHECK(crowded > 50);
  const AgentField all = one.agent_field(rasters[0], true);
  CHECK(all.count[0] == one.agents.size() && all.count[0] == 400u);
  CHECK(one.agent_field(rasters[5]).count == std::vector<uint32_t>(256u, 0u));

  // a refused raster throws and the next one is right, on the engine and on the mesh
  int threw = 0;
  cs_field_desc bad = rasters[1];
  bad.cell_w = 0.0;
  try {
    one.agent_field(bad);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "agent_field") != nullptr;
  }
  bad = rasters[1];
  bad.nx = 4096u; bad.ny = 4096u;
  try {
    mesh.agent_field(bad, true);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "agent_field") != nullptr;
  }
  CHECK(threw == 2);
  agree(one.agent_field(rasters[1], true), brute(one.agents, rasters[1], nullptr), true);
  agree(mesh.agent_field(rasters[1], true), brute(mesh.agents, rasters[1], nullptr), true);
  steps(one, 5);
  steps(mesh, 5);
  CHECK(mesh.agent_field(rasters[2]).count == one.agent_field(rasters[2]).count);
  std::printf("field: passed\n");
  return 0;
}
