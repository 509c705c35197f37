// The pairs of agents within a distance from C++ (include/crowdsim.hpp over include/crowdstep_state.h): close_pairs and
// count_close_pairs on one engine and on a 2 x 2 mesh against a brute-force double loop over `agents` by the rule the
// header writes: the same pairs in the same order, the same d2 bits, with and without roles, under a limit, and a
// refused call throws.  Runs on an MI355X (tests/test_gpu_close_pairs_cpp.py builds and launches it).
#include <algorithm>
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

struct Found {
  uint64_t a, b;
  double d2;
};

// the rule of the header on every two entries of `agents` (volatile: every operation rounded once); rect: role A
template <class Map>
static std::vector<Found> brute(const Map& agents, double size, double distance, const cs_selection* rect_a) {
  std::vector<const Agent*> part;
  for (const auto& kv : agents) {
    const Point p = kv.second.position;
    if (0.0 <= p.x && p.x < size && 0.0 <= p.y && p.y < size) part.push_back(&kv.second);
  }
  std::sort(part.begin(), part.end(), [](const Agent* l, const Agent* r) { return l->agent_id < r->agent_id; });
  auto in_a = [&](const Agent* g) {
    return !rect_a || (rect_a->x0 <= g->position.x && g->position.x < rect_a->x1 && rect_a->y0 <= g->position.y &&
                       g->position.y < rect_a->y1);
  };
  std::vector<Found> out;
  volatile double dist2 = distance * distance;
  for (std::size_t i = 0; i < part.size(); ++i)
    for (std::size_t j = i + 1; j < part.size(); ++j) {
      volatile double dx = part[i]->position.x - part[j]->position.x, dy = part[i]->position.y - part[j]->position.y;
      volatile double xx = dx * dx, yy = dy * dy;
      volatile double d2 = xx + yy;
      if (!(d2 < dist2)) continue;
      if (!(in_a(part[i]) || in_a(part[j]))) continue;  // (role B is everyone)
      out.push_back(Found{part[i]->agent_id, part[j]->agent_id, d2});
    }
  return out;
}

static void agree(const ClosePairs& got, const std::vector<Found>& want, std::size_t limit) {
  CHECK(got.count == want.size());
  const std::size_t n = std::min(want.size(), limit);
  CHECK(got.pairs.size() == n && got.d2.size() == n);
  for (std::size_t k = 0; k < n; ++k) {
    CHECK(got.pairs[k].a == want[k].a && got.pairs[k].b == want[k].b);
    CHECK(std::memcmp(&got.d2[k], &want[k].d2, sizeof(double)) == 0);
  }
}

int main() {
  const double size = 60.0;
  const LocationHash2D grid(size, size, 2.0, Point{0.0, 0.0});
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
  std::size_t total = 0;
  for (double distance : {0.0, 0.6, 1.25, 2.0}) {  // (2.0: the most a mesh with one halo cell of 2 m allows)
    for (const cs_selection* a : {(const cs_selection*)nullptr, (const cs_selection*)&box}) {
      const std::vector<Found> want = brute(one.agents, size, distance, a);
      total += want.size();
      agree(one.close_pairs(distance, a), want, SIZE_MAX);
      agree(mesh.close_pairs(distance, a), want, SIZE_MAX);
      agree(one.close_pairs(distance, a, nullptr, 7), want, 7);
      agree(mesh.close_pairs(distance, a, nullptr, 7), want, 7);
      CHECK(one.count_close_pairs(distance, a) == want.size() && mesh.count_close_pairs(distance, a) == want.size());
      agree(one.close_pairs(distance, nullptr, a), want, SIZE_MAX);  // (the roles are symmetric)
    }
  }
  CHECK(total > 500);
  CHECK(one.count_close_pairs(INFINITY) == 400u * 399u / 2u);
  CHECK(one.count_close_pairs(1.25) > 0 && one.count_close_pairs(1.25) < 400u * 399u / 2u);

  // a refused call throws and the next one is right, on the engine and on the mesh
  int threw = 0;
  try {
    one.close_pairs(-1.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "close_pairs") != nullptr;
  }
  try {
    mesh.close_pairs(2.5);  // above halo_cells * cell_size
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "close_pairs") != nullptr;
  }
  CHECK(threw == 2);
  agree(one.close_pairs(1.25), brute(one.agents, size, 1.25, nullptr), SIZE_MAX);
  agree(mesh.close_pairs(1.25), brute(mesh.agents, size, 1.25, nullptr), SIZE_MAX);
  steps(one, 5);
  steps(mesh, 5);
  agree(mesh.close_pairs(1.25), brute(one.agents, size, 1.25, nullptr), SIZE_MAX);
  std::printf("close pairs: passed\n");
  return 0;
}
