// The neighbours of each agent from C++ (include/crowdsim.hpp over include/crowdstep_state.h): agent_neighbours and
// count_agents_with_neighbours on one engine and on a 2 x 2 mesh against a brute-force double loop over `agents` by the
// rules the header writes: the same rows, byte for byte, with and without selections, a min_count and a limit, and a
// refused call throws.  Runs on an MI355X (tests/test_gpu_neighbours_cpp.py builds and launches it).
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

static bool in_rect(const cs_selection* r, const Point& p) {
  return !r || (r->x0 <= p.x && p.x < r->x1 && r->y0 <= p.y && p.y < r->y1);
}

// the rules of the header on `agents` (volatile: every operation rounded once); rects: subjects / others (null: everyone)
template <class Map>
static std::vector<cs_neighbour_stat> brute(const Map& agents, double size, double distance, const cs_selection* subjects,
                                            const cs_selection* others, uint64_t min_count) {
  std::vector<const Agent*> part;
  for (const auto& kv : agents) {
    const Point p = kv.second.position;
    if (0.0 <= p.x && p.x < size && 0.0 <= p.y && p.y < size) part.push_back(&kv.second);
  }
  std::sort(part.begin(), part.end(), [](const Agent* l, const Agent* r) { return l->agent_id < r->agent_id; });
  volatile double dist2 = distance * distance;
  std::vector<cs_neighbour_stat> out;
  for (std::size_t i = 0; i < part.size(); ++i) {
    if (!in_rect(subjects, part[i]->position)) continue;
    cs_neighbour_stat row{};
    row.id = part[i]->agent_id;
    row.nearest = CS_NO_NEIGHBOUR;
    row.nearest_d2 = INFINITY;
    for (std::size_t j = 0; j < part.size(); ++j) {  // (ascending id: the first of equal d2 is the smallest id)
      if (j == i || !in_rect(others, part[j]->position)) continue;
      volatile double dx = part[i]->position.x - part[j]->position.x, dy = part[i]->position.y - part[j]->position.y;
      volatile double xx = dx * dx, yy = dy * dy;
      volatile double d2 = xx + yy;
      if (!(d2 < dist2)) continue;
      ++row.count;
      if (d2 < row.nearest_d2) {
        row.nearest_d2 = d2;
        row.nearest = part[j]->agent_id;
      }
    }
    if (row.count >= min_count) out.push_back(row);
  }
  return out;
}

static void agree(const std::vector<cs_neighbour_stat>& got, uint64_t count, const std::vector<cs_neighbour_stat>& want) {
  CHECK(count == want.size());
  CHECK(got.size() == want.size());
  CHECK(got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(cs_neighbour_stat)) == 0);
}

int main() {
  static_assert(sizeof(cs_neighbour_stat) == 32, "four 8-byte words");
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

  cs_selection box{}, strip{};
  box.terms = CS_SEL_RECT;
  box.x0 = 24.0; box.y0 = 22.5; box.x1 = 37.25; box.y1 = 36.0;  // across both cuts of the mesh (30 m)
  strip.terms = CS_SEL_RECT;
  strip.x0 = 0.0; strip.y0 = 28.0; strip.x1 = 60.0; strip.y1 = 33.0;  // along one cut
  std::size_t rows = 0, with = 0;
  uint64_t most = 0;
  for (double distance : {0.0, 1.0, 1.25, 2.0}) {  // (2.0: the most a mesh with one halo cell of 2 m allows)
    for (const cs_selection* sub : {(const cs_selection*)nullptr, (const cs_selection*)&box}) {
      for (const cs_selection* oth : {(const cs_selection*)nullptr, (const cs_selection*)&strip}) {
        for (uint64_t min_count : {(uint64_t)0, (uint64_t)1, (uint64_t)3}) {
          const std::vector<cs_neighbour_stat> want = brute(one.agents, size, distance, sub, oth, min_count);
          rows += want.size();
          for (const cs_neighbour_stat& r : want) {
            with += r.count > 0;
            most = std::max(most, r.count);
          }
          agree(one.agent_neighbours(distance, sub, oth, min_count),
                one.count_agents_with_neighbours(distance, sub, oth, min_count), want);
          agree(mesh.agent_neighbours(distance, sub, oth, min_count),
                mesh.count_agents_with_neighbours(distance, sub, oth, min_count), want);
        }
      }
    }
  }
  std::printf("neighbours: %zu rows compared, %zu with a neighbour, the largest count %llu\n", rows, with,
              (unsigned long long)most);
  CHECK(rows > 2000 && with > 500 && most >= 4);
  // a limit: the first rows
  const std::vector<cs_neighbour_stat> all = brute(one.agents, size, 1.25, nullptr, nullptr, 0);
  CHECK(all.size() == 400);
  const std::vector<cs_neighbour_stat> few = one.agent_neighbours(1.25, nullptr, nullptr, 0, 7);
  CHECK(few.size() == 7 && std::memcmp(few.data(), all.data(), 7 * sizeof(cs_neighbour_stat)) == 0);
  const std::vector<cs_neighbour_stat> few_m = mesh.agent_neighbours(1.25, nullptr, nullptr, 0, 7);
  CHECK(few_m.size() == 7 && std::memcmp(few_m.data(), all.data(), 7 * sizeof(cs_neighbour_stat)) == 0);
  // +inf on one engine: everyone but itself
  const std::vector<cs_neighbour_stat> far = one.agent_neighbours(INFINITY);
  CHECK(far.size() == 400);
  for (const cs_neighbour_stat& r : far) CHECK(r.count == 399);
  agree(far, one.count_agents_with_neighbours(INFINITY, nullptr, nullptr, 399), brute(one.agents, size, INFINITY, nullptr, nullptr, 0));

  // a refused call throws and the next one is right, on the engine and on the mesh
  int threw = 0;
  try {
    one.agent_neighbours(-1.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "agent_neighbours") != nullptr;
  }
  try {
    mesh.agent_neighbours(2.5);  // above halo_cells * cell_size
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "halo_cells") != nullptr;
  }
  CHECK(threw == 2);
  steps(one, 5);
  steps(mesh, 5);
  const std::vector<cs_neighbour_stat> later = brute(one.agents, size, 1.25, nullptr, nullptr, 2);
  agree(one.agent_neighbours(1.25, nullptr, nullptr, 2), one.count_agents_with_neighbours(1.25, nullptr, nullptr, 2), later);
  agree(mesh.agent_neighbours(1.25, nullptr, nullptr, 2), mesh.count_agents_with_neighbours(1.25, nullptr, nullptr, 2), later);
  std::printf("neighbours: passed\n");
  return 0;
}
