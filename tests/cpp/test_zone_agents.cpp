// Agents in polygon zones from C++ (include/crowdsim.hpp over include/crowdstep_state.h): zone_agents and
// count_zone_agents on one engine and on a 2 x 2 mesh against a brute-force loop over `agents` by the rule the header
// writes: the same rows, byte for byte, with and without a filter, with a limit, and a refused call throws.
// tests/test_gpu_zone_agents_cpp.py builds and launches this on an MI355X.
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

// the ring test of the header (volatile: every operation rounded once)
static bool in_ring(const cs_zone& z, const std::vector<double>& v, double x, double y) {
  const double* r = v.data() + 2 * z.first;
  double bx0 = r[0], bx1 = r[0], by0 = r[1], by1 = r[1];
  for (uint32_t i = 1; i < z.count; ++i) {
    bx0 = std::min(bx0, r[2 * i]);
    bx1 = std::max(bx1, r[2 * i]);
    by0 = std::min(by0, r[2 * i + 1]);
    by1 = std::max(by1, r[2 * i + 1]);
  }
  if (!(bx0 <= x && x <= bx1 && by0 <= y && y <= by1)) return false;
  unsigned crossings = 0;
  for (uint32_t i = 0; i < z.count; ++i) {
    const uint32_t j = (i + 1) % z.count;
    const bool up = r[2 * i + 1] <= r[2 * j + 1];
    const double lx = up ? r[2 * i] : r[2 * j], ly = up ? r[2 * i + 1] : r[2 * j + 1];
    const double hx = up ? r[2 * j] : r[2 * i], hy = up ? r[2 * j + 1] : r[2 * i + 1];
    if (ly == hy) continue;
    if (!(ly <= y && y < hy)) continue;
    volatile double ex = hx - lx, ey = hy - ly, px = x - lx, py = y - ly;
    volatile double t1 = ex * py, t2 = ey * px;
    volatile double c = t1 - t2;
    crossings += c > 0.0;
  }
  return crossings % 2 == 1;
}

template <class Map>
static std::vector<cs_zone_agent> brute(const Map& agents, double size, const std::vector<cs_zone>& zones,
                                        const std::vector<double>& v, const cs_selection* filter,
                                        std::vector<uint64_t>* counts) {
  std::vector<const Agent*> order;
  for (const auto& kv : agents) order.push_back(&kv.second);
  std::sort(order.begin(), order.end(), [](const Agent* l, const Agent* r) { return l->agent_id < r->agent_id; });
  std::vector<cs_zone_agent> out;
  counts->assign(zones.size(), 0);
  for (std::size_t k = 0; k < zones.size(); ++k)
    for (const Agent* q : order) {
      const Point p = q->position;
      if (!(0.0 <= p.x && p.x < size && 0.0 <= p.y && p.y < size)) continue;
      if (!in_rect(filter, p) || !in_ring(zones[k], v, p.x, p.y)) continue;
      out.push_back(cs_zone_agent{(uint64_t)k, q->agent_id});
      (*counts)[k] += 1;
    }
  return out;
}

template <class Sim>
static void agree(Sim& sim, const std::vector<cs_zone>& zones, const std::vector<double>& v, const cs_selection* filter,
                  const std::vector<cs_zone_agent>& want, const std::vector<uint64_t>& counts) {
  const std::vector<cs_zone_agent> got = sim.zone_agents(zones, v, filter);
  CHECK(got.size() == want.size());
  CHECK(got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(cs_zone_agent)) == 0);
  CHECK(sim.count_zone_agents(zones, v, filter) == counts);
  const std::size_t some = want.size() / 3;
  const std::vector<cs_zone_agent> head = sim.zone_agents(zones, v, filter, some);
  CHECK(head.size() == some && (!some || std::memcmp(head.data(), want.data(), some * sizeof(cs_zone_agent)) == 0));
}

static void ring(std::vector<cs_zone>* zones, std::vector<double>* v, std::initializer_list<double> xy) {
  zones->push_back(cs_zone{(uint64_t)v->size() / 2, (uint32_t)(xy.size() / 2), 0u});
  v->insert(v->end(), xy.begin(), xy.end());
}

int main() {
  static_assert(sizeof(cs_zone) == 16 && sizeof(cs_zone_agent) == 16, "two 8-byte words each");
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

  // rooms astride both cuts of the mesh (30 m): rectangles in both windings, an L, a slanted cabin, a bow tie, a triangle
  // fan that shares its vertices, a sliver, one zone over everything, one outside the grid
  std::vector<cs_zone> zones;
  std::vector<double> v;
  for (int k = 0; k < 12; ++k) {
    const double x0 = 16.0 + 2.3 * k, y0 = 15.5 + 1.7 * k, x1 = x0 + 6.1, y1 = y0 + 7.3;
    if (k % 2) ring(&zones, &v, {x0, y0, x1, y0, x1, y1, x0, y1});
    else ring(&zones, &v, {x0, y1, x1, y1, x1, y0, x0, y0});
  }
  ring(&zones, &v, {20.0, 20.0, 40.0, 20.0, 40.0, 28.0, 28.0, 28.0, 28.0, 40.0, 20.0, 40.0});  // an L
  ring(&zones, &v, {25.0, 18.0, 36.5, 24.25, 33.0, 31.0, 21.5, 24.75});                       // a cabin at an angle
  ring(&zones, &v, {22.0, 22.0, 38.0, 38.0, 38.0, 22.0, 22.0, 38.0});                         // a bow tie
  ring(&zones, &v, {29.9, 10.0, 30.1, 10.0, 30.05, 50.0});                                    // a sliver along a cut
  ring(&zones, &v, {-10.0, -10.0, 70.0, -10.0, 70.0, 70.0, -10.0, 70.0});                     // everything
  ring(&zones, &v, {61.0, 61.0, 70.0, 61.0, 65.0, 70.0});                                     // outside
  const uint64_t fan = v.size() / 2;  // a fan of triangles round (30, 30): zones that share vertices
  const double hub[2] = {30.0, 30.0};
  v.insert(v.end(), hub, hub + 2);
  for (int k = 0; k < 9; ++k) {
    const double a = 0.7 * k;
    v.push_back(30.0 + 11.0 * std::cos(a));
    v.push_back(30.0 + 11.0 * std::sin(a));
  }
  // triangle k = (rim k, rim k + 1, hub written again behind them): runs of three that overlap
  for (int k = 0; k < 8; ++k) {
    zones.push_back(cs_zone{(uint64_t)v.size() / 2, 3u, 0u});
    v.push_back(hub[0]);
    v.push_back(hub[1]);
    v.push_back(v[2 * (fan + 1 + k)]);
    v.push_back(v[2 * (fan + 1 + k) + 1]);
    v.push_back(v[2 * (fan + 2 + k)]);
    v.push_back(v[2 * (fan + 2 + k) + 1]);
  }
  zones.push_back(cs_zone{fan + 1, 9u, 0u});  // the rim alone, a run inside the run of vertices written above

  cs_selection box{};
  box.terms = CS_SEL_RECT;
  box.x0 = 24.0; box.y0 = 22.5; box.x1 = 37.25; box.y1 = 36.0;  // across both cuts of the mesh
  std::size_t rows = 0, busy = 0, empty = 0;
  std::vector<uint64_t> counts;
  for (const cs_selection* filter : {(const cs_selection*)nullptr, (const cs_selection*)&box}) {
    const std::vector<cs_zone_agent> want = brute(one.agents, size, zones, v, filter, &counts);
    rows += want.size();
    for (uint64_t c : counts) {
      busy += c >= 5;
      empty += c == 0;
    }
    agree(one, zones, v, filter, want, counts);
    agree(mesh, zones, v, filter, want, counts);
    if (!filter) CHECK(counts[16] == one.agents.size() && counts[17] == 0);
  }
  std::printf("zone agents: %zu rows compared, %zu zones with five agents or more, %zu empty\n", rows, busy, empty);
  CHECK(rows > 500 && busy > 20 && empty >= 2);
  // no zones at all
  CHECK(one.zone_agents(std::vector<cs_zone>{}, v).empty() && mesh.count_zone_agents(std::vector<cs_zone>{}, v).empty());

  // a refused call throws and the next one is right, on the engine and on the mesh
  int threw = 0;
  std::vector<cs_zone> bad = zones;
  bad[7].count = 2;
  try {
    one.zone_agents(bad, v);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "zone_agents: zone 7") != nullptr;
  }
  bad = zones;
  bad[3].flags = 1;
  try {
    mesh.count_zone_agents(bad, v);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "zone_agents: zone 3") != nullptr;
  }
  CHECK(threw == 2);
  steps(one, 5);
  steps(mesh, 5);
  const std::vector<cs_zone_agent> later = brute(one.agents, size, zones, v, &box, &counts);
  agree(one, zones, v, &box, later, counts);
  agree(mesh, zones, v, &box, later, counts);
  std::printf("zone agents: passed\n");
  return 0;
}
