// Who crosses a line from C++ (include/crowdsim.hpp over include/crowdstep_state.h): gate_crossings and
// count_gate_crossings on one engine and on a 2 x 2 mesh against a brute-force loop over `agents` by the rule the header
// writes: the same rows, byte for byte, with and without a filter, with a limit, and a refused call throws.
// tests/test_gpu_gate_crossings_cpp.py builds and launches this on an MI355X.
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

// the rule of the header on `agents` (volatile: every operation rounded once), the rows ascending by (gate, id); rect:
// the filter (null: everyone)
template <class Map>
static std::vector<cs_gate_crossing> brute(const Map& agents, double size, const std::vector<cs_gate>& gates, double speed_max,
                                           const cs_selection* filter, std::vector<uint64_t>* counts) {
  std::vector<const Agent*> order;
  for (const auto& kv : agents) order.push_back(&kv.second);
  std::sort(order.begin(), order.end(), [](const Agent* l, const Agent* r) { return l->agent_id < r->agent_id; });
  std::vector<cs_gate_crossing> out;
  counts->assign(2 * gates.size(), 0);
  volatile double S2 = speed_max * speed_max;
  for (std::size_t k = 0; k < gates.size(); ++k) {
    const cs_gate& g = gates[k];
    volatile double T = g.t1 - g.t0;
    volatile double ex = g.bx - g.ax, ey = g.by - g.ay;
    for (const Agent* qp : order) {
      const Agent& q = *qp;
      const Point p = q.position;
      if (!(0.0 <= p.x && p.x < size && 0.0 <= p.y && p.y < size)) continue;
      if (!in_rect(filter, p)) continue;
      const double vx = q.velocity.x, vy = q.velocity.y;  // (the f32 of the device, widened by cs_read_agents)
      volatile double sx = vx * vx, sy = vy * vy;
      volatile double ss = sx + sy;
      if (!(ss < S2)) continue;
      volatile double mx = vx * g.t0, my = vy * g.t0;
      volatile double px = p.x + mx, py = p.y + my;
      volatile double rx = px - g.ax, ry = py - g.ay;
      volatile double a1 = ex * ry, a2 = ey * rx;
      volatile double c0 = a1 - a2;
      volatile double b1 = ex * vy, b2 = ey * vx;
      volatile double cv = b1 - b2;
      volatile double d1 = rx * vy, d2 = ry * vx;
      volatile double cu = d1 - d2;
      if (!((cv > 0.0 && c0 <= 0.0) || (cv < 0.0 && c0 >= 0.0))) continue;
      volatile double s = (-c0) / cv;
      if (!(s > 0.0)) s = 0.0;
      volatile double u = cu / cv;
      if (!(s < T && u >= 0.0 && u < 1.0)) continue;
      const int32_t dir = cv > 0.0 ? 1 : -1;
      out.push_back(cs_gate_crossing{(uint32_t)k, dir, q.agent_id, s, u});
      (*counts)[2 * k + (dir < 0)] += 1;
    }
  }
  return out;
}

template <class Sim>
static void agree(Sim& sim, const std::vector<cs_gate>& gates, double speed_max, const cs_selection* filter,
                  const std::vector<cs_gate_crossing>& want, const std::vector<uint64_t>& counts) {
  const std::vector<cs_gate_crossing> got = sim.gate_crossings(gates, speed_max, filter);
  CHECK(got.size() == want.size());
  CHECK(got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(cs_gate_crossing)) == 0);
  CHECK(sim.count_gate_crossings(gates, speed_max, filter) == counts);
  const std::size_t some = want.size() / 3;
  const std::vector<cs_gate_crossing> head = sim.gate_crossings(gates, speed_max, filter, some);
  CHECK(head.size() == some && (!some || std::memcmp(head.data(), want.data(), some * sizeof(cs_gate_crossing)) == 0));
}

int main() {
  static_assert(sizeof(cs_gate) == 48 && sizeof(cs_gate_crossing) == 32, "six doubles; two 4-byte and three 8-byte words");
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

  // doors of 2 m in both orientations and both windings through the crowd, lanes across the whole grid and beyond it,
  // along both cuts of the mesh (x = 30, y = 30), diagonals, a chain, windows that open later, a gate with A == B
  std::vector<cs_gate> gates;
  for (int k = 0; k < 40; ++k) {
    const double x = 18.0 + 0.55 * k, y = 17.0 + 0.6 * k;
    gates.push_back(cs_gate{x, y, x, y + 2.0, 0.0, 3.0});
    gates.push_back(cs_gate{x + 2.0, 50.0 - y, x, 50.0 - y, 0.0, 3.0});
    gates.push_back(cs_gate{x, y, x + 1.5, y + 1.5, 0.5 * (k % 4), 0.5 * (k % 4) + 2.0});
    gates.push_back(cs_gate{-5.0, 16.0 + 0.7 * k, 66.0, 16.5 + 0.7 * k, 0.0, 1.0 + 0.1 * k});
  }
  gates.push_back(cs_gate{30.0, -4.0, 30.0, 70.0, 0.0, 8.0});
  gates.push_back(cs_gate{70.0, 30.0, -4.0, 30.0, 0.0, 8.0});
  gates.push_back(cs_gate{25.0, 25.0, 25.0, 25.0, 0.0, 8.0});
  for (int k = 0; k < 10; ++k) gates.push_back(cs_gate{16.0 + 3.0 * k, 28.0, 19.0 + 3.0 * k, 28.0, 0.0, 6.0});
  cs_selection box{};
  box.terms = CS_SEL_RECT;
  box.x0 = 24.0; box.y0 = 22.5; box.x1 = 37.25; box.y1 = 36.0;  // across both cuts of the mesh
  std::size_t rows = 0, left = 0, right = 0, later = 0;
  std::vector<uint64_t> counts;
  const double speeds[3] = {INFINITY, 0.5, 2.0};
  for (const double speed_max : speeds) {
    for (const cs_selection* filter : {(const cs_selection*)nullptr, (const cs_selection*)&box}) {
      const std::vector<cs_gate_crossing> want = brute(one.agents, size, gates, speed_max, filter, &counts);
      rows += want.size();
      for (const cs_gate_crossing& r : want) {
        CHECK(0.0 <= r.s && r.s < gates[r.gate].t1 - gates[r.gate].t0 && 0.0 <= r.u && r.u < 1.0 && !std::signbit(r.s));
        left += r.dir == 1;
        right += r.dir == -1;
        later += r.s > 0.0;
      }
      agree(one, gates, speed_max, filter, want, counts);
      agree(mesh, gates, speed_max, filter, want, counts);
    }
  }
  std::printf("gate crossings: %zu rows compared, %zu to the left, %zu to the right, %zu after t0\n", rows, left, right, later);
  CHECK(rows > 500 && left > 50 && right > 50 && later > 50 && left + right == rows);
  // no gates at all
  CHECK(one.gate_crossings(std::vector<cs_gate>{}, 2.0).empty() && mesh.count_gate_crossings(std::vector<cs_gate>{}, 2.0).empty());

  // a refused call throws and the next one is right, on the engine and on the mesh
  int threw = 0;
  std::vector<cs_gate> bad = gates;
  bad[7].t1 = bad[7].t0 - 1.0;
  try {
    one.gate_crossings(bad, 2.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "gate_crossings: gate 7") != nullptr;
  }
  try {
    mesh.count_gate_crossings(gates, -1.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "gate_crossings") != nullptr;
  }
  CHECK(threw == 2);
  steps(one, 5);
  steps(mesh, 5);
  const std::vector<cs_gate_crossing> after = brute(one.agents, size, gates, 1.5, &box, &counts);
  agree(one, gates, 1.5, &box, after, counts);
  agree(mesh, gates, 1.5, &box, after, counts);
  std::printf("gate crossings: passed\n");
  return 0;
}
