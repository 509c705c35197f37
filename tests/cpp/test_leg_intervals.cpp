// Every agent that enters a timed leg from C++ (include/crowdsim.hpp over include/crowdstep_state.h): leg_intervals and
// count_leg_intervals on one engine and on a 2 x 2 mesh against a brute-force loop over `agents` by the rule the header
// writes: the same rows, byte for byte, with and without targets, with a limit, and a refused call throws.
// tests/test_gpu_leg_intervals_cpp.py builds and launches this on an MI355X.
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

// the rule of the header on `agents` (volatile: every operation rounded once), the rows ascending by (leg, id); rect:
// the targets (null: everyone)
template <class Map>
static std::vector<cs_leg_interval> brute(const Map& agents, double size, const std::vector<cs_leg>& legs, double distance,
                                          double speed_max, const cs_selection* targets, std::vector<uint64_t>* counts) {
  std::vector<const Agent*> order;
  for (const auto& kv : agents) order.push_back(&kv.second);
  std::sort(order.begin(), order.end(), [](const Agent* l, const Agent* r) { return l->agent_id < r->agent_id; });
  std::vector<cs_leg_interval> out;
  counts->assign(legs.size(), 0);
  volatile double D2 = distance * distance, S2 = speed_max * speed_max;
  for (std::size_t k = 0; k < legs.size(); ++k) {
    const cs_leg& l = legs[k];
    volatile double T = l.t1 - l.t0;
    for (const Agent* qp : order) {
      const Agent& q = *qp;
      const Point p = q.position;
      if (!(0.0 <= p.x && p.x < size && 0.0 <= p.y && p.y < size)) continue;
      if (q.agent_id == l.ignore || !in_rect(targets, p)) continue;
      const double vxq = q.velocity.x, vyq = q.velocity.y;  // (the f32 of the device, widened by cs_read_agents)
      volatile double sx = vxq * vxq, sy = vyq * vyq;
      volatile double ss = sx + sy;
      if (!(ss < S2)) continue;
      volatile double mx = vxq * l.t0, my = vyq * l.t0;
      volatile double px = p.x + mx, py = p.y + my;
      volatile double rx = px - l.x0, ry = py - l.y0;
      volatile double rxx = rx * rx, ryy = ry * ry;
      volatile double d2 = rxx + ryy;
      volatile double wx = vxq - l.vx, wy = vyq - l.vy;
      volatile double ax = rx * wx, ay = ry * wy;
      volatile double a = ax + ay;
      volatile double wxx = wx * wx, wyy = wy * wy;
      volatile double ww = wxx + wyy;
      volatile double c1 = rx * wy, c2 = ry * wx;
      volatile double cr = c1 - c2;
      volatile double dw = D2 * ww, cc = cr * cr;
      volatile double h2 = dw - cc;
      volatile double root = std::sqrt(h2);
      volatile double s = 0.0;
      if (!(d2 < D2)) {
        if (!(a < 0.0)) continue;
        if (!(h2 > 0.0)) continue;
        volatile double num = -a - root;
        s = num / ww;
        if (s < 0.0) s = 0.0;
      }
      if (!(s < T)) continue;
      volatile double e;
      if (!(h2 > 0.0)) {
        e = ww == 0.0 ? T : s;
      } else {
        volatile double num = -a + root;
        e = num / ww;
        if (!(e > s)) e = s;
        if (!(e < T)) e = T;
      }
      out.push_back(cs_leg_interval{(uint64_t)k, q.agent_id, s, e});
      (*counts)[k] += 1;
    }
  }
  return out;
}

template <class Sim>
static void agree(Sim& sim, const std::vector<cs_leg>& legs, double distance, double speed_max, const cs_selection* targets,
                  const std::vector<cs_leg_interval>& want, const std::vector<uint64_t>& counts) {
  const std::vector<cs_leg_interval> got = sim.leg_intervals(legs, distance, speed_max, targets);
  CHECK(got.size() == want.size());
  CHECK(got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(cs_leg_interval)) == 0);
  CHECK(sim.count_leg_intervals(legs, distance, speed_max, targets) == counts);
  const std::size_t some = want.size() / 3;
  const std::vector<cs_leg_interval> head = sim.leg_intervals(legs, distance, speed_max, targets, some);
  CHECK(head.size() == some && (!some || std::memcmp(head.data(), want.data(), some * sizeof(cs_leg_interval)) == 0));
}

int main() {
  static_assert(sizeof(cs_leg_interval) == 32, "four 8-byte words");
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

  // robot paths of 15 legs of 1 s from six agents (their ids ascending), each ignoring its agent, every third leg a
  // wait; long legs from outside the grid across both cuts of the mesh; waits on the cuts; legs that walk along with an
  // agent, with its very velocity
  std::vector<const Agent*> order;
  for (const auto& kv : one.agents) order.push_back(&kv.second);
  std::sort(order.begin(), order.end(), [](const Agent* l, const Agent* r) { return l->agent_id < r->agent_id; });
  std::vector<cs_leg> legs;
  for (std::size_t c = 0; c < 6; ++c) {
    const Agent& from = *order[c * 67 + 3];
    double x = from.position.x, y = from.position.y;
    for (int k = 0; k < 15; ++k) {
      const double vx = k % 3 == 2 ? 0.0 : 0.25 * (double)((k + (int)c) % 5 - 2), vy = k % 3 == 2 ? 0.0 : 0.25 * (double)(k % 4 - 1);
      legs.push_back(cs_leg{x, y, vx, vy, (double)k, (double)k + 1.0, from.agent_id});
      x = x + vx;
      y = y + vy;
    }
  }
  for (int k = 0; k < 40; ++k) {
    legs.push_back(cs_leg{-5.0, 16.0 + 0.7 * k, 2.0, 0.0, 0.0, 35.0, CS_NO_HIT});
    legs.push_back(cs_leg{17.0 + 0.6 * k, 66.0, 0.0, -4.0, 0.5, 12.0, CS_NO_HIT});
    legs.push_back(cs_leg{30.0, 18.0 + 0.6 * k, 0.0, 0.0, 0.25 * k, 0.25 * k + 4.0, CS_NO_HIT});
    legs.push_back(cs_leg{18.0 + 0.6 * k, 30.0, 0.0, 0.0, 0.0, 0.1 * k, CS_NO_HIT});
    const Agent& with = *order[k * 9 + 1];
    legs.push_back(cs_leg{with.position.x + 0.1, with.position.y, with.velocity.x, with.velocity.y, 0.0, 2.0, CS_NO_HIT});
  }
  cs_selection box{};
  box.terms = CS_SEL_RECT;
  box.x0 = 24.0; box.y0 = 22.5; box.x1 = 37.25; box.y1 = 36.0;  // across both cuts of the mesh
  std::size_t rows = 0, stays = 0, leaves = 0, at_zero = 0;
  std::vector<uint64_t> counts;
  const double queries[4][2] = {{0.5, INFINITY}, {1.0, 0.5}, {0.2, 2.0}, {0.0, INFINITY}};
  for (const auto& q : queries) {
    for (const cs_selection* targets : {(const cs_selection*)nullptr, (const cs_selection*)&box}) {
      const std::vector<cs_leg_interval> want = brute(one.agents, size, legs, q[0], q[1], targets, &counts);
      rows += want.size();
      for (const cs_leg_interval& r : want) {
        const double T = legs[r.leg].t1 - legs[r.leg].t0;
        CHECK(0.0 <= r.s_in && r.s_in <= r.s_out && r.s_out <= T);
        stays += r.s_out == T;
        leaves += r.s_out < T;
        at_zero += r.s_in == 0.0;
      }
      agree(one, legs, q[0], q[1], targets, want, counts);
      agree(mesh, legs, q[0], q[1], targets, want, counts);
    }
  }
  std::printf("leg intervals: %zu rows compared, %zu stay until the leg ends, %zu leave, %zu inside at the start\n", rows, stays,
              leaves, at_zero);
  CHECK(rows > 500 && stays > 50 && leaves > 50 && at_zero > 50 && at_zero < rows - 50);
  // no legs at all
  CHECK(one.leg_intervals(std::vector<cs_leg>{}, 0.5, 2.0).empty() && mesh.count_leg_intervals(std::vector<cs_leg>{}, 0.5, 2.0).empty());

  // a refused call throws and the next one is right, on the engine and on the mesh
  int threw = 0;
  std::vector<cs_leg> bad = legs;
  bad[7].t1 = bad[7].t0 - 1.0;
  try {
    one.leg_intervals(bad, 0.5, 2.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "leg_intervals: leg 7") != nullptr;
  }
  try {
    mesh.count_leg_intervals(legs, 0.5, -1.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "leg_intervals") != nullptr;
  }
  CHECK(threw == 2);
  steps(one, 5);
  steps(mesh, 5);
  const std::vector<cs_leg_interval> later = brute(one.agents, size, legs, 0.6, 1.5, &box, &counts);
  agree(one, legs, 0.6, 1.5, &box, later, counts);
  agree(mesh, legs, 0.6, 1.5, &box, later, counts);
  std::printf("leg intervals: passed\n");
  return 0;
}
