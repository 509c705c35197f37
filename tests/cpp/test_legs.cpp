// Paths against the moving crowd from C++ (include/crowdsim.hpp over include/crowdstep_state.h): leg_conflicts and
// count_leg_conflicts on one engine and on a 2 x 2 mesh against a brute-force loop over `agents` by the rule the header
// writes: the same rows, byte for byte, with and without targets, and a refused call throws.  It prints the number of
// conflicts and a checksum of the bits of one query, which tests/test_gpu_leg_conflicts_cpp.py (it builds and launches
// this on an MI355X) compares with what the Python side computes for the same scene.
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

// the rule of the header on `agents` (volatile: every operation rounded once); rect: the targets (null: everyone)
template <class Map>
static std::vector<cs_leg_hit> brute(const Map& agents, double size, const std::vector<cs_leg>& legs, double distance,
                                     double speed_max, const cs_selection* targets) {
  std::vector<cs_leg_hit> out;
  volatile double D2 = distance * distance, S2 = speed_max * speed_max;
  for (const cs_leg& l : legs) {
    cs_leg_hit best{CS_NO_HIT, INFINITY};
    volatile double T = l.t1 - l.t0;
    for (const auto& kv : agents) {
      const Agent& q = kv.second;
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
      volatile double s = 0.0;
      if (!(d2 < D2)) {
        volatile double wx = vxq - l.vx, wy = vyq - l.vy;
        volatile double ax = rx * wx, ay = ry * wy;
        volatile double a = ax + ay;
        if (!(a < 0.0)) continue;
        volatile double wxx = wx * wx, wyy = wy * wy;
        volatile double ww = wxx + wyy;
        volatile double c1 = rx * wy, c2 = ry * wx;
        volatile double cr = c1 - c2;
        volatile double dw = D2 * ww, cc = cr * cr;
        volatile double h2 = dw - cc;
        if (!(h2 > 0.0)) continue;
        volatile double root = std::sqrt(h2);
        volatile double num = -a - root;
        s = num / ww;
        if (s < 0.0) s = 0.0;
      }
      if (!(s < T)) continue;
      if (s < best.s || (s == best.s && q.agent_id < best.id)) best = cs_leg_hit{q.agent_id, s};
    }
    out.push_back(best);
  }
  return out;
}

static std::size_t hits_of(const std::vector<cs_leg_hit>& rows) {
  return (std::size_t)std::count_if(rows.begin(), rows.end(), [](const cs_leg_hit& h) { return h.id != CS_NO_HIT; });
}

static void agree(const std::vector<cs_leg_hit>& got, std::size_t count, const std::vector<cs_leg_hit>& want) {
  CHECK(count == hits_of(want));
  CHECK(got.size() == want.size());
  CHECK(got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(cs_leg_hit)) == 0);
}

int main() {
  static_assert(sizeof(cs_leg) == 56 && sizeof(cs_leg_hit) == 16, "seven and two 8-byte words");
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
  // wait; long legs from outside the grid across both cuts of the mesh (30 m), some of them parallel to an axis; waits
  // on the cuts
  std::vector<const Agent*> order;
  for (const auto& kv : one.agents) order.push_back(&kv.second);
  std::sort(order.begin(), order.end(), [](const Agent* l, const Agent* r) { return l->agent_id < r->agent_id; });
  std::vector<cs_leg> legs;
  for (std::size_t c = 0; c < 6; ++c) {
    const Agent& from = *order[c * 67 + 3];
    double x = from.position.x, y = from.position.y;
    for (int k = 0; k < 15; ++k) {  // (velocities from small integers: the Python side forms the same bits)
      const double vx = k % 3 == 2 ? 0.0 : 0.25 * (double)((k + (int)c) % 5 - 2), vy = k % 3 == 2 ? 0.0 : 0.25 * (double)(k % 4 - 1);
      legs.push_back(cs_leg{x, y, vx, vy, (double)k, (double)k + 1.0, from.agent_id});
      x = x + vx;
      y = y + vy;
    }
  }
  for (int k = 0; k < 60; ++k) {
    legs.push_back(cs_leg{-5.0, 16.0 + 0.45 * k, 2.0, 0.0, 0.0, 35.0, CS_NO_HIT});
    legs.push_back(cs_leg{17.0 + 0.4 * k, 66.0, 0.0, -4.0, 0.5, 12.0, CS_NO_HIT});
    legs.push_back(cs_leg{64.0, 50.0 - 0.5 * k, -1.0, -0.25 + 0.01 * k, 1.0, 1.0 + 0.5 * k, CS_NO_HIT});
    legs.push_back(cs_leg{30.0, 18.0 + 0.4 * k, 0.0, 0.0, 0.25 * k, 0.25 * k + 4.0, CS_NO_HIT});
    legs.push_back(cs_leg{18.0 + 0.4 * k, 30.0, 0.0, 0.0, 0.0, 0.1 * k, CS_NO_HIT});
  }
  cs_selection box{};
  box.terms = CS_SEL_RECT;
  box.x0 = 24.0; box.y0 = 22.5; box.x1 = 37.25; box.y1 = 36.0;  // across both cuts of the mesh
  std::size_t rows = 0, hits = 0, at_zero = 0;
  const double queries[4][2] = {{0.5, INFINITY}, {1.0, 0.5}, {0.2, 2.0}, {0.0, INFINITY}};
  for (const auto& q : queries) {
    for (const cs_selection* targets : {(const cs_selection*)nullptr, (const cs_selection*)&box}) {
      const std::vector<cs_leg_hit> want = brute(one.agents, size, legs, q[0], q[1], targets);
      rows += want.size();
      hits += hits_of(want);
      for (const cs_leg_hit& h : want) at_zero += h.id != CS_NO_HIT && h.s == 0.0;
      agree(one.leg_conflicts(legs, q[0], q[1], targets), one.count_leg_conflicts(legs, q[0], q[1], targets), want);
      agree(mesh.leg_conflicts(legs, q[0], q[1], targets), mesh.count_leg_conflicts(legs, q[0], q[1], targets), want);
    }
  }
  std::printf("legs: %zu rows compared, %zu conflicts, %zu of them at s == 0\n", rows, hits, at_zero);
  CHECK(rows == 8 * legs.size() && hits > 100 && hits < rows - 100 && at_zero > 10);
  // what the Python side recomputes for this scene: the conflicts and the xor of the bits of every row
  const std::vector<cs_leg_hit> all = one.leg_conflicts(legs, 0.5, 2.0);
  uint64_t x_ids = 0, x_s = 0;
  for (std::size_t k = 0; k < all.size(); ++k) {
    uint64_t s_bits;
    std::memcpy(&s_bits, &all[k].s, 8);
    x_ids ^= all[k].id * (uint64_t)(2 * k + 1);
    x_s ^= s_bits;
  }
  std::printf("legs: check 0.5 2.0 legs %zu conflicts %zu ids %016llx s %016llx\n", all.size(), hits_of(all),
              (unsigned long long)x_ids, (unsigned long long)x_s);
  // no legs at all
  CHECK(one.leg_conflicts(std::vector<cs_leg>{}, 0.5, 2.0).empty() &&
        mesh.count_leg_conflicts(std::vector<cs_leg>{}, 0.5, 2.0) == 0);

  // a refused call throws and the next one is right, on the engine and on the mesh
  int threw = 0;
  std::vector<cs_leg> bad = legs;
  bad[7].t1 = bad[7].t0 - 1.0;
  try {
    one.leg_conflicts(bad, 0.5, 2.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "leg_conflicts: leg 7") != nullptr;
  }
  try {
    mesh.leg_conflicts(legs, 0.5, -1.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "leg_conflicts") != nullptr;
  }
  CHECK(threw == 2);
  steps(one, 5);
  steps(mesh, 5);
  const std::vector<cs_leg_hit> later = brute(one.agents, size, legs, 0.6, 1.5, &box);
  agree(one.leg_conflicts(legs, 0.6, 1.5, &box), one.count_leg_conflicts(legs, 0.6, 1.5, &box), later);
  agree(mesh.leg_conflicts(legs, 0.6, 1.5, &box), mesh.count_leg_conflicts(legs, 0.6, 1.5, &box), later);
  std::printf("legs: passed\n");
  return 0;
}
