// Sending agents to goals by id in batches from C++ (include/crowdsim.hpp over include/crowdstep_state.h): a batch is
// planned and booked in batch order, a refused batch throws and calls no planner, and a 2 x 2 mesh does the same as one
// engine.  Prints the statuses and the crowd after 20 steps; tests/test_gpu_set_targets.py runs the same scene through
// the Python layer and compares.  Runs on an MI355X.
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

// start, a point 2 to the left of the midpoint, goal (the DoglegRoutes of the Python tests)
struct Doglegs : RouteFollower {
  std::vector<std::pair<Point, Point>> calls;
  std::vector<Point> plan_route(Point s, Point g) override {
    calls.push_back({s, g});
    if (g.x > 900.0) return {};
    const double mx = 0.5 * (s.x + g.x), my = 0.5 * (s.y + g.y), dx = g.x - s.x, dy = g.y - s.y;
    double n = std::hypot(dx, dy);
    if (n == 0.0) n = 1.0;
    return {s, Point{mx - 2.0 * dy / n, my + 2.0 * dx / n}, g};
  }
};

template <class Sim>
static void steps(Sim& s, int n) {
  for (int k = 0; k < n; ++k) s.step(std::chrono::duration<double>(0.1));
}
template <class A, class B>
static bool same_crowd(const A& a, const B& b) {
  if (a.size() != b.size()) return false;
  for (const auto& kv : a) {
    auto it = b.find(kv.first);
    if (it == b.end() || kv.second.position.x != it->second.position.x || kv.second.position.y != it->second.position.y ||
        kv.second.velocity.x != it->second.velocity.x || kv.second.velocity.y != it->second.velocity.y)
      return false;
  }
  return true;
}

int main() {
  const LocationHash2D grid(80.0, 80.0, 2.0, Point{0.0, 0.0});
  auto none = std::make_shared<NoLocalPlan>();
  std::vector<Point> pts;
  for (int ix = 0; ix < 6; ++ix)
    for (int iy = 0; iy < 6; ++iy) pts.push_back(Point{30.0 + 1.5 * ix, 34.0 + 1.5 * iy});
  auto make = [] {
    auto f = std::make_shared<Doglegs>();
    f->scale = 4.0;
    f->speed = 1.2;
    return f;
  };

  auto hlp = make();
  Simulation sim(grid);
  const auto ids = sim.add_agents(pts, hlp, none, 2.0);
  std::vector<Point> goals(ids.size(), Point{60.0, 20.0});
  goals[5] = Point{1000.0, 20.0};  // no contiguous path

  // a refused batch: throws, no planner called
  std::vector<AgentId> bad(ids);
  bad[7] = 1000000;
  bool threw = false;
  try {
    sim.set_targets(bad, goals);
  } catch (const std::runtime_error& e) {
    threw = std::strstr(e.what(), "unknown agent id") != nullptr;
  }
  CHECK(threw && hlp->calls.empty());

  const std::vector<uint8_t> st = sim.set_targets(ids, goals);
  CHECK(st.size() == ids.size() && st[0] == CS_TARGET_PLANNED && st[5] == CS_TARGET_NO_PATH);
  std::size_t planned = 0, booked = 0;
  for (uint8_t s : st) {
    planned += s == CS_TARGET_PLANNED;
    booked += s == CS_TARGET_BOOKED;
  }
  CHECK(planned + booked + 1 == ids.size() && booked > planned && hlp->calls.size() == planned + 1);
  CHECK(hlp->calls[0].first.x == pts[0].x && hlp->calls[0].first.y == pts[0].y);
  steps(sim, 20);
  CHECK(sim.agents.at(ids[5]).position.x == pts[5].x && sim.agents.at(ids[0]).position.x != pts[0].x);
  const std::vector<uint8_t> again = sim.set_targets({ids[5]}, {Point{60.0, 20.0}}, Vec2f{0.5, 0.5});
  CHECK(again.size() == 1 && (again[0] == CS_TARGET_PLANNED || again[0] == CS_TARGET_BOOKED));
  steps(sim, 5);

  std::printf("statuses");
  for (uint8_t s : st) std::printf(" %u", (unsigned)s);
  std::printf(" %u\n", (unsigned)again[0]);
  for (AgentId id : ids) {
    const Agent& a = sim.agents.at(id);
    std::printf("agent %llu %.17g %.17g %.17g %.17g\n", (unsigned long long)id, a.position.x, a.position.y, a.velocity.x,
                a.velocity.y);
  }

  // a 2 x 2 mesh does the same as one engine
  auto hlp_m = make();
  TiledSimulation mesh(grid, 2, 2, 1);
  const auto ids_m = mesh.add_agents(pts, hlp_m, none, 2.0);
  CHECK(ids_m == ids);
  threw = false;
  try {
    mesh.set_targets(bad, goals);
  } catch (const std::runtime_error& e) {
    threw = std::strstr(e.what(), "unknown agent id") != nullptr;
  }
  CHECK(threw && hlp_m->calls.empty());
  CHECK(mesh.set_targets(ids_m, goals) == st);
  steps(mesh, 20);
  CHECK(mesh.set_targets({ids[5]}, {Point{60.0, 20.0}}, Vec2f{0.5, 0.5}) == again);
  steps(mesh, 5);
  CHECK(same_crowd(mesh.agents, sim.agents));
  std::printf("set targets: passed\n");
  return 0;
}
