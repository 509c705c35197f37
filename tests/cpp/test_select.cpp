// Selecting, counting and removing agents by region, owner and state from C++ (include/crowdsim.hpp over
// include/crowdstep_state.h): a selection equals the filter of `agents` by the rule the header writes, a count equals the
// lengths, remove_selected equals remove_agents(select_agents(..)) on a twin, remove_source_sink(id, true) takes the
// sink's crowd with it, and a 2 x 2 mesh answers as one engine.  Runs on an MI355X (tests/test_gpu_select_cpp.py builds
// and launches it).
#include <algorithm>
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

static bool same(const Agent& a, const Agent& b) {
  return a.agent_id == b.agent_id && a.position.x == b.position.x && a.position.y == b.position.y &&
         a.velocity.x == b.velocity.x && a.velocity.y == b.velocity.y && a.next_waypoint == b.next_waypoint;
}
template <class Map>
static bool same_crowd(const Map& a, const Map& b) {
  if (a.size() != b.size()) return false;
  for (const auto& kv : a) {
    auto it = b.find(kv.first);
    if (it == b.end() || !same(kv.second, it->second)) return false;
  }
  return true;
}
template <class Sim>
static void steps(Sim& s, int n) {
  for (int k = 0; k < n; ++k) s.step(std::chrono::duration<double>(0.05));
}

// the geometric and state terms of the header, on an entry of `agents` (volatile: each product and sum rounded once)
static bool pred(const cs_selection& s, const Agent& a) {
  bool ok = true;
  const double x = a.position.x, y = a.position.y, vx = a.velocity.x, vy = a.velocity.y;
  if (s.terms & CS_SEL_RECT) ok = ok && s.x0 <= x && x < s.x1 && s.y0 <= y && y < s.y1;
  if (s.terms & CS_SEL_CIRCLE) {
    volatile double dx = x - s.cx, dy = y - s.cy;
    volatile double xx = dx * dx, yy = dy * dy, rr = s.r * s.r;
    volatile double d2 = xx + yy;
    ok = ok && d2 < rr;
  }
  if (s.terms & CS_SEL_WAYPOINT) ok = ok && s.wp_lo <= a.next_waypoint && a.next_waypoint <= s.wp_hi;
  if (s.terms & CS_SEL_SPEED) {
    volatile double xx = vx * vx, yy = vy * vy, lo = s.speed_lo * s.speed_lo, hi = s.speed_hi * s.speed_hi;
    volatile double v2 = xx + yy;
    ok = ok && lo <= v2 && v2 < hi;
  }
  return ok;
}
template <class Map>
static std::vector<AgentId> filter(const Map& agents, const cs_selection& s) {
  std::vector<AgentId> out;
  for (const auto& kv : agents)
    if (pred(s, kv.second)) out.push_back(kv.first);
  std::sort(out.begin(), out.end());
  return out;
}

struct Destroyed : EventListener {
  std::vector<AgentId> ids;
  void agent_spawned(Vec2f, AgentId) override {}
  void agent_destroyed(AgentId agent) override { ids.push_back(agent); }
};

static cs_selection rect(double x0, double y0, double x1, double y1) {
  cs_selection s{};
  s.terms = CS_SEL_RECT;
  s.x0 = x0; s.y0 = y0; s.x1 = x1; s.y1 = y1;
  return s;
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
  auto make_sink = [&]() {
    auto ss = std::make_shared<SourceSink>();
    ss->source = Vec2f{8.0, 50.0};
    ss->radius_sink = 0.5;
    ss->crowd_generator = std::make_shared<MonotonicCrowd>(10.0);
    ss->high_level_planner = std::make_shared<StubHighLevelPlan>(Vec2f{1.0, 0.0});
    ss->local_planner = zan;
    ss->waypoints = {Vec2f{55.0, 50.0}};
    ss->loop_forever = false;
    ss->agent_eyesight_range = 2.0;
    return ss;
  };

  // 1. one engine: a selection == the filter of `agents`, ascending; limits; counts
  Simulation a(grid), twin(grid);
  auto heard_a = std::make_shared<Destroyed>(), heard_twin = std::make_shared<Destroyed>();
  a.add_event_listener(heard_a);
  twin.add_event_listener(heard_twin);
  std::size_t sink_a = 0, sink_twin = 0;
  for (Simulation* s : {&a, &twin}) {
    s->add_agents(pts_e, east, zan, 2.0);
    s->add_agents(pts_w, west, zan, 2.0);
    (s == &a ? sink_a : sink_twin) = s->add_source_sink(make_sink());
  }
  steps(a, 30);
  steps(twin, 30);
  CHECK(same_crowd(a.agents, twin.agents));
  cs_selection circle{};
  circle.terms = CS_SEL_CIRCLE;
  circle.cx = 28.0; circle.cy = 29.0; circle.r = 6.5;
  cs_selection fast{};
  fast.terms = CS_SEL_SPEED | CS_SEL_RECT;
  fast.x0 = 0.0; fast.y0 = 0.0; fast.x1 = 33.3; fast.y1 = 60.0;
  fast.speed_lo = 0.45; fast.speed_hi = 10.0;
  cs_selection all{};
  cs_selection nobody = rect(5.0, 5.0, 5.0, 9.0);
  const std::vector<cs_selection> sels{rect(20.0, 18.5, 31.0, 33.25), circle, fast, all, nobody};
  const std::vector<uint64_t> counts = a.count_agents(sels);
  for (std::size_t k = 0; k < sels.size(); ++k) {
    const std::vector<AgentId> want = filter(a.agents, sels[k]);
    CHECK(a.select_agents(sels[k]) == want);
    CHECK(counts[k] == want.size());
    const std::vector<AgentId> few = a.select_agents(sels[k], 5);
    CHECK(few.size() == std::min<std::size_t>(5, want.size()) && std::equal(few.begin(), few.end(), want.begin()));
  }
  CHECK(!filter(a.agents, sels[0]).empty() && !filter(a.agents, fast).empty() && counts[3] == a.agents.size() && counts[4] == 0);
  // planners and owners
  cs_selection by_hlp{};
  by_hlp.terms = CS_SEL_HLP;
  by_hlp.hlp = a.planner_handle(west);
  CHECK(a.select_agents(by_hlp).size() == pts_w.size());
  by_hlp.hlp = a.planner_handle(std::make_shared<StubHighLevelPlan>(Vec2f{0.0, 0.0}));  // never used here
  CHECK(a.select_agents(by_hlp).empty());
  cs_selection of_sink{};
  of_sink.terms = CS_SEL_SOURCE_SINK;
  of_sink.source_sink = (uint32_t)sink_a;
  const std::vector<AgentId> spawned = a.select_agents(of_sink);
  CHECK(spawned.size() >= 2 && a.agents.size() == pts_e.size() + pts_w.size() + spawned.size());
  of_sink.source_sink = UINT32_MAX;
  CHECK(a.select_agents(of_sink).size() == pts_e.size() + pts_w.size());

  // 2. a refused selection throws and the next one is right
  bool threw = false;
  try {
    cs_selection bad{};
    bad.terms = 128u;
    a.select_agents(bad);
  } catch (const std::runtime_error& e) {
    threw = std::strstr(e.what(), "select_agents") != nullptr;
  }
  CHECK(threw);
  CHECK(a.select_agents(sels[0]) == filter(a.agents, sels[0]));

  // 3. remove_selected == remove_agents(select_agents(..)) on the twin: state, events, later steps
  const std::vector<AgentId> gone = a.remove_selected(sels[0]);
  twin.remove_agents(twin.select_agents(sels[0]));
  CHECK(!gone.empty() && heard_a->ids == gone && heard_twin->ids == gone);
  CHECK(same_crowd(a.agents, twin.agents));
  steps(a, 10);
  steps(twin, 10);
  CHECK(same_crowd(a.agents, twin.agents));

  // 4. remove_source_sink(id, true): the sink's crowd goes with it and nobody is spawned afterwards
  of_sink.source_sink = (uint32_t)sink_a;
  CHECK(!a.select_agents(of_sink).empty());
  a.remove_source_sink(sink_a, true);
  CHECK(a.select_agents(of_sink).empty());
  steps(a, 10);
  CHECK(a.select_agents(of_sink).empty());
  twin.remove_source_sink(sink_twin);  // (the default: the crowd walks on, and is still found by its owner)
  steps(twin, 10);
  of_sink.source_sink = (uint32_t)sink_twin;
  CHECK(!twin.select_agents(of_sink).empty());

  // 5. a 2 x 2 mesh against one engine: rectangles across the cuts
  TiledSimulation mesh(grid, 2, 2, 1);
  Simulation one(grid);
  mesh.add_agents(pts_e, east, zan, 2.0);
  one.add_agents(pts_e, east, zan, 2.0);
  mesh.add_agents(pts_w, west, zan, 2.0);
  one.add_agents(pts_w, west, zan, 2.0);
  steps(mesh, 5);
  steps(one, 5);
  const cs_selection across = rect(22.0, 20.0, 36.0, 38.0);
  CHECK(mesh.select_agents(across) == one.select_agents(across) && !one.select_agents(across).empty());
  CHECK(mesh.select_agents(across) == filter(one.agents, across));
  CHECK(mesh.count_agents(sels) == one.count_agents(sels));
  CHECK(mesh.remove_selected(across) == one.remove_selected(across));
  CHECK(same_crowd(mesh.agents, one.agents));
  steps(mesh, 10);
  steps(one, 10);
  CHECK(same_crowd(mesh.agents, one.agents));
  std::printf("select: passed\n");
  return 0;
}
