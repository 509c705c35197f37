// Reading and removing agents by id in batches from C++ (include/crowdsim.hpp over include/crowdstep_state.h): a batched
// read equals the entries of `agents`, a batched remove equals the loop of single removes on a twin, a refused batch
// throws and removes nothing, and a 2 x 2 mesh does the same as one engine.  Runs on an MI355X
// (tests/test_gpu_agents_by_id.py builds and launches it).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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
         a.velocity.x == b.velocity.x && a.velocity.y == b.velocity.y && a.next_waypoint == b.next_waypoint &&
         a.eyesight_range == b.eyesight_range;
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

struct Destroyed : EventListener {
  std::vector<AgentId> ids;
  void agent_spawned(Vec2f, AgentId) override {}
  void agent_destroyed(AgentId agent) override { ids.push_back(agent); }
};

int main() {
  const LocationHash2D grid(60.0, 60.0, 2.0, Point{0.0, 0.0});
  auto plan = std::make_shared<StubHighLevelPlan>(Vec2f{0.3, 0.2});
  auto zan = std::make_shared<Zanlungo>(1.0, 1.0, 0.0, 0.4, 2.0, 0.2);
  std::vector<Point> pts;
  for (int ix = 0; ix < 20; ++ix)
    for (int iy = 0; iy < 20; ++iy) pts.push_back(Point{18.0 + 1.1 * ix + 0.01 * iy, 17.0 + 1.2 * iy + 0.02 * ix});

  // 1. one engine: read by id == the entries of `agents`, in the order asked, repeats answered
  Simulation a(grid), twin(grid);
  auto heard_a = std::make_shared<Destroyed>(), heard_twin = std::make_shared<Destroyed>();
  a.add_event_listener(heard_a);
  twin.add_event_listener(heard_twin);
  const auto ids = a.add_agents(pts, plan, zan, 2.0);
  twin.add_agents(pts, plan, zan, 2.0);
  steps(a, 5);
  steps(twin, 5);
  std::vector<AgentId> ask;
  for (std::size_t k = 0; k < ids.size(); k += 7) ask.push_back(ids[ids.size() - 1 - k]);
  ask.push_back(ask[0]);
  const std::vector<Agent> got = a.read_agents(ask);
  CHECK(got.size() == ask.size());
  for (std::size_t k = 0; k < ask.size(); ++k) CHECK(same(got[k], a.agents.at(ask[k])));
  ask.pop_back();

  // 2. a missing id: throws without `found`, flagged with it
  std::vector<AgentId> some{ids[3], (AgentId)1000000, ids[4]};
  bool threw = false;
  try {
    a.read_agents(some);
  } catch (const std::runtime_error& e) {
    threw = std::strstr(e.what(), "unknown agent id") != nullptr;
  }
  CHECK(threw);
  std::vector<uint8_t> found;
  const std::vector<Agent> part = a.read_agents(some, &found);
  CHECK(found.size() == 3 && found[0] == 1 && found[1] == 0 && found[2] == 1);
  CHECK(part[1].agent_id == 1000000 && part[1].position.x == 0.0 && same(part[2], a.agents.at(ids[4])));

  // 3. a refused remove (an id twice; an unknown id) throws and removes nothing
  for (int which = 0; which < 2; ++which) {
    std::vector<AgentId> bad{ids[0], ids[1], which ? (AgentId)1000000 : ids[0]};
    threw = false;
    try {
      a.remove_agents(bad);
    } catch (const std::runtime_error& e) {
      threw = std::strstr(e.what(), which ? "unknown agent id" : "twice") != nullptr;
    }
    CHECK(threw);
    CHECK(same_crowd(a.agents, twin.agents) && heard_a->ids.empty());
  }

  // 4. one batched remove == the loop of single removes: state, events in the order of the batch, later steps
  a.remove_agents(ask);
  for (AgentId id : ask) twin.remove_agents(id);
  CHECK(a.agents.size() == ids.size() - ask.size());
  CHECK(same_crowd(a.agents, twin.agents));
  CHECK(heard_a->ids == ask && heard_twin->ids == ask);
  steps(a, 10);
  steps(twin, 10);
  CHECK(same_crowd(a.agents, twin.agents));

  // 5. a 2 x 2 mesh against one engine: the batch spans all four tiles
  TiledSimulation mesh(grid, 2, 2, 1);
  Simulation one(grid);
  const auto ids_m = mesh.add_agents(pts, plan, zan, 2.0);
  const auto ids_1 = one.add_agents(pts, plan, zan, 2.0);
  CHECK(ids_m == ids_1);
  steps(mesh, 3);
  steps(one, 3);
  std::vector<AgentId> span;
  for (std::size_t k = 0; k < ids_1.size(); k += 9) span.push_back(ids_1[k]);
  const std::vector<Agent> from_mesh = mesh.read_agents(span), from_one = one.read_agents(span);
  for (std::size_t k = 0; k < span.size(); ++k) CHECK(same(from_mesh[k], from_one[k]));
  std::vector<AgentId> bad(span);
  bad.push_back((AgentId)1000000);
  threw = false;
  try {
    mesh.remove_agents(bad);
  } catch (const std::runtime_error& e) {
    threw = std::strstr(e.what(), "unknown agent id") != nullptr;
  }
  CHECK(threw);
  CHECK(same_crowd(mesh.agents, one.agents));
  mesh.remove_agents(span);
  one.remove_agents(span);
  CHECK(mesh.agents.size() == ids_1.size() - span.size());
  CHECK(same_crowd(mesh.agents, one.agents));
  steps(mesh, 10);
  steps(one, 10);
  CHECK(same_crowd(mesh.agents, one.agents));
  std::printf("agents by id: passed\n");
  return 0;
}
