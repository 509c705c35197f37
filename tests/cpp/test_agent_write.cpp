// Writing agents between steps from C++ (include/crowdsim.hpp over include/crowdstep_state.h): a read -> write round
// trip that changes nothing, a refused batch that changes nothing, and a
// 2 x 2 mesh whose written agent moves to the diagonal tile, against one engine.  Runs on an MI355X
// (tests/test_gpu_agent_write.py builds and launches it).
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

int main() {
  const LocationHash2D grid(60.0, 60.0, 2.0, Point{0.0, 0.0});
  auto plan = std::make_shared<StubHighLevelPlan>(Vec2f{0.3, 0.2});
  auto zan = std::make_shared<Zanlungo>(1.0, 1.0, 0.0, 0.4, 2.0, 0.2);
  std::vector<Point> pts;
  for (int ix = 0; ix < 20; ++ix)
    for (int iy = 0; iy < 20; ++iy) pts.push_back(Point{18.0 + 1.1 * ix + 0.01 * iy, 17.0 + 1.2 * iy + 0.02 * ix});

  // 1. round trip: read, write back unchanged (all fields), step: equal to an untouched twin
  Simulation a(grid), twin(grid);
  a.add_agents(pts, plan, zan, 2.0);
  twin.add_agents(pts, plan, zan, 2.0);
  for (int s = 0; s < 5; ++s) {
    a.step(std::chrono::duration<double>(0.05));
    twin.step(std::chrono::duration<double>(0.05));
  }
  std::vector<Agent> all;
  for (const auto& kv : a.agents) all.push_back(kv.second);
  a.write_agents(all);
  CHECK(same_crowd(a.agents, twin.agents));
  for (int s = 0; s < 10; ++s) {
    a.step(std::chrono::duration<double>(0.05));
    twin.step(std::chrono::duration<double>(0.05));
  }
  CHECK(same_crowd(a.agents, twin.agents));

  // 2. a refused batch (an id given twice) throws and changes nothing
  std::vector<Agent> twice{all[0], all[0]};
  bool threw = false;
  try {
    a.write_agents(twice);
  } catch (const std::runtime_error& e) {
    threw = std::strstr(e.what(), "twice") != nullptr;
  }
  CHECK(threw);
  CHECK(same_crowd(a.agents, twin.agents));

  // 3. a 2 x 2 mesh: agent 0 teleported to the diagonal tile with a new velocity, the same write on one engine; the two
  //    stay equal, bit for bit, through the steps that follow
  TiledSimulation mesh(grid, 2, 2, 1);
  Simulation one(grid);
  const auto ids_m = mesh.add_agents(pts, plan, zan, 2.0);
  const auto ids_1 = one.add_agents(pts, plan, zan, 2.0);
  CHECK(ids_m == ids_1);
  for (int s = 0; s < 3; ++s) {
    mesh.step(std::chrono::duration<double>(0.05));
    one.step(std::chrono::duration<double>(0.05));
  }
  CHECK(same_crowd(mesh.agents, one.agents));
  Agent moved = one.agents.at(ids_1[0]);  // (starts in the tile of the low x rows and low y columns)
  moved.position = Point{47.25, 51.875};
  moved.velocity = Vec2f{-0.25, 0.125};
  mesh.write_agents(std::vector<Agent>{moved}, CS_WRITE_POSITION | CS_WRITE_VELOCITY);
  one.write_agents(std::vector<Agent>{moved}, CS_WRITE_POSITION | CS_WRITE_VELOCITY);
  CHECK(mesh.agents.at(ids_1[0]).position.x == 47.25 && mesh.agents.at(ids_1[0]).position.y == 51.875);
  CHECK(same_crowd(mesh.agents, one.agents));
  for (int s = 0; s < 10; ++s) {
    mesh.step(std::chrono::duration<double>(0.05));
    one.step(std::chrono::duration<double>(0.05));
  }
  CHECK(same_crowd(mesh.agents, one.agents));
  std::printf("agent write: passed\n");
  return 0;
}
