// The clusters of agents under a distance from C++ (include/crowdsim.hpp over include/crowdstep_state.h): agent_clusters and
// count_clusters on one engine and on a 2 x 2 mesh against a brute-force double loop plus a union-find over `agents` by
// the rules the header writes: the same ids, labels, sizes and boxes, the sums under their bound, with and without a
// selection and a min_size, and a refused call throws.  Runs on an MI355X (tests/test_gpu_clusters_cpp.py builds and
// launches it).
#include <algorithm>
#include <cmath>
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

template <class Sim>
static void steps(Sim& s, int n) {
  for (int k = 0; k < n; ++k) s.step(std::chrono::duration<double>(0.05));
}

struct Want {
  std::vector<uint64_t> ids, labels;
  std::vector<cs_cluster> clusters;
  std::vector<double> abs_x, abs_y;  // sum|x|, sum|y| per cluster, for the bound of the sums
};

// the rules of the header on `agents` (volatile: every operation rounded once); rect: the members (null: everyone)
template <class Map>
static Want brute(const Map& agents, double size, double distance, const cs_selection* rect, uint64_t min_size) {
  std::vector<const Agent*> part;
  for (const auto& kv : agents) {
    const Point p = kv.second.position;
    if (!(0.0 <= p.x && p.x < size && 0.0 <= p.y && p.y < size)) continue;
    if (rect && !(rect->x0 <= p.x && p.x < rect->x1 && rect->y0 <= p.y && p.y < rect->y1)) continue;
    part.push_back(&kv.second);
  }
  std::sort(part.begin(), part.end(), [](const Agent* l, const Agent* r) { return l->agent_id < r->agent_id; });
  std::vector<std::size_t> parent(part.size());
  for (std::size_t i = 0; i < parent.size(); ++i) parent[i] = i;
  auto find = [&](std::size_t x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  volatile double dist2 = distance * distance;
  for (std::size_t i = 0; i < part.size(); ++i)
    for (std::size_t j = i + 1; j < part.size(); ++j) {
      volatile double dx = part[i]->position.x - part[j]->position.x, dy = part[i]->position.y - part[j]->position.y;
      volatile double xx = dx * dx, yy = dy * dy;
      volatile double d2 = xx + yy;
      if (!(d2 < dist2)) continue;
      const std::size_t a = find(i), b = find(j);
      if (a != b) parent[std::max(a, b)] = std::min(a, b);  // (sorted by id: the smaller index is the smaller id)
    }
  std::map<uint64_t, std::vector<std::size_t>> by_label;
  for (std::size_t i = 0; i < part.size(); ++i) by_label[part[find(i)]->agent_id].push_back(i);
  Want out;
  std::vector<std::pair<uint64_t, uint64_t>> members;
  for (const auto& kv : by_label) {
    if (kv.second.size() < std::max<uint64_t>(min_size, 1)) continue;
    cs_cluster c{};
    c.label = kv.first;
    c.size = kv.second.size();
    c.min_x = c.min_y = INFINITY;
    c.max_x = c.max_y = -INFINITY;
    double ax = 0.0, ay = 0.0;
    long double sx = 0.0L, sy = 0.0L;  // (64 bits of mantissa: the rounded sum, but for 2^-64 per term)
    for (std::size_t i : kv.second) {
      const Point p = part[i]->position;
      c.min_x = std::min(c.min_x, p.x);
      c.min_y = std::min(c.min_y, p.y);
      c.max_x = std::max(c.max_x, p.x);
      c.max_y = std::max(c.max_y, p.y);
      sx += (long double)p.x;
      sy += (long double)p.y;
      ax += std::fabs(p.x);
      ay += std::fabs(p.y);
      members.push_back({part[i]->agent_id, kv.first});
    }
    c.sum_x = (double)sx;
    c.sum_y = (double)sy;
    out.clusters.push_back(c);
    out.abs_x.push_back(ax);
    out.abs_y.push_back(ay);
  }
  std::sort(members.begin(), members.end());
  for (const auto& m : members) {
    out.ids.push_back(m.first);
    out.labels.push_back(m.second);
  }
  return out;
}

// ids, labels, sizes and boxes exactly; the sums within size * 2^-52 * sum|x| of the rounded sum
static void agree(const AgentClusters& got, const ClusterCounts& counts, const Want& want) {
  CHECK(counts.agents == want.ids.size() && counts.clusters == want.clusters.size());
  CHECK(got.ids == want.ids && got.labels == want.labels);
  CHECK(got.clusters.size() == want.clusters.size());
  for (std::size_t k = 0; k < want.clusters.size(); ++k) {
    const cs_cluster &g = got.clusters[k], &w = want.clusters[k];
    CHECK(g.label == w.label && g.size == w.size);
    CHECK(g.min_x == w.min_x && g.min_y == w.min_y && g.max_x == w.max_x && g.max_y == w.max_y);
    const double eps = (double)w.size * std::ldexp(1.0, -52);
    CHECK(std::fabs(g.sum_x - w.sum_x) <= eps * want.abs_x[k] && std::fabs(g.sum_y - w.sum_y) <= eps * want.abs_y[k]);
    if (w.size == 1) CHECK(g.sum_x == w.min_x && g.sum_y == w.min_y);
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
  std::size_t multi = 0, total = 0;
  for (double distance : {0.0, 1.0, 1.25, 2.0}) {  // (2.0: the most a mesh with one halo cell of 2 m allows)
    for (const cs_selection* sel : {(const cs_selection*)nullptr, (const cs_selection*)&box}) {
      for (uint64_t min_size : {(uint64_t)1, (uint64_t)3}) {
        const Want want = brute(one.agents, size, distance, sel, min_size);
        total += want.clusters.size();
        for (const cs_cluster& c : want.clusters) multi += c.size > 1;
        agree(one.agent_clusters(distance, sel, min_size), one.count_clusters(distance, sel, min_size), want);
        agree(mesh.agent_clusters(distance, sel, min_size), mesh.count_clusters(distance, sel, min_size), want);
      }
    }
  }
  CHECK(total > 500 && multi > 10);
  const Want all = brute(one.agents, size, INFINITY, nullptr, 1);
  CHECK(all.clusters.size() == 1 && all.clusters[0].size == 400);
  agree(one.agent_clusters(INFINITY), one.count_clusters(INFINITY), all);

  // a refused call throws and the next one is right, on the engine and on the mesh
  int threw = 0;
  try {
    one.agent_clusters(-1.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "agent_clusters") != nullptr;
  }
  try {
    mesh.agent_clusters(2.5);  // above halo_cells * cell_size
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "agent_clusters") != nullptr;
  }
  CHECK(threw == 2);
  steps(one, 5);
  steps(mesh, 5);
  const Want later = brute(one.agents, size, 1.25, nullptr, 2);
  agree(one.agent_clusters(1.25, nullptr, 2), one.count_clusters(1.25, nullptr, 2), later);
  agree(mesh.agent_clusters(1.25, nullptr, 2), mesh.count_clusters(1.25, nullptr, 2), later);
  std::printf("clusters: passed\n");
  return 0;
}
