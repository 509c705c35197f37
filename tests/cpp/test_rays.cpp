// Rays against the crowd from C++ (include/crowdsim.hpp over include/crowdstep_state.h): cast_rays and count_ray_hits on
// one engine and on a 2 x 2 mesh against a brute-force loop over `agents` by the rule the header writes: the same rows,
// byte for byte, with and without targets, and a refused call throws.  It prints the number of hits and a checksum of
// the bits of one query, which tests/test_gpu_rays_cpp.py (it builds and launches this on an MI355X) compares with what the
// Python side computes for the same scene.
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
static std::vector<cs_ray_hit> brute(const Map& agents, double size, const std::vector<cs_ray>& rays, double radius,
                                     const cs_selection* targets) {
  std::vector<cs_ray_hit> out;
  volatile double R2 = radius * radius;
  for (const cs_ray& r : rays) {
    cs_ray_hit best{CS_NO_HIT, INFINITY};
    volatile double uxx = r.ux * r.ux, uyy = r.uy * r.uy;
    volatile double uu = uxx + uyy;
    for (const auto& kv : agents) {
      const Agent& q = kv.second;
      const Point p = q.position;
      if (!(0.0 <= p.x && p.x < size && 0.0 <= p.y && p.y < size)) continue;
      if (q.agent_id == r.ignore || !in_rect(targets, p)) continue;
      volatile double rx = p.x - r.ox, ry = p.y - r.oy;
      volatile double rxx = rx * rx, ryy = ry * ry;
      volatile double d2 = rxx + ryy;
      volatile double t = 0.0;
      if (!(d2 < R2)) {
        volatile double bx = rx * r.ux, by = ry * r.uy;
        volatile double b = bx + by;
        if (!(b > 0.0)) continue;
        volatile double c1 = rx * r.uy, c2 = ry * r.ux;
        volatile double cr = c1 - c2;
        volatile double ru = R2 * uu, cc = cr * cr;
        volatile double h2 = ru - cc;
        if (!(h2 > 0.0)) continue;
        volatile double root = std::sqrt(h2);
        volatile double num = b - root;
        t = num / uu;
        if (t < 0.0) t = 0.0;
      }
      if (!(t < r.t_max)) continue;
      if (t < best.t || (t == best.t && q.agent_id < best.id)) best = cs_ray_hit{q.agent_id, t};
    }
    out.push_back(best);
  }
  return out;
}

static std::size_t hits_of(const std::vector<cs_ray_hit>& rows) {
  return (std::size_t)std::count_if(rows.begin(), rows.end(), [](const cs_ray_hit& h) { return h.id != CS_NO_HIT; });
}

static void agree(const std::vector<cs_ray_hit>& got, std::size_t count, const std::vector<cs_ray_hit>& want) {
  CHECK(count == hits_of(want));
  CHECK(got.size() == want.size());
  CHECK(got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(cs_ray_hit)) == 0);
}

int main() {
  static_assert(sizeof(cs_ray) == 48 && sizeof(cs_ray_hit) == 16, "six and two 8-byte words");
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

  // fans of 90 beams from six agents (their ids ascending), each ignoring its caster, and a grid of long segments
  // from outside the grid across both cuts of the mesh (30 m), some of them parallel to an axis
  std::vector<const Agent*> order;
  for (const auto& kv : one.agents) order.push_back(&kv.second);
  std::sort(order.begin(), order.end(), [](const Agent* l, const Agent* r) { return l->agent_id < r->agent_id; });
  std::vector<cs_ray> rays;
  for (std::size_t c = 0; c < 6; ++c) {
    const Agent& from = *order[c * 67 + 3];
    for (int k = 0; k < 90; ++k)  // (directions from small integers: the Python side forms the same bits)
      rays.push_back(cs_ray{from.position.x, from.position.y, (double)(k % 10) - 4.5, (double)(k / 10) - 4.0,
                            0.25 + 0.05 * k, from.agent_id});
  }
  for (int k = 0; k < 60; ++k) {
    rays.push_back(cs_ray{-5.0, 16.0 + 0.45 * k, 1.0, 0.0, INFINITY, CS_NO_HIT});
    rays.push_back(cs_ray{17.0 + 0.4 * k, 66.0, 0.0, -2.0, 40.0, CS_NO_HIT});
    rays.push_back(cs_ray{64.0, 50.0 - 0.5 * k, -1.0, -0.25 + 0.01 * k, 80.0, CS_NO_HIT});
  }
  cs_selection box{};
  box.terms = CS_SEL_RECT;
  box.x0 = 24.0; box.y0 = 22.5; box.x1 = 37.25; box.y1 = 36.0;  // across both cuts of the mesh
  std::size_t rows = 0, hits = 0, at_zero = 0;
  for (const double radius : {0.2, 0.05, 0.6, 0.0}) {
    for (const cs_selection* targets : {(const cs_selection*)nullptr, (const cs_selection*)&box}) {
      const std::vector<cs_ray_hit> want = brute(one.agents, size, rays, radius, targets);
      rows += want.size();
      hits += hits_of(want);
      for (const cs_ray_hit& h : want) at_zero += h.id != CS_NO_HIT && h.t == 0.0;
      agree(one.cast_rays(rays, radius, targets), one.count_ray_hits(rays, radius, targets), want);
      agree(mesh.cast_rays(rays, radius, targets), mesh.count_ray_hits(rays, radius, targets), want);
    }
  }
  std::printf("rays: %zu rows compared, %zu hits, %zu of them at t == 0\n", rows, hits, at_zero);
  CHECK(rows == 8 * rays.size() && hits > 500 && hits < rows - 500);
  // what the Python side recomputes for this scene: the hits and the xor of the bits of every row
  const std::vector<cs_ray_hit> all = one.cast_rays(rays, 0.2);
  uint64_t x_ids = 0, x_t = 0;
  for (std::size_t k = 0; k < all.size(); ++k) {
    uint64_t t_bits;
    std::memcpy(&t_bits, &all[k].t, 8);
    x_ids ^= all[k].id * (uint64_t)(2 * k + 1);
    x_t ^= t_bits;
  }
  std::printf("rays: check 0.2 rays %zu hits %zu ids %016llx t %016llx\n", all.size(), hits_of(all),
              (unsigned long long)x_ids, (unsigned long long)x_t);
  // no rays at all
  CHECK(one.cast_rays(std::vector<cs_ray>{}, 0.2).empty() && mesh.count_ray_hits(std::vector<cs_ray>{}, 0.2) == 0);

  // a refused call throws and the next one is right, on the engine and on the mesh
  int threw = 0;
  std::vector<cs_ray> bad = rays;
  bad[7].ux = bad[7].uy = 0.0;
  try {
    one.cast_rays(bad, 0.2);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "cast_rays: ray 7") != nullptr;
  }
  try {
    mesh.cast_rays(rays, -1.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "cast_rays") != nullptr;
  }
  CHECK(threw == 2);
  steps(one, 5);
  steps(mesh, 5);
  const std::vector<cs_ray_hit> later = brute(one.agents, size, rays, 0.3, &box);
  agree(one.cast_rays(rays, 0.3, &box), one.count_ray_hits(rays, 0.3, &box), later);
  agree(mesh.cast_rays(rays, 0.3, &box), mesh.count_ray_hits(rays, 0.3, &box), later);
  std::printf("rays: passed\n");
  return 0;
}
