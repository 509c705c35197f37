// Encounters from C++ (include/crowdsim.hpp over include/crowdstep_state.h): encounters and count_encounters on one engine
// and on a 2 x 2 mesh against a brute-force double loop over `agents` by the rule the header writes: the same rows, byte
// for byte, with and without roles and a limit, and a refused call throws.  It prints the count and a checksum of the
// bits of one query, which tests/test_gpu_encounters_cpp.py (it builds and launches this on an MI355X) compares with what
// the Python side computes for the same scene.
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

// the rule of the header on `agents` (volatile: every operation rounded once); rects: the roles (null: everyone)
template <class Map>
static std::vector<cs_encounter> brute(const Map& agents, double size, double distance, double horizon, double range,
                                       const cs_selection* sel_a, const cs_selection* sel_b, uint64_t* in_range) {
  std::vector<const Agent*> part;
  for (const auto& kv : agents) {
    const Point p = kv.second.position;
    if (0.0 <= p.x && p.x < size && 0.0 <= p.y && p.y < size) part.push_back(&kv.second);
  }
  std::sort(part.begin(), part.end(), [](const Agent* l, const Agent* r) { return l->agent_id < r->agent_id; });
  volatile double range2 = range * range, lim2 = distance * distance;
  std::vector<cs_encounter> out;
  *in_range = 0;
  for (std::size_t i = 0; i < part.size(); ++i) {
    for (std::size_t j = i + 1; j < part.size(); ++j) {
      const Agent &p = *part[i], &q = *part[j];
      const bool ap = in_rect(sel_a, p.position), bp = in_rect(sel_b, p.position);
      const bool aq = in_rect(sel_a, q.position), bq = in_rect(sel_b, q.position);
      if (!((ap && bq) || (aq && bp))) continue;
      volatile double rx = q.position.x - p.position.x, ry = q.position.y - p.position.y;
      volatile double wx = (double)(float)q.velocity.x - (double)(float)p.velocity.x;
      volatile double wy = (double)(float)q.velocity.y - (double)(float)p.velocity.y;
      volatile double rxx = rx * rx, ryy = ry * ry;
      volatile double d2 = rxx + ryy;
      if (!(d2 < range2)) continue;
      ++*in_range;
      volatile double wxx = wx * wx, wyy = wy * wy, rwx = rx * wx, rwy = ry * wy;
      volatile double ww = wxx + wyy, rw = rwx + rwy;
      volatile double t = 0.0;
      if (rw < 0.0) {
        volatile double minus = -rw;
        t = minus / ww;
        if (!(t < horizon)) t = horizon;
      }
      volatile double wxt = wx * t, wyt = wy * t;
      volatile double cx = rx + wxt, cy = ry + wyt;
      volatile double cxx = cx * cx, cyy = cy * cy;
      volatile double m2 = cxx + cyy;
      if (!(m2 < lim2)) continue;
      cs_encounter row{};
      row.a = p.agent_id;
      row.b = q.agent_id;
      row.t = t;
      row.d2 = m2;
      out.push_back(row);
    }
  }
  return out;
}

static void agree(const std::vector<cs_encounter>& got, uint64_t count, const std::vector<cs_encounter>& want) {
  CHECK(count == want.size());
  CHECK(got.size() == want.size());
  CHECK(got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(cs_encounter)) == 0);
}

int main() {
  static_assert(sizeof(cs_encounter) == 32, "four 8-byte words");
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

  cs_selection box{}, strip{};
  box.terms = CS_SEL_RECT;
  box.x0 = 24.0; box.y0 = 22.5; box.x1 = 37.25; box.y1 = 36.0;  // across both cuts of the mesh (30 m)
  strip.terms = CS_SEL_RECT;
  strip.x0 = 0.0; strip.y0 = 28.0; strip.x1 = 60.0; strip.y1 = 33.0;  // along one cut
  std::size_t rows = 0, still = 0, free = 0, clamped = 0;
  uint64_t near = 0;
  const double numbers[][3] = {{0.8, 2.0, 2.0}, {1.0, 1.0, 2.0}, {1.5, 1.0, 2.0}, {1.5, 0.0, 2.0}, {0.0, 1.0, 2.0},
                               {INFINITY, INFINITY, 1.5}, {0.6, 1.0, 0.0}};  // (range 2.0: the most one halo cell of 2 m allows)
  for (const auto& q : numbers) {
    for (const cs_selection* a : {(const cs_selection*)nullptr, (const cs_selection*)&box}) {
      for (const cs_selection* b : {(const cs_selection*)nullptr, (const cs_selection*)&strip}) {
        uint64_t in_range = 0;
        const std::vector<cs_encounter> want = brute(one.agents, size, q[0], q[1], q[2], a, b, &in_range);
        rows += want.size();
        near += in_range;
        for (const cs_encounter& r : want) {
          still += r.t == 0.0;
          free += 0.0 < r.t && r.t < q[1];
          clamped += r.t == q[1] && q[1] > 0.0;
        }
        agree(one.encounters(q[0], q[1], q[2], a, b), one.count_encounters(q[0], q[1], q[2], a, b), want);
        agree(mesh.encounters(q[0], q[1], q[2], a, b), mesh.count_encounters(q[0], q[1], q[2], a, b), want);
      }
    }
  }
  std::printf("encounters: %zu rows compared of %llu pairs in range; t == 0: %zu, 0 < t < horizon: %zu, t == horizon: %zu\n",
              rows, (unsigned long long)near, still, free, clamped);
  CHECK(rows > 500 && rows < near && still > 5 && free > 5 && clamped > 5);
  // a limit: the first rows
  uint64_t in_range = 0;
  const std::vector<cs_encounter> all = brute(one.agents, size, 0.8, 2.0, 2.0, nullptr, nullptr, &in_range);
  CHECK(all.size() > 7);
  const std::vector<cs_encounter> few = one.encounters(0.8, 2.0, 2.0, nullptr, nullptr, 7);
  CHECK(few.size() == 7 && std::memcmp(few.data(), all.data(), 7 * sizeof(cs_encounter)) == 0);
  const std::vector<cs_encounter> few_m = mesh.encounters(0.8, 2.0, 2.0, nullptr, nullptr, 7);
  CHECK(few_m.size() == 7 && std::memcmp(few_m.data(), all.data(), 7 * sizeof(cs_encounter)) == 0);
  // what the Python side recomputes for this scene: the count and the xor of the bits of every row
  uint64_t x_ids = 0, x_t = 0, x_d2 = 0;
  for (const cs_encounter& r : one.encounters(0.8, 2.0, 2.0)) {
    uint64_t t_bits, d2_bits;
    std::memcpy(&t_bits, &r.t, 8);
    std::memcpy(&d2_bits, &r.d2, 8);
    x_ids ^= (r.a << 20) ^ r.b;
    x_t ^= t_bits;
    x_d2 ^= d2_bits;
  }
  std::printf("encounters: check 0.8 2.0 2.0 count %zu ids %016llx t %016llx d2 %016llx\n", all.size(),
              (unsigned long long)x_ids, (unsigned long long)x_t, (unsigned long long)x_d2);
  // +inf everywhere on one engine: every pair with a finite m2
  CHECK(one.count_encounters(INFINITY, INFINITY, INFINITY) == 400u * 399u / 2u);

  // a refused call throws and the next one is right, on the engine and on the mesh
  int threw = 0;
  try {
    one.encounters(0.5, -1.0, 2.0);
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "encounters") != nullptr;
  }
  try {
    mesh.encounters(0.5, 1.0, 2.5);  // above halo_cells * cell_size
  } catch (const std::runtime_error& e) {
    threw += std::strstr(e.what(), "halo_cells") != nullptr;
  }
  CHECK(threw == 2);
  steps(one, 5);
  steps(mesh, 5);
  const std::vector<cs_encounter> later = brute(one.agents, size, 1.0, 1.5, 2.0, nullptr, &box, &in_range);
  agree(one.encounters(1.0, 1.5, 2.0, nullptr, &box), one.count_encounters(1.0, 1.5, 2.0, nullptr, &box), later);
  agree(mesh.encounters(1.0, 1.5, 2.0, nullptr, &box), mesh.count_encounters(1.0, 1.5, 2.0, nullptr, &box), later);
  std::printf("encounters: passed\n");
  return 0;
}
