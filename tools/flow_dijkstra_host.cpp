// The compiled host baseline of tools/flow_solve_bench.py: the rule of cs_flow_field_solve (include/crowdstep_state.h,
// "Solving a flow field on the device") as a plain std::priority_queue Dijkstra, host only, single thread.  Distances
// only: it is what a host would run instead of the device's rounds, and its f64 results are the device's, bit for bit.
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -o libflow_dijkstra_host.so tools/flow_dijkstra_host.cpp
#include <chrono>
#include <cmath>
#include <cstdint>
#include <functional>
#include <limits>
#include <queue>
#include <utility>
#include <vector>

// s: the slowness per bin as f64 (already slowness * (1 + weight * count)), or null for 1.  Returns seconds.
extern "C" double flow_dijkstra_host(uint32_t nx, uint32_t ny, double cell_w, double cell_h, const uint8_t* goals,
                                     const uint8_t* blocked, const double* s, double* dist) {
  const auto t0 = std::chrono::steady_clock::now();
  const double diag = std::sqrt(cell_w * cell_w + cell_h * cell_h);
  const double inf = std::numeric_limits<double>::infinity();
  const size_t bins = (size_t)nx * ny;
  using Item = std::pair<double, uint32_t>;
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
  for (size_t b = 0; b < bins; ++b) {
    dist[b] = inf;
    if (goals[b] && !(blocked && blocked[b])) {
      dist[b] = 0.0;
      heap.emplace(0.0, (uint32_t)b);
    }
  }
  auto wall = [&](int64_t x, int64_t y) { return blocked && blocked[(size_t)y * nx + (size_t)x]; };
  while (!heap.empty()) {
    const Item top = heap.top();
    heap.pop();
    if (top.first > dist[top.second]) continue;
    const int64_t iy = top.second / nx, ix = top.second - (uint32_t)iy * nx;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (!dx && !dy) continue;
        const int64_t jx = ix - dx, jy = iy - dy;  // the bin whose step (dx, dy) leads here
        if (jx < 0 || jy < 0 || jx >= (int64_t)nx || jy >= (int64_t)ny || wall(jx, jy)) continue;
        if (dx && dy && (wall(ix, jy) || wall(jx, iy))) continue;
        const size_t j = (size_t)jy * nx + (size_t)jx;
        const double len = dx && dy ? diag : dx ? cell_w : cell_h;
        const double c = top.first + len * (s ? s[j] : 1.0);
        if (c < dist[j]) {
          dist[j] = c;
          heap.emplace(c, (uint32_t)j);
        }
      }
  }
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
