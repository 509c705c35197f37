// tools/exp2_underflow.hip -- where v_exp_f32 (fast_exp2, __builtin_amdgcn_exp2f) starts to return +0, in the denormal
// mode the engine is built with (no -ffast-math: f32 denormals on).  The force pass of the tiled step kernel skips terms
// whose exp2 argument is at or below -ZAN_EXP2_ZERO (cs_device_types.hip.inc); this checks that bound on the chip.
// Every f32 from -64 down to -inf is evaluated once; prints one JSON line:
//   last_nonzero_input   the most negative input whose result is not +0
//   first_zero_input     the least negative input whose result is +0
//   smallest_nonzero     the smallest positive result seen (< 2^-126 would mean denormal results)
//   bad_below            inputs at or below -ZAN_EXP2_ZERO (160) whose result is not +0 (must be 0)
//   build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -o tools/exp2_underflow tools/exp2_underflow.hip
//   run:   tools/exp2_underflow
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr uint32_t LO = 0xC2800000u;  // -64.0f
constexpr uint32_t HI = 0xFF800000u;  // -inf (larger bit patterns of negative floats are more negative)
constexpr uint32_t BOUND = 0xC3200000u;  // -160.0f

// out[0]: max input bits with a result != +0; out[1]: min input bits with result +0; out[2]: min non-zero result bits;
// out[3]: count of inputs at or below -160 with a result != +0
__global__ void sweep(uint32_t* out) {
  const uint32_t stride = gridDim.x * blockDim.x;
  uint32_t last_nz = 0u, first_z = 0xFFFFFFFFu, small = 0xFFFFFFFFu, bad = 0u;
  for (uint64_t b = (uint64_t)LO + blockIdx.x * blockDim.x + threadIdx.x; b <= HI; b += stride) {
    const uint32_t xb = (uint32_t)b;
    float x;
    memcpy(&x, &xb, 4);
    const float r = __builtin_amdgcn_exp2f(x);
    uint32_t rb;
    memcpy(&rb, &r, 4);
    if (rb != 0u) {
      last_nz = xb > last_nz ? xb : last_nz;
      small = rb < small ? rb : small;
      if (xb >= BOUND) ++bad;
    } else {
      first_z = xb < first_z ? xb : first_z;
    }
  }
  atomicMax(&out[0], last_nz);
  atomicMin(&out[1], first_z);
  atomicMin(&out[2], small);
  atomicAdd(&out[3], bad);
}

static float as_f(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}

int main() {
  uint32_t* d;
  CHECK(hipMalloc(&d, 4 * sizeof(uint32_t)));
  const uint32_t init[4] = {0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u};
  CHECK(hipMemcpy(d, init, sizeof(init), hipMemcpyHostToDevice));
  sweep<<<4096, 256>>>(d);
  CHECK(hipGetLastError());
  uint32_t h[4];
  CHECK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
  CHECK(hipFree(d));
  printf("{\"last_nonzero_input\": %.9g, \"first_zero_input\": %.9g, \"smallest_nonzero\": %.9g, \"bad_below\": %u}\n",
         as_f(h[0]), as_f(h[1]), as_f(h[2]), h[3]);
  return 0;
}
