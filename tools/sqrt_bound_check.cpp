// Exhaustive check of sqrt_le_bound (csrc/kfx_sqrtbound.h, the function the ICP
// plan calls): for every non-negative float x, (sqrtf(x) <= t) == (x <= bound(t)).
// build: g++ -O2 -ffp-contract=off tools/sqrt_bound_check.cpp -o /tmp/sqrt_bound_check
// usage: sqrt_bound_check [stride]   (every stride-th float, default 1, and always the 64 floats on either
// side of each bound; exit status 1 on a mismatch)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <cstdlib>
#include <limits>

#include "../slam-kinectfusion_amd/csrc/kfx_sqrtbound.h"
using kfx::sqrt_le_bound;
int main(int argc, char **argv) {
  const uint64_t stride = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
  if (stride == 0) return 2;
  long total = 0;
  float ts[] = {0.015f, std::sin(30.f * 0.017453293f), 0.f, 1e-30f, 3.f, 1e30f, 0.1f, 0.5f};
  for (float t : ts) {
    float b = sqrt_le_bound(t);
    long bad = 0;
    for (uint64_t u = 0; u < 0x80000000ull; u += stride) {  // every non-negative float incl. inf/NaN
      uint32_t w = (uint32_t)u; float x; memcpy(&x, &w, 4);
      if ((std::sqrt(x) <= t) != (x <= b)) ++bad;
    }
    // whatever the stride, the 64 floats on either side of the bound: the only place the two forms can part
    uint32_t wb; memcpy(&wb, &b, 4);
    for (int64_t u = (int64_t)wb - 64; b >= 0.f && u <= (int64_t)wb + 64; ++u) {
      if (u < 0 || u >= 0x80000000ll) continue;
      uint32_t w = (uint32_t)u; float x; memcpy(&x, &w, 4);
      if ((std::sqrt(x) <= t) != (x <= b)) ++bad;
    }
    printf("t=%g bound=%a mismatches=%ld\n", t, b, bad);
    total += bad;
  }
  return total ? 1 : 0;
}
