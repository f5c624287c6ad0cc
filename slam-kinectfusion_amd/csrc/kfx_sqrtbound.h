// The ICP lane's threshold tests `sqrtf(x) <= t` as one compare `x <= bound`
// (kfx_kernels.hip icp_lane; the bound is taken once per plan on the host).
// Checked over every non-negative float by tools/sqrt_bound_check.cpp, which
// includes this header (tests/test_sqrt_bound.py).
#pragma once
#include <cmath>
#include <limits>

#if defined(__HIPCC__)
#define KFX_HD __host__ __device__
#else
#define KFX_HD
#endif

namespace kfx {

// The largest float x with RN(sqrtf(x)) <= t (x >= 0), so that the ICP lane's
// `sqrtf(x) <= t` is the single compare `x <= bound` for every non-negative x
// (RN(sqrt) is monotonic; a NaN x fails both).  t < 0 admits nothing, t NaN
// nothing (the bound is NaN), t = +inf everything.
KFX_HD inline float sqrt_le_bound(float t) {
  if (std::isnan(t)) return t;
  if (t < 0.f) return -1.f;
  if (std::isinf(t)) return t;
  float x = t * t;
  if (std::isinf(x)) x = std::numeric_limits<float>::max();
  while (x > 0.f && std::sqrt(x) > t) x = std::nextafter(x, 0.f);
  for (;;) {
    const float n = std::nextafter(x, std::numeric_limits<float>::infinity());
    if (std::isinf(n) || std::sqrt(n) > t) break;
    x = n;
  }
  return x;
}

}  // namespace kfx
