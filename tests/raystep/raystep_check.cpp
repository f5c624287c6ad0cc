// Brute-force check of kfx::ray_sample_end (csrc/kfx_raystep.h) against the plain march loop
//   for (x = L0; x < tfar; x = x + step)
// whose trip count it returns, and of kfx::ff_add as the loop's value at an index (the raycast
// takes a hit's ray_len from it).  argv: seed cases.  Prints "bad <count>".
#include "kfx_raystep.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

namespace {

constexpr int kMaxRun = 4200;  // the generators keep runs within ~4100 samples
float seq[kMaxRun + 1];

float ulps(float x, int n) {  // x moved by n units in the last place
  uint32_t b;
  std::memcpy(&b, &x, 4);
  b = (uint32_t)((int32_t)b + n);
  std::memcpy(&x, &b, 4);
  return x;
}

bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0 || (std::isnan(a) && std::isnan(b)); }

}  // namespace

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 7u;
  const long cases = argc > 2 ? std::atol(argv[2]) : 100000;
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  // the configurations' march steps, vs[0] = range / dims as kfx_api.hip computes it
  // (C2 512^3 and C3/C4 1024^3 over 2.048 m, C5 2048^3 over 4.096 m, C1 128^3, the 64^3 tests)
  const float steps[5] = {2.048f / 512.f, 2.048f / 1024.f, 4.096f / 2048.f, 2.048f / 128.f, 2.048f / 64.f};
  const float edges[5] = {0.25f, 0.5f, 1.f, 2.f, 4.f};
  long bad = 0, skipped = 0;
  for (long it = 0; it < cases; ++it) {
    float step = steps[g() % 5], L0, tfar;
    // a run of at most `room` samples and tfar <= 8 m (the longest ray of C5 is 4.096 * sqrt(3) m)
    auto far = [&](int room) { return std::fmin(8.f, L0 + U(g) * (float)room * step); };
    switch (it % 12) {
      case 0: case 1:  // camera outside: L0 = tnear + step
        L0 = U(g) * 3.f + step;
        tfar = far(g() % 4 == 0 ? 4096 : 600);
        break;
      case 2:  // camera inside: L0 = 0 + step
        L0 = 0.f + step;
        tfar = far(g() % 4 == 0 ? 4096 : 600);
        break;
      case 3:  // L0 within +-8 ulp of a binade edge
        L0 = ulps(edges[g() % 5], (int)(g() % 17) - 8);
        tfar = far(g() % 4 == 0 ? 4096 : 300);
        break;
      case 4:  // tfar within +-4 steps of L0 on both sides, and tfar <= L0
        L0 = U(g) * 6.f + step;
        tfar = g() % 8 == 0 ? L0 : L0 + (U(g) * 8.f - 4.f) * step;
        break;
      case 5: case 6: {  // tfar exactly on a sequence value, or 1 ulp beside it
        L0 = g() % 2 ? U(g) * 4.f + step : ulps(edges[g() % 5], (int)(g() % 17) - 8);
        const int k = (int)(g() % (g() % 4 == 0 ? 4096 : 400));
        float x = L0;
        for (int i = 0; i < k && x < 8.f; ++i) x = x + step;
        tfar = it % 12 == 5 ? x : ulps(x, g() % 2 ? 1 : -1);
        break;
      }
      case 7:  // non-finite tfar or L0
        L0 = g() % 8 == 0 ? NAN : U(g) * 4.f;
        tfar = g() % 2 ? NAN : INFINITY;
        break;
      case 8:  // the longest runs: C5's step from near the camera to 8 m
        step = steps[2];
        L0 = U(g) * 0.5f + step;
        tfar = std::fmin(8.f, L0 + (3000.f + U(g) * 1096.f) * step);
        break;
      case 9:  // other steps
        step = 0.001f + U(g) * 0.03f;
        L0 = U(g) * 6.f + (g() % 2 ? step : 0.f);
        tfar = far(g() % 4 == 0 ? 4096 : 500);
        break;
      case 10: {  // steps with trailing-zero mantissas: ties
        uint32_t b;
        step = 0.001f + U(g) * 0.03f;
        std::memcpy(&b, &step, 4);
        b &= ~((1u << (g() % 21)) - 1u);
        std::memcpy(&step, &b, 4);
        L0 = U(g) * 4.f;
        tfar = far(500);
        break;
      }
      default:  // negative start (not a ray's, but the loop is the same), crossing zero
        L0 = -U(g) * 0.5f;
        tfar = L0 + U(g) * 300.f * step;
        break;
    }
    const int got = kfx::ray_sample_end(L0, step, tfar);
    if (std::isinf(tfar) && !std::isnan(L0)) {  // the plain loop never ends: the documented cap
      if (got != kfx::kRaySampleCap) {
        if (bad < 10) std::printf("L0=%a step=%a tfar=inf got %d\n", L0, step, got);
        ++bad;
      }
      continue;
    }
    int end = 0;
    float x = L0;
    for (; x < tfar && end < kMaxRun; x = x + step) seq[end++] = x;
    seq[end] = x;
    if (end >= kMaxRun) {  // (no generator reaches this)
      ++skipped;
      continue;
    }
    if (got != end) {
      if (bad < 10) std::printf("L0=%a step=%a tfar=%a loop %d ray_sample_end %d\n", L0, step, tfar, end, got);
      ++bad;
    }
    const int ks[3] = {0, end > 0 ? end - 1 : 0, end > 0 ? (int)(g() % (unsigned)end) : 0};
    for (int k : ks) {
      const float v = kfx::ff_add(L0, step, k), w = kfx::ff_add_fast(L0, step, k);
      if (!same(v, seq[k]) || !same(w, seq[k])) {
        if (bad < 10) std::printf("L0=%a step=%a k=%d loop %a ff_add %a ff_add_fast %a\n", L0, step, k, seq[k], v, w);
        ++bad;
      }
    }
  }
  if (skipped * 100 > cases) {
    std::printf("skipped %ld of %ld cases\n", skipped, cases);
    return 2;
  }
  std::printf("bad %ld\n", bad);
  return bad != 0;
}
