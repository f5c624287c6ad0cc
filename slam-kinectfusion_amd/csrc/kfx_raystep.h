// Exact trip count of the raycast's march loop (raycast's sample-index bound).
//
// The reference marches a ray by  for (; ray_len < tfar; ray_len += step)
// (tsdf_volume.cu:210-260): ray_len at iteration k is k float adds of one
// constant to one start value, ff_add(L0, step, k) (kfx_ffadd.h), so where the
// loop ends is a function of the iteration index alone.  ray_sample_end gives
// that index once per ray; the march then compares integers instead of
// carrying ray_len through every sample, and a hit's exact ray_len is one
// ff_add from L0.  The sequence never decreases (step > 0, round to nearest),
// so from any k with ff_add(L0, step, k) < tfar plain adds reach the answer
// exactly, whatever estimate chose that k.  Checked against the plain loop on
// millions of cases (tests/test_raystep.py).  Host and device share this code.
#pragma once
#include "kfx_ffadd.h"

namespace kfx {

// ray_sample_end saturates here: the loop would run at least this long (tfar
// = +inf, a step that is not positive or that no longer moves ray_len)
constexpr int kRaySampleCap = 1 << 30;

// Iterations of  for (x = L0; x < tfar; x = x + step): the smallest k >= 0
// with ff_add(L0, step, k) >= tfar; 0 when !(L0 < tfar) (NaN on either side
// included).
KFX_HD inline int ray_sample_end(float L0, float step, float tfar) {
  if (!(L0 < tfar)) return 0;
  if (!(step > 0.f)) return kRaySampleCap;  // x never grows (or turns NaN): no end
  // continuous estimate, then a few steps below it (the accumulated rounding
  // of a few thousand adds stays below one step for the volumes in use)
  const float est = (tfar - L0) / step;
  int k = est < (float)kRaySampleCap ? (int)est : kRaySampleCap;
  float x;
  for (int back = 4;;) {  // (one ff_add call site: the estimate too far backs off and retries)
    k = k > back ? k - back : 0;
    x = ff_add(L0, step, k);
    if (k == 0 || x < tfar) break;
    if (back < (1 << 28)) back *= 2;
  }
  while (x < tfar && k < kRaySampleCap) {
    const float xn = x + step;
    if (xn == x) return kRaySampleCap;  // fixed point below tfar
    x = xn;
    ++k;
  }
  return k;
}

}  // namespace kfx
