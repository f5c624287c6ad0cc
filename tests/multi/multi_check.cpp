// multi_check — the host-only arithmetic of the multi-start ICP
// (csrc/kfx_multi.h) as a stand-alone program: the chunk rule against its
// definition over a grid of sizes and batch counts, and the float32 pose
// product against a product that rounds each step through a volatile float
// (one rounding per multiply and per add, left to right: what the device and
// the oracle do), on random rigid poses and on entries that expose a fused or
// reordered sum.  Prints "bad N chunk C poses P"; exit status 1 when N > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kfx_multi.h"

static long long chunk_def(int w, int h, long long n) {
  long long pb = ((long long)(w / 32) * 32 * ((h / 32) * 32) + 1023) / 1024;
  if (pb < 1) pb = 1;
  const long long want = (512 + pb - 1) / pb;
  long long c = n / want;
  if (c < 1) c = 1;
  if (c > 16) c = 16;
  return c;
}

static float rn_mul(float a, float b) {
  volatile float v = a * b;
  return v;
}
static float rn_add(float a, float b) {
  volatile float v = a + b;
  return v;
}
static void mul_ref(const float *aR, const float *at, const float *bR, const float *bt, float *oR, float *ot) {
  for (int j = 0; j < 3; ++j) {
    for (int i = 0; i < 3; ++i) {
      float v = 0.f;
      for (int k = 0; k < 3; ++k) v = rn_add(v, rn_mul(aR[3 * j + k], bR[3 * k + i]));
      oR[3 * j + i] = v;
    }
    float d = 0.f;
    for (int k = 0; k < 3; ++k) d = rn_add(d, rn_mul(aR[3 * j + k], bt[k]));
    ot[j] = rn_add(d, at[j]);
  }
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uni() {  // splitmix64, [0, 1)
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) / 9007199254740992.0;
}
static void rigid(float *R, float *t, double ang, double tr) {
  double a[3] = {uni() - 0.5, uni() - 0.5, uni() - 0.5};
  const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) + 1e-12;
  for (double &v : a) v /= n;
  const double th = ang * (2 * uni() - 1), s = std::sin(th), c = std::cos(th), c1 = 1 - c;
  const double m[9] = {c + c1 * a[0] * a[0],        c1 * a[0] * a[1] - s * a[2], c1 * a[0] * a[2] + s * a[1],
                       c1 * a[0] * a[1] + s * a[2], c + c1 * a[1] * a[1],        c1 * a[1] * a[2] - s * a[0],
                       c1 * a[0] * a[2] - s * a[1], c1 * a[1] * a[2] + s * a[0], c + c1 * a[2] * a[2]};
  for (int i = 0; i < 9; ++i) R[i] = (float)m[i];
  for (int i = 0; i < 3; ++i) t[i] = (float)(tr * (2 * uni() - 1));
}

int main(int argc, char **argv) {
  const int reps = argc > 1 ? std::atoi(argv[1]) : 20000;
  long long bad = 0, chunks = 0, poses = 0;
  const int sizes[][2] = {{1, 1},    {31, 31},   {32, 32},   {80, 48},    {80, 60},     {96, 32},    {160, 120},
                          {320, 240}, {640, 480}, {1280, 720}, {2048, 2048}, {8192, 8192}, {33, 4096}, {4096, 33}};
  std::vector<long long> ns = {1, 2, 3, 7, 8, 15, 16, 17, 20, 21, 127, 128, 129, 130, 255, 256, 257, 511, 512, 4095, 4096,
                               8191, 8192, 8193, 65535, 65536};
  for (const auto &s : sizes)
    for (long long n : ns) {
      const int c = kfx::icp_multi_chunk_rule(s[0], s[1], n);
      ++chunks;
      if (c != chunk_def(s[0], s[1], n) || c < 1 || c > 16 || c > (n > 1 ? n : 1)) {
        ++bad;
        std::printf("chunk %dx%d n %lld: %d\n", s[0], s[1], n, c);
      }
    }
  // the documented points: QVGA has 70 pixel blocks (320 x 224 covered), 80 x 48 has 2
  if (kfx::icp_multi_pixel_blocks(320, 240) != 70 || kfx::icp_multi_pixel_blocks(80, 48) != 2 ||
      kfx::icp_multi_pixel_blocks(16, 16) != 1 || kfx::icp_multi_chunk_rule(320, 240, 130) != 16 ||
      kfx::icp_multi_chunk_rule(320, 240, 21) != 2 || kfx::icp_multi_chunk_rule(80, 48, 130) != 1 ||
      kfx::icp_multi_chunk_rule(80, 48, 600) != 2)
    ++bad, std::printf("documented chunk points\n");
  for (int r = 0; r < reps; ++r) {
    float aR[9], at[3], bR[9], bt[3], oR[9], ot[3], wR[9], wt[3];
    rigid(aR, at, r % 3 ? 3.2 : 0.01, r % 2 ? 3.0 : 1e-3);
    rigid(bR, bt, r % 5 ? 0.05 : 3.2, r % 7 ? 0.02 : 5.0);
    if (r % 11 == 0)  // entries whose products cancel: a fused multiply-add would keep the low bits
      aR[0] = 1.f + 1.1920929e-7f, bR[0] = 1.f - 5.9604645e-8f, aR[1] = -1.f, bR[3] = 1.f;
    kfx::pose_mul_f32(aR, at, bR, bt, oR, ot);
    mul_ref(aR, at, bR, bt, wR, wt);
    ++poses;
    if (std::memcmp(oR, wR, sizeof(oR)) || std::memcmp(ot, wt, sizeof(ot))) {
      ++bad;
      if (bad < 10) std::printf("pose product %d differs\n", r);
    }
  }
  std::printf("bad %lld chunk %lld poses %lld\n", bad, chunks, poses);
  return bad ? 1 : 0;
}
