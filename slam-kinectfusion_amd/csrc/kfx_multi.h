// kfx_multi.h — the host-only arithmetic of the multi-start ICP (DESIGN.md
// §27): the chunk rule and the float32 pose product the world poses are composed
// with.  Plain C++, no HIP: tests/multi/multi_check.cpp builds it alone.
#pragma once

namespace kfx {

constexpr int kIcpMultiBlockPix = 1024;    // pixels of the floor-covered region per block (k_icp_acc's)
constexpr int kIcpMultiMaxChunk = 16;      // poses one block walks at the most
constexpr int kIcpMultiFillBlocks = 512;   // the grid a batch aims for: two blocks on each of 256 CUs

// pixel blocks of a w x h level: the floor-covered region (A2: 32 x 32 tiles) in blocks of 1024, at least one
inline long long icp_multi_pixel_blocks(int w, int h) {
  const long long npix = (long long)((w / 32) * 32) * ((h / 32) * 32);
  const long long pb = (npix + kIcpMultiBlockPix - 1) / kIcpMultiBlockPix;
  return pb < 1 ? 1 : pb;
}

// Poses per block of a batch of n >= 1: the most, up to 16, that still leave a
// grid of 512 blocks (pixel blocks x chunks), at least 1.  A block keeps its
// 1024 pixels' current-frame vertices and normals in registers over its chunk,
// so a longer chunk saves their loads (24 bytes per pixel and pose) but leaves
// fewer blocks; below 512 blocks CUs idle, which costs more than the loads.
inline int icp_multi_chunk_rule(int w, int h, long long n) {
  const long long pb = icp_multi_pixel_blocks(w, h);
  const long long want = (kIcpMultiFillBlocks + pb - 1) / pb;  // chunks that fill the grid
  const long long c = n / want;
  return (int)(c < 1 ? 1 : (c > kIcpMultiMaxChunk ? kIcpMultiMaxChunk : c));
}

// Affine3f product o = a * b in the float order of the device's pose_mul (the
// oracle's kfo_pose_mul): every entry a sum of three products added left to
// right from 0, the translation's sum then added to a's.  R: 9 floats row-major,
// t: 3.  Built without contraction, the sums round as the device's.
inline void pose_mul_f32(const float *aR, const float *at, const float *bR, const float *bt, float *oR, float *ot) {
  for (int j = 0; j < 3; ++j) {
    for (int i = 0; i < 3; ++i) {
      float v = 0.f;
      for (int k = 0; k < 3; ++k) v += aR[3 * j + k] * bR[3 * k + i];
      oR[3 * j + i] = v;
    }
    float d = 0.f;
    for (int k = 0; k < 3; ++k) d += aR[3 * j + k] * bt[k];
    ot[j] = d + at[j];
  }
}

}  // namespace kfx
