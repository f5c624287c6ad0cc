// kfx_device.h — device code that two or more of the kernel files
// (kfx_kernels.hip, kfx_extract.hip, kfx_volume_io.hip, kfx_view.hip,
// kfx_shift.hip, kfx_quality.hip) use (the raycast march's functions: kfx_ray.h; the
// extraction's per-voxel functions: kfx_extract_dev.h).  Everything lives
// in an unnamed namespace: each file gets its own internal copy.  A helper with
// one user lives in that file instead.
#pragma once
#include "kfx_internal.h"

namespace kfx {
namespace {

constexpr float kDivShortMax = 0.0000305185f;  // device_utils.cuh:6

struct f3 {
  float x, y, z;
};
__device__ __forceinline__ f3 add(f3 a, f3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ f3 sub(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ f3 scl(f3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ f3 mulc(f3 a, f3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ f3 cross(f3 a, f3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ f3 normalized(f3 v) {
  const float t = sqrtf(dot(v, v));
  return {v.x / t, v.y / t, v.z / t};
}
__device__ __forceinline__ f3 rmul(const float *R, f3 v) {
  return {R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z,
          R[6] * v.x + R[7] * v.y + R[8] * v.z};
}
__device__ __forceinline__ f3 ld3(const float *p, size_t i) {
  return {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
}
__device__ __forceinline__ void st3(float *p, size_t i, f3 v) {
  p[3 * i] = v.x;
  p[3 * i + 1] = v.y;
  p[3 * i + 2] = v.z;
}

// The uchar conversion and __m_normalize of the shaders (k_render, k_view):
// IEEE sqrt and division, NaN -> 0, as the oracle's kfo_render.
__device__ __forceinline__ uint8_t render_u8(float x) { return x >= 1.f ? (uint8_t)fminf(x, 255.f) : 0; }
__device__ __forceinline__ f3 normalized_ieee(f3 v) {
  const float t = sqrtf(dot(v, v));
  return {v.x / t, v.y / t, v.z / t};
}

// z is the global slice; the view stores slices [zb, zb+zn) (tile-column
// layout, kfx_internal.h VolView)
__device__ __forceinline__ size_t vox_index(const VolView &v, int x, int y, int z) {
  return (((size_t)(y >> 3) * v.tiles_x + (x >> 3)) * (size_t)v.zn + (size_t)(z - v.zb)) * 64 +
         ((y & 7) << 3) + (x & 7);
}

// Occupancy marking (VolView::bocc / socc): some voxel of column tile (tx, ty)
// in global slices [zlo, zhi] holds a negative tsdf.  Sets, dilated by one,
// the bricks (zlo>>3)-1 .. (zhi>>3)+1 of the 3x3 tiles around (tx, ty) (lanes
// 0..8 of the calling wave) and the super-bricks (zlo>>5)-1 .. (zhi>>5)+1 of
// the 3x3 super tiles around (tx>>2, ty>>2) (lanes 9..17).  A plain read
// first skips the atomic when the bits are already set (bits are never
// cleared inside a launch, so a stale read is a subset).
template <typename W>
__device__ __forceinline__ void occ_set_bits(W *base, int lo, int hi) {
  constexpr int kb = 8 * sizeof(W);
  for (int b = lo; b <= hi;) {
    const int wi = b / kb, e = min(hi, wi * kb + kb - 1);
    const W m = (e - b == kb - 1 ? ~(W)0 : (((W)1 << (e - b + 1)) - (W)1)) << (b % kb);
    if ((base[wi] & m) != m) atomicOr(&base[wi], m);
    b = e + 1;
  }
}
__device__ void occ_mark(const VolView &v, int tx, int ty, int zlo, int zhi, int lane) {
  if (lane < 9) {
    const int x = tx + lane % 3 - 1, y = ty + lane / 3 - 1;
    if (x < 0 || y < 0 || x >= v.tiles_x || y >= v.tiles_y) return;
    occ_set_bits(v.bocc + (size_t)(y * v.tiles_x + x) * v.bw, max((zlo >> 3) - 1 - v.bz0, 0),
                 min((zhi >> 3) + 1 - v.bz0, v.nbz - 1));
  } else if (lane < 18) {
    const int k = lane - 9;
    const int x = (tx >> 2) + k % 3 - 1, y = (ty >> 2) + k / 3 - 1;
    if (x < 0 || y < 0 || x >= v.stx || y >= v.sty) return;
    occ_set_bits(v.socc + (size_t)(y * v.stx + x) * v.sw, max((zlo >> 5) - 1 - v.sz0, 0),
                 min((zhi >> 5) + 1 - v.sz0, v.nsz - 1));
  }
}
// Wave-wide [min lo, max hi] then occ_mark (all 64 lanes active).
__device__ __forceinline__ void occ_mark_wave(const VolView &v, int tile, int lo, int hi, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = min(lo, __shfl_xor(lo, off));
    hi = max(hi, __shfl_xor(hi, off));
  }
  if (hi >= lo) occ_mark(v, tile % v.tiles_x, tile / v.tiles_x, lo, hi, lane);
}

}  // namespace
}  // namespace kfx
