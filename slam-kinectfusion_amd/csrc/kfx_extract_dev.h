// kfx_extract_dev.h — the per-voxel device functions of the point extraction
// (FullScan6 and the vertex attributes), shared by kfx_extract.hip (the sweep
// kernels) and kfx_shift.hip (the eviction kernels) so both produce the same
// bytes.  Unnamed namespace, as kfx_device.h: each file gets its own copy.
#pragma once
#include "kfx_device.h"

namespace kfx {
namespace {

// ---- vertex attributes (kfx_extract_points_attr / kfx_extract_mesh_attr,
// definitions: include/kfx.h) --------------------------------------
// Gradient of F at voxel q = (x, y, z) (Fq = F(q)): per axis the difference of
// the two neighbours, one-sided (doubled) when only one is valid, 0 when none
// is.  Valid = inside the global volume and weight != 0.  A slab's owned items
// read slices z - 1 .. z + 2 only: inside its kSlabHalo stored halo.
__device__ __forceinline__ f3 tsdf_gradient(const VolView &v, int x, int y, int z, float Fq) {
  float g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int q = k == 0 ? x : (k == 1 ? y : z), dim = k == 0 ? v.X : (k == 1 ? v.Y : v.Z);
    float hi = Fq, lo = Fq;
    int valid = 0;
    if (q + 1 < dim) {
      const size_t j = vox_index(v, x + (k == 0), y + (k == 1), z + (k == 2));
      if (v.weight[j] != 0) {
        hi = (float)v.tsdf[j] * kDivShortMax;
        ++valid;
      }
    }
    if (q >= 1) {
      const size_t j = vox_index(v, x - (k == 0), y - (k == 1), z - (k == 2));
      if (v.weight[j] != 0) {
        lo = (float)v.tsdf[j] * kDivShortMax;
        ++valid;
      }
    }
    float d = hi - lo;
    if (valid == 1) d = d * 2.f;
    g[k] = d / v.vs[k];
  }
  return {g[0], g[1], g[2]};
}
// The 4 attribute words {nx, ny, nz, b | g<<8 | r<<16 | a<<24} of the vertex on
// the grid edge from voxel a = (x, y, z) to b = a + e_axis, written as integers
// (the colour word is never a float).  Called by emitting lanes only: the
// loads hit the bricks the wave has just read.
__device__ __forceinline__ void vertex_attr(const VolView &v, const DevPose &aff, int x, int y, int z, int axis,
                                            uint32_t *dst) {
  const int xb = x + (axis == 0), yb = y + (axis == 1), zb = z + (axis == 2);
  const size_t ia = vox_index(v, x, y, z), ib = vox_index(v, xb, yb, zb);
  const int qa = v.tsdf[ia], qb = v.tsdf[ib];
  const float Fa = (float)qa * kDivShortMax, Fb = (float)qb * kDivShortMax;
  const f3 ga = tsdf_gradient(v, x, y, z, Fa), gb = tsdf_gradient(v, xb, yb, zb, Fb);
  const float wa = fabsf(Fb), wb = fabsf(Fa);  // a's share is b's distance, as for the position
  const f3 m = {ga.x * wa + gb.x * wb, ga.y * wa + gb.y * wb, ga.z * wa + gb.z * wb};
  const f3 w = rmul(aff.R, m);
  const float l = sqrtf(w.x * w.x + w.y * w.y + w.z * w.z);
  f3 n = {0.f, 0.f, 0.f};
  if (l != 0.f) n = {w.x / l, w.y / l, w.z / l};
  const uint32_t ca = v.rgb[ia] & 0xffffffu, cb = v.rgb[ib] & 0xffffffu;
  uint32_t col = 0u;
  if (ca != 0u && cb != 0u) {
    const uint32_t ta = (uint32_t)abs(qa), tb = (uint32_t)abs(qb), den = ta + tb;  // den > 0: a crossing
#pragma unroll
    for (int j = 0; j < 3; ++j)
      col |= ((((ca >> (8 * j)) & 0xffu) * tb + ((cb >> (8 * j)) & 0xffu) * ta + (den >> 1)) / den) << (8 * j);
    col |= 0xff000000u;
  } else if ((ca | cb) != 0u) {
    col = (ca | cb) | 0xff000000u;
  }
  dst[0] = __float_as_uint(n.x);
  dst[1] = __float_as_uint(n.y);
  dst[2] = __float_as_uint(n.z);
  dst[3] = col;
}
// words per attributed vertex (kfx_vertex)
constexpr int kVertexWords = 7;
__device__ __forceinline__ void st_vertex(uint32_t *dst, f3 p) {
  dst[0] = __float_as_uint(p.x);
  dst[1] = __float_as_uint(p.y);
  dst[2] = __float_as_uint(p.z);
}

// Point-cloud extraction — FullScan6 (tsdf_volume.cu:307-481) of one voxel:
// the points of its +x, +y, +z edges (kfx_extract.hip has the definitions).
// axes (kAttr): the edge axis of point l in bits 2l, 2l + 1
template <bool kAttr = false>
__device__ __forceinline__ int extract_voxel(const VolView &v, const DevPose &aff, int x, int y,
                                             int z, f3 (&pts)[3], int *axes = nullptr) {
  const size_t i = vox_index(v, x, y, z);
  const int W = v.weight[i];
  const float F = (float)v.tsdf[i] * kDivShortMax;
  if (W == 0 || F == 1.f) return 0;
  const f3 V = {((float)x + 0.5f) * v.vs[0], ((float)y + 0.5f) * v.vs[1], ((float)z + 0.5f) * v.vs[2]};
  const f3 t = {aff.t[0], aff.t[1], aff.t[2]};
  int n = 0;
  auto edge = [&](int axis, size_t j) {
    const int Wn = v.weight[j];
    const float Fn = (float)v.tsdf[j] * kDivShortMax;
    if (Wn != 0 && Fn != 1.f && ((F > 0 && Fn < 0) || (F < 0 && Fn > 0))) {
      f3 p = V;
      const float Va = axis == 0 ? V.x : (axis == 1 ? V.y : V.z);
      const float Vn = Va + v.vs[axis];
      const float d_inv = 1.f / (fabsf(F) + fabsf(Fn));
      const float c = (Va * fabsf(Fn) + Vn * fabsf(F)) * d_inv;
      if (axis == 0) p.x = c;
      else if (axis == 1) p.y = c;
      else p.z = c;
      if constexpr (kAttr) *axes |= axis << (2 * n);
      pts[n++] = add(rmul(aff.R, p), t);
    }
  };
  if (x + 1 < v.X) edge(0, vox_index(v, x + 1, y, z));
  if (y + 1 < v.Y) edge(1, vox_index(v, x, y + 1, z));
  edge(2, vox_index(v, x, y, z + 1));  // z + 1 < Z: guaranteed by the z range
  return n;
}

}  // namespace
}  // namespace kfx
