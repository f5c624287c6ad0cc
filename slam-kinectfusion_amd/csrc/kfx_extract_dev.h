// kfx_extract_dev.h — the per-voxel device functions of the point extraction
// (FullScan6 and the vertex attributes) and the brick sweeps of one wave,
// shared by kfx_extract.hip (the sweep kernels), kfx_shift.hip (the eviction
// kernels) and kfx_world.hip (the world map) so all produce the same bytes.
// Unnamed namespace, as kfx_device.h: each file gets its own copy.
#pragma once
#include "kfx_device.h"

namespace kfx {
namespace {

// ---- views --------------------------------------------------------------------
// The per-voxel functions below are templates over a view of the voxels: the
// dense volume (VolView, global memory) here, a world brick's staged tile in
// kfx_world.hip (WorldTile, LDS).  A view has vs[3] and these accessors:
//   vw_index(v, x, y, z)   the voxel's handle for the three loads below
//   vw_weight / vw_tsdf / vw_rgb(v, i)   the stored values (raw)
//   vw_above(v, k, q) / vw_below(v, k, q)   index q + 1 / q - 1 of axis k exists
//   vw_coord(v, k, q)      (float) of the index the position is computed from
__device__ __forceinline__ size_t vw_index(const VolView &v, int x, int y, int z) { return vox_index(v, x, y, z); }
__device__ __forceinline__ int vw_weight(const VolView &v, size_t i) { return v.weight[i]; }
__device__ __forceinline__ int vw_tsdf(const VolView &v, size_t i) { return v.tsdf[i]; }
__device__ __forceinline__ uint32_t vw_rgb(const VolView &v, size_t i) { return v.rgb[i]; }
__device__ __forceinline__ bool vw_above(const VolView &v, int k, int q) {
  return q + 1 < (k == 0 ? v.X : (k == 1 ? v.Y : v.Z));
}
__device__ __forceinline__ bool vw_below(const VolView &, int, int q) { return q >= 1; }
__device__ __forceinline__ float vw_coord(const VolView &, int, int q) { return (float)q; }

// ---- vertex attributes (kfx_extract_points_attr / kfx_extract_mesh_attr,
// definitions: include/kfx.h) --------------------------------------
// Gradient of F at voxel q = (x, y, z) (Fq = F(q)): per axis the difference of
// the two neighbours, one-sided (doubled) when only one is valid, 0 when none
// is.  Valid = inside the global volume and weight != 0.  A slab's owned items
// read slices z - 1 .. z + 2 only: inside its kSlabHalo stored halo.
template <typename View>
__device__ __forceinline__ f3 tsdf_gradient(const View &v, int x, int y, int z, float Fq) {
  float g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int q = k == 0 ? x : (k == 1 ? y : z);
    float hi = Fq, lo = Fq;
    int valid = 0;
    if (vw_above(v, k, q)) {
      const auto j = vw_index(v, x + (k == 0), y + (k == 1), z + (k == 2));
      if (vw_weight(v, j) != 0) {
        hi = (float)vw_tsdf(v, j) * kDivShortMax;
        ++valid;
      }
    }
    if (vw_below(v, k, q)) {
      const auto j = vw_index(v, x - (k == 0), y - (k == 1), z - (k == 2));
      if (vw_weight(v, j) != 0) {
        lo = (float)vw_tsdf(v, j) * kDivShortMax;
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
template <typename View>
__device__ __forceinline__ void vertex_attr(const View &v, const DevPose &aff, int x, int y, int z, int axis,
                                            uint32_t *dst) {
  const int xb = x + (axis == 0), yb = y + (axis == 1), zb = z + (axis == 2);
  const auto ia = vw_index(v, x, y, z), ib = vw_index(v, xb, yb, zb);
  const int qa = vw_tsdf(v, ia), qb = vw_tsdf(v, ib);
  const float Fa = (float)qa * kDivShortMax, Fb = (float)qb * kDivShortMax;
  const f3 ga = tsdf_gradient(v, x, y, z, Fa), gb = tsdf_gradient(v, xb, yb, zb, Fb);
  const float wa = fabsf(Fb), wb = fabsf(Fa);  // a's share is b's distance, as for the position
  const f3 m = {ga.x * wa + gb.x * wb, ga.y * wa + gb.y * wb, ga.z * wa + gb.z * wb};
  const f3 w = rmul(aff.R, m);
  const float l = sqrtf(w.x * w.x + w.y * w.y + w.z * w.z);
  f3 n = {0.f, 0.f, 0.f};
  if (l != 0.f) n = {w.x / l, w.y / l, w.z / l};
  const uint32_t ca = vw_rgb(v, ia) & 0xffffffu, cb = vw_rgb(v, ib) & 0xffffffu;
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
template <bool kAttr = false, typename View>
__device__ __forceinline__ int extract_voxel(const View &v, const DevPose &aff, int x, int y,
                                             int z, f3 (&pts)[3], int *axes = nullptr) {
  const auto i = vw_index(v, x, y, z);
  const int W = vw_weight(v, i);
  const float F = (float)vw_tsdf(v, i) * kDivShortMax;
  if (W == 0 || F == 1.f) return 0;
  const f3 V = {(vw_coord(v, 0, x) + 0.5f) * v.vs[0], (vw_coord(v, 1, y) + 0.5f) * v.vs[1],
                (vw_coord(v, 2, z) + 0.5f) * v.vs[2]};
  const f3 t = {aff.t[0], aff.t[1], aff.t[2]};
  int n = 0;
  auto edge = [&](int axis, decltype(i) j) {
    const int Wn = vw_weight(v, j);
    const float Fn = (float)vw_tsdf(v, j) * kDivShortMax;
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
  if (vw_above(v, 0, x)) edge(0, vw_index(v, x + 1, y, z));
  if (vw_above(v, 1, y)) edge(1, vw_index(v, x, y + 1, z));
  edge(2, vw_index(v, x, y, z + 1));  // z + 1 exists: guaranteed by the z range
  return n;
}

// One extraction wave's brick (lanes = the tile's 64 columns, slices [z0, z1)):
// kEmit = false returns the wave's point count; true writes the points at
// base + (canonical rank) (rank < cap only) and returns the count too.
// kAttr (emit only): 7-word attributed points (kfx_vertex) instead of float3.
template <bool kEmit, bool kAttr = false, typename View>
__device__ __forceinline__ unsigned extract_wave(const View &v, const DevPose &aff, int x, int y, int z0,
                                                 int z1, unsigned long long base, float *out,
                                                 unsigned long long cap) {
  const int lane = threadIdx.x & 63;
  unsigned total = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int z = z0; z < z1; ++z) {
    f3 pts[3];
    int axes = 0;
    const int n = extract_voxel<kEmit && kAttr>(v, aff, x, y, z, pts, &axes);
    const unsigned long long b1 = __ballot(n >= 1), b2 = __ballot(n >= 2), b3 = __ballot(n >= 3);
    if (kEmit) {
      const unsigned long long r = base + (unsigned long long)(__popcll(b1 & below) +
                                                               __popcll(b2 & below) +
                                                               __popcll(b3 & below));
#pragma unroll
      for (int l = 0; l < 3; ++l)  // (unrolled: pts stays in registers)
        if (l < n && r + l < cap) {
          if constexpr (kAttr) {
            uint32_t *dst = reinterpret_cast<uint32_t *>(out) + (size_t)(r + l) * kVertexWords;
            st_vertex(dst, pts[l]);
            vertex_attr(v, aff, x, y, z, (axes >> (2 * l)) & 3, dst + 3);
          } else {
            st3(out, (size_t)(r + l), pts[l]);
          }
        }
    }
    const unsigned wt = (unsigned)(__popcll(b1) + __popcll(b2) + __popcll(b3));
    base += wt;
    total += wt;
  }
  return total;
}

// Marching cubes (§8 f5; C5 asks for a mesh, the reference has none).  Cube
// (x, y, z) = the 8 voxels (x+dx, y+dy, z+dz); all 8 must have weight > 0;
// corner c = dx | dy<<1 | dz<<2 is inside when its tsdf < 0.  `tab` (256 x
// 16 bytes, built by the host, kfx_export.hip build_mc_table) lists per configuration
// the triangles as edge indices (edge e: axis e/4, the 4 edges of an axis in
// ascending lower-corner order).  An edge vertex interpolates the two voxel
// centres as the point extraction does (FullScan6, tsdf_volume.cu:341-360),
// then the volume pose.  Triangles come out in the canonical order of the
// point cloud (8-slice chunk, tile, z, lane, triangle), 9 floats each.
// kAttr: also writes the 7-word attributed vertex (kfx_vertex) to dst.
template <bool kAttr = false, typename View>
__device__ __forceinline__ f3 mc_vertex(const View &v, const DevPose &aff, int x, int y, int z, int e,
                                        const float (&F)[8], uint32_t *dst = nullptr) {
  const int a = e >> 2, k = e & 3;
  // lower corner of edge e: the k-th corner (ascending) with bit a clear
  int c = 0, m = 0;
  for (int q = 0; q < 8; ++q)
    if (!((q >> a) & 1)) {
      if (m == k) c = q;
      ++m;
    }
  const int cn = c | (1 << a);
  f3 V = {(vw_coord(v, 0, x + (c & 1)) + 0.5f) * v.vs[0], (vw_coord(v, 1, y + ((c >> 1) & 1)) + 0.5f) * v.vs[1],
          (vw_coord(v, 2, z + ((c >> 2) & 1)) + 0.5f) * v.vs[2]};
  const float Fa = F[c], Fb = F[cn];
  const float Va = a == 0 ? V.x : (a == 1 ? V.y : V.z);
  const float Vn = Va + v.vs[a];
  const float d_inv = 1.f / (fabsf(Fa) + fabsf(Fb));
  const float cc = (Va * fabsf(Fb) + Vn * fabsf(Fa)) * d_inv;
  if (a == 0) V.x = cc;
  else if (a == 1) V.y = cc;
  else V.z = cc;
  const f3 p = add(rmul(aff.R, V), {aff.t[0], aff.t[1], aff.t[2]});
  if constexpr (kAttr) {
    st_vertex(dst, p);
    vertex_attr(v, aff, x + (c & 1), y + ((c >> 1) & 1), z + ((c >> 2) & 1), a, dst + 3);
  }
  return p;
}

// One marching-cubes wave's brick (as extract_wave): triangles in the
// canonical order, 9 floats each.
// kAttr (emit only): 21 words per triangle (3 kfx_vertex).
template <bool kEmit, bool kAttr = false, typename View>
__device__ __forceinline__ unsigned mesh_wave(const View &v, const DevPose &aff, const uint8_t *__restrict__ tab,
                                              int x, int y, int z0, int z1, unsigned long long base, float *out,
                                              unsigned long long cap) {
  const int lane = threadIdx.x & 63;
  unsigned total = 0;
  for (int z = z0; z < z1; ++z) {
    float F[8];
    int cfg = 0, nt = 0;
    if (vw_above(v, 0, x) && vw_above(v, 1, y)) {
      bool all = true;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const auto i = vw_index(v, x + (c & 1), y + ((c >> 1) & 1), z + ((c >> 2) & 1));
        all = all && vw_weight(v, i) > 0;
        F[c] = (float)vw_tsdf(v, i) * kDivShortMax;
        cfg |= (F[c] < 0.f ? 1 : 0) << c;
      }
      if (all) nt = tab[16 * cfg];
    }
    // wave prefix of the triangle counts (lane order)
    int incl = nt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (kEmit) {
      const unsigned long long r0 = base + (unsigned long long)(incl - nt);
      for (int t = 0; t < nt; ++t) {
        if (r0 + t >= cap) break;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if constexpr (kAttr)
            (void)mc_vertex<true>(v, aff, x, y, z, tab[16 * cfg + 1 + 3 * t + k], F,
                                  reinterpret_cast<uint32_t *>(out) + (size_t)(3 * (r0 + t) + k) * kVertexWords);
          else
            st3(out, (size_t)(3 * (r0 + t) + k), mc_vertex(v, aff, x, y, z, tab[16 * cfg + 1 + 3 * t + k], F));
        }
      }
    }
    const unsigned wt = (unsigned)__shfl(incl, 63);
    base += wt;
    total += wt;
  }
  return total;
}

// ---- indexed mesh ----------------------------------------------
// A mesh vertex is the grid edge it lies on, owned by its lower voxel a (b = a
// + e_axis).  The edge is used iff its ends differ in sign and one of the four
// cubes around it (at a, a - e_j, a - e_k, a - e_j - e_k for the two other
// axes) is complete: inside the view with all 8 weights > 0.  These are the
// edges mesh_wave's triangles name, each once.
// Returns the used edges of voxel (x, y, z) as a mask, bit axis.
template <typename View>
__device__ __forceinline__ int owned_edges(const View &v, int x, int y, int z) {
  const auto ia = vw_index(v, x, y, z);
  if (vw_weight(v, ia) <= 0) return 0;  // a is a corner of all four cubes
  const bool na = vw_tsdf(v, ia) < 0;
  const int q[3] = {x, y, z};
  int mask = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!vw_above(v, a, q[a])) continue;
    const auto ib = vw_index(v, x + (a == 0), y + (a == 1), z + (a == 2));
    if (vw_weight(v, ib) <= 0 || (vw_tsdf(v, ib) < 0) == na) continue;
    const int j = (a + 1) % 3, k = (a + 2) % 3;
    bool used = false;
#pragma unroll
    for (int s = 0; s < 4; ++s) {  // the cube at a - (s & 1) e_j - (s >> 1) e_k
      const int sj = s & 1, sk = s >> 1;
      if (!(sj ? vw_below(v, j, q[j]) : vw_above(v, j, q[j])) || !(sk ? vw_below(v, k, q[k]) : vw_above(v, k, q[k])))
        continue;
      int o[3] = {x, y, z};
      o[j] -= sj;
      o[k] -= sk;
      bool all = true;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        all = all && vw_weight(v, vw_index(v, o[0] + (c & 1), o[1] + ((c >> 1) & 1), o[2] + ((c >> 2) & 1))) > 0;
      used = used || all;
    }
    if (used) mask |= 1 << a;
  }
  return mask;
}

// The vertex of the edge from voxel (x, y, z) along `a`: mc_vertex<true>'s 7
// words for that edge (the same expressions in the same order).
template <typename View>
__device__ __forceinline__ void edge_vertex(const View &v, const DevPose &aff, int x, int y, int z, int a,
                                            uint32_t *dst) {
  f3 V = {(vw_coord(v, 0, x) + 0.5f) * v.vs[0], (vw_coord(v, 1, y) + 0.5f) * v.vs[1],
          (vw_coord(v, 2, z) + 0.5f) * v.vs[2]};
  const float Fa = (float)vw_tsdf(v, vw_index(v, x, y, z)) * kDivShortMax;
  const float Fb = (float)vw_tsdf(v, vw_index(v, x + (a == 0), y + (a == 1), z + (a == 2))) * kDivShortMax;
  const float Va = a == 0 ? V.x : (a == 1 ? V.y : V.z);
  const float Vn = Va + v.vs[a];
  const float d_inv = 1.f / (fabsf(Fa) + fabsf(Fb));
  const float cc = (Va * fabsf(Fb) + Vn * fabsf(Fa)) * d_inv;
  if (a == 0) V.x = cc;
  else if (a == 1) V.y = cc;
  else V.z = cc;
  const f3 p = add(rmul(aff.R, V), {aff.t[0], aff.t[1], aff.t[2]});
  st_vertex(dst, p);
  vertex_attr(v, aff, x, y, z, a, dst + 3);
}

// A vertex's key inside its unit (8 x 8 x 8 voxels: a window unit or a world
// brick), < kEdgeKeys; ascends with the canonical order (z & 7, lane, axis).
constexpr int kEdgeKeys = 8 * 64 * 3;
__device__ __forceinline__ unsigned edge_key(int x, int y, int z, int a) {
  return (unsigned)((((z & 7) * 64 + (y & 7) * 8 + (x & 7)) * 3) + a);
}

// One wave's unit (as extract_wave): kEmit = false returns the count of its
// used owned edges; true also writes each one's vertex at verts[base + rank]
// and its key at keys[base + rank], rank = the canonical order inside the unit.
template <bool kEmit, typename View>
__device__ __forceinline__ unsigned edge_wave(const View &v, const DevPose &aff, int x, int y, int z0, int z1,
                                              unsigned long long base, uint32_t *verts, uint16_t *keys) {
  const int lane = threadIdx.x & 63;
  unsigned total = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int z = z0; z < z1; ++z) {
    const int m = owned_edges(v, x, y, z);
    const int n = __popc((unsigned)m);
    const unsigned long long b1 = __ballot(n >= 1), b2 = __ballot(n >= 2), b3 = __ballot(n >= 3);
    if (kEmit) {
      unsigned long long r = base + (unsigned long long)(__popcll(b1 & below) + __popcll(b2 & below) +
                                                         __popcll(b3 & below));
#pragma nounroll  // (one copy of the attribute code, as mc_vertex with its runtime axis: 3 copies take 185 VGPRs)
      for (int a = 0; a < 3; ++a)
        if ((m >> a) & 1) {
          edge_vertex(v, aff, x, y, z, a, verts + (size_t)r * kVertexWords);
          keys[r] = (uint16_t)edge_key(x, y, z, a);
          ++r;
        }
    }
    const unsigned wt = (unsigned)(__popcll(b1) + __popcll(b2) + __popcll(b3));
    base += wt;
    total += wt;
  }
  return total;
}

// The index of the vertex with key `key` among the n keys at keys[first ..]
// (ascending); 0xFFFFFFFF when it is not there (a bug the tests catch).
__device__ __forceinline__ uint32_t edge_find(const uint16_t *__restrict__ keys, unsigned long long first, unsigned n,
                                              unsigned key) {
  unsigned lo = 0, hi = n;  // first position with keys[first + position] >= key
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    if (keys[first + mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && keys[first + lo] == key) ? (uint32_t)(first + lo) : 0xffffffffu;
}

// mesh_wave's triangles of one unit as indices: tris[3 (base + rank) + corner] =
// find(x, y, z, axis) of the corner's edge, (x, y, z) its owner voxel in the
// view's coordinates (the cube's voxel + the edge's lower corner).
template <typename View, typename Find>
__device__ __forceinline__ void index_wave(const View &v, const uint8_t *__restrict__ tab, int x, int y, int z0, int z1,
                                           unsigned long long base, uint32_t *tris, const Find &find) {
  const int lane = threadIdx.x & 63;
  for (int z = z0; z < z1; ++z) {
    int cfg = 0, nt = 0;
    if (vw_above(v, 0, x) && vw_above(v, 1, y)) {
      bool all = true;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const auto i = vw_index(v, x + (c & 1), y + ((c >> 1) & 1), z + ((c >> 2) & 1));
        all = all && vw_weight(v, i) > 0;
        cfg |= (vw_tsdf(v, i) < 0 ? 1 : 0) << c;
      }
      if (all) nt = tab[16 * cfg];
    }
    int incl = nt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    const unsigned long long r0 = base + (unsigned long long)(incl - nt);
    for (int t = 0; t < 3 * nt; ++t) {
      const int e = tab[16 * cfg + 1 + t];
      const int a = e >> 2, k = e & 3;
      const int c = ((k >> a) << (a + 1)) | (k & ((1 << a) - 1));  // the k-th corner (ascending) with bit a clear
      tris[(size_t)(3 * r0 + t)] = find(x + (c & 1), y + ((c >> 1) & 1), z + ((c >> 2) & 1), a);
    }
    base += (unsigned)__shfl(incl, 63);
  }
}

}  // namespace
}  // namespace kfx
