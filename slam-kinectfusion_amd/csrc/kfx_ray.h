// kfx_ray.h — the raycast march's device functions, shared by the frame's
// raycast (kfx_kernels.hip, k_raycast) and the free-viewpoint render
// (kfx_view.hip, k_view): voxel reads, the trilinear normal, the empty-space
// skip over the occupancy maps and the tile order.  As kfx_device.h, everything
// lives in an unnamed namespace: each file gets its own internal copy.
#pragma once
#include <climits>

#include "kfx_internal.h"
#include "kfx_device.h"

namespace kfx {
namespace {

constexpr float kInf = __builtin_huge_valf();

// __float2int_rn / __float2int_rd, out-of-range -> INT_MIN (rejected by every
// bounds check, as the saturated CUDA result is)
__device__ __forceinline__ int f2i_rn(float v) {
  const float r = rintf(v);
  return (r > -2.0e9f && r < 2.0e9f) ? (int)r : INT_MIN;
}
__device__ __forceinline__ int f2i_rd(float v) {
  const float r = floorf(v);
  return (r > -2.0e9f && r < 2.0e9f) ? (int)r : INT_MIN;
}

// Blocks are dealt round-robin to the 8 XCDs; remap so that each XCD gets a
// contiguous band of work (raycast: 16x16 pixel tiles whose rays gather the
// same voxel lines; ICP: pixel rows whose correspondences gather the same
// rows of the previous maps), which then hits in that XCD's L2.  Bijective
// for any count.
__device__ __forceinline__ int xcd_remap(int b, int nb) {
  const int q = nb / 8, r = nb % 8, xcd = b % 8;
  return xcd * q + min(xcd, r) + b / 8;
}

// 32-bit-offset buffer access (raw buffer resource; loads past num_records
// return 0 and stores are dropped, so a rejected lane passes offset ~0u).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), (short)0, (int)bytes, 0x00020000);
}
constexpr unsigned kOob = 0xFFFFFFFFu;

// tsdf reads of the march: kIdx32 (local volume < 2^31 voxels) uses a buffer
// load with a 32-bit byte offset (24-bit multiplies; rejected samples read 0
// past the buffer end without a memory access), else 64-bit pointers.
template <bool kIdx32>
struct RayMem;
template <>
struct RayMem<true> {
  __amdgpu_buffer_rsrc_t t;
  unsigned zn, tiles_x;
  int zb;
  __device__ RayMem(const VolView &v)
      : t(make_rsrc(v.tsdf, (unsigned)(2 * v.local_voxels()))), zn((unsigned)v.zn),
        tiles_x((unsigned)v.tiles_x), zb(v.zb) {}
  __device__ int16_t ld(bool valid, int x, int y, int z) const {
    const unsigned ux = (unsigned)x, uy = (unsigned)y;
    const unsigned tile = __umul24(uy >> 3, tiles_x) + (ux >> 3);
    const unsigned idx = ((__umul24(tile, zn) + (unsigned)(z - zb)) << 6) | ((uy & 7u) << 3 | (ux & 7u));
    return __builtin_amdgcn_raw_buffer_load_b16(t, valid ? idx * 2u : kOob, 0, 0);
  }
};
template <>
struct RayMem<false> {
  const VolView *v;
  __device__ RayMem(const VolView &vv) : v(&vv) {}
  __device__ int16_t ld(bool valid, int x, int y, int z) const {
    return valid ? v->tsdf[vox_index(*v, x, y, z)] : (int16_t)0;
  }
};

#ifndef KFX_RAY_OCC
#define KFX_RAY_OCC 5  // raycast: waves per SIMD the register budget must allow (4800 waves at VGA: one round at 5)
#endif
#ifndef KFX_RAY_SLAB_OCC
#define KFX_RAY_SLAB_OCC 4  // slab and 64-bit-index raycasts: waves per SIMD (their extra registers spill at 5)
#endif
#ifndef KFX_RAY_KR
#define KFX_RAY_KR 14  // raycast: samples per batch (loads in flight per lane)
#endif

struct RayConsts {
  f3 vs, vs_inv, gd;
  float step;
  float skip_cap;  // most samples one skip replays (accumulated rounding < 0.1 voxel)
};

__device__ __forceinline__ float voxel2tsdf(const VolView &v, const RayConsts &rc, f3 p) {
  const int x = f2i_rn(p.x * rc.vs_inv.x);
  const int y = f2i_rn(p.y * rc.vs_inv.y);
  const int z = f2i_rn(p.z * rc.vs_inv.z);
  if (x >= v.X - 1 || y >= v.Y - 1 || z >= v.Z - 1 || x < 1 || y < 1 || z < 1) return NAN;
  if ((unsigned)(z - v.zb) >= (unsigned)v.zn) return NAN;  // not stored on this slab
  return (float)v.tsdf[vox_index(v, x, y, z)] * kDivShortMax;
}

__device__ __forceinline__ float interp(const VolView &v, f3 cf) {
  const int gx = f2i_rd(cf.x), gy = f2i_rd(cf.y), gz = f2i_rd(cf.z);
  if (gx < 0 || gx >= v.X - 1 || gy < 0 || gy >= v.Y - 1 || gz < 0 || gz >= v.Z - 1) return NAN;
  // slabs: an owned event's normal reads within the stored halo (DESIGN.md
  // §7); the check only keeps any other read in bounds
  if ((unsigned)(gz - v.zb) >= (unsigned)(v.zn - 1)) return NAN;
  const float a = cf.x - (float)gx, b = cf.y - (float)gy, c = cf.z - (float)gz;
  const float t000 = (float)v.tsdf[vox_index(v, gx, gy, gz)] * kDivShortMax;
  const float t001 = (float)v.tsdf[vox_index(v, gx, gy, gz + 1)] * kDivShortMax;
  const float t010 = (float)v.tsdf[vox_index(v, gx, gy + 1, gz)] * kDivShortMax;
  const float t011 = (float)v.tsdf[vox_index(v, gx, gy + 1, gz + 1)] * kDivShortMax;
  const float t100 = (float)v.tsdf[vox_index(v, gx + 1, gy, gz)] * kDivShortMax;
  const float t101 = (float)v.tsdf[vox_index(v, gx + 1, gy, gz + 1)] * kDivShortMax;
  const float t110 = (float)v.tsdf[vox_index(v, gx + 1, gy + 1, gz)] * kDivShortMax;
  const float t111 = (float)v.tsdf[vox_index(v, gx + 1, gy + 1, gz + 1)] * kDivShortMax;
  float s = 0.f;
  s += t000 * (1 - a) * (1 - b) * (1 - c);
  s += t001 * (1 - a) * (1 - b) * c;
  s += t010 * (1 - a) * b * (1 - c);
  s += t011 * (1 - a) * b * c;
  s += t100 * a * (1 - b) * (1 - c);
  s += t101 * a * (1 - b) * c;
  s += t110 * a * b * (1 - c);
  s += t111 * a * b * c;
  return s;
}

// interp for volumes whose local voxel count fits 32-bit offsets (kIdx32):
// the same corners, weights and sum order, but one tile-column index
// for (gx, gy, gz) and the other seven corners as offsets from it (z + 1 is
// always the next 64-voxel slice of the same column: the load's +128 B
// immediate; x + 1 / y + 1 cross into the next tile only at x & 7 == 7 /
// y & 7 == 7), read by buffer loads.  In three steps, so that the loads of
// several interpolations share one round trip: the index math (tri32_at), the
// 8 corner loads (tri32_load) and the weighted sum (tri32_sum).
struct Tri32 {
  unsigned o00, o01, o10, o11;  // byte offsets of the (x, y), (x, y+1), (x+1, y), (x+1, y+1) columns at gz
};
__device__ __forceinline__ bool tri32_ok(const VolView &v, int gx, int gy, int gz) {
  return !(gx < 0 || gx >= v.X - 1 || gy < 0 || gy >= v.Y - 1 || gz < 0 || gz >= v.Z - 1) &&
         !((unsigned)(gz - v.zb) >= (unsigned)(v.zn - 1));
}
__device__ __forceinline__ Tri32 tri32_at(const VolView &v, f3 cf) {
  const int gx = f2i_rd(cf.x), gy = f2i_rd(cf.y), gz = f2i_rd(cf.z);
  const bool ok = tri32_ok(v, gx, gy, gz);
  const unsigned col = (unsigned)v.zn << 6;  // voxels per tile column
  const unsigned tile = __umul24((unsigned)gy >> 3, (unsigned)v.tiles_x) + ((unsigned)gx >> 3);
  const unsigned i0 = ((tile * (unsigned)v.zn + (unsigned)(gz - v.zb)) << 6) | (((unsigned)gy & 7u) << 3 | ((unsigned)gx & 7u));
  const unsigned dx = (gx & 7) == 7 ? col - 7u : 1u;
  const unsigned dy = (gy & 7) == 7 ? __umul24((unsigned)v.tiles_x, col) - 56u : 8u;
  // (an invalid interpolation reads voxels 0 and 64 and returns NaN)
  Tri32 q;
  q.o00 = ok ? i0 << 1 : 0u;
  q.o01 = ok ? (i0 + dy) << 1 : 0u;
  q.o10 = ok ? (i0 + dx) << 1 : 0u;
  q.o11 = ok ? (i0 + dx + dy) << 1 : 0u;
  return q;
}
__device__ __forceinline__ void tri32_load(__amdgpu_buffer_rsrc_t t, const Tri32 &q, int16_t *r) {
  r[0] = (int16_t)__builtin_amdgcn_raw_buffer_load_b16(t, q.o00, 0, 0);
  r[1] = (int16_t)__builtin_amdgcn_raw_buffer_load_b16(t, q.o00 + 128u, 0, 0);
  r[2] = (int16_t)__builtin_amdgcn_raw_buffer_load_b16(t, q.o01, 0, 0);
  r[3] = (int16_t)__builtin_amdgcn_raw_buffer_load_b16(t, q.o01 + 128u, 0, 0);
  r[4] = (int16_t)__builtin_amdgcn_raw_buffer_load_b16(t, q.o10, 0, 0);
  r[5] = (int16_t)__builtin_amdgcn_raw_buffer_load_b16(t, q.o10 + 128u, 0, 0);
  r[6] = (int16_t)__builtin_amdgcn_raw_buffer_load_b16(t, q.o11, 0, 0);
  r[7] = (int16_t)__builtin_amdgcn_raw_buffer_load_b16(t, q.o11 + 128u, 0, 0);
}
// (the weights are taken from cf again after the loads: three registers
// instead of a, b, c carried across the round trip)
__device__ __forceinline__ float tri32_sum(const VolView &v, f3 cf, const int16_t *r) {
  const int gx = f2i_rd(cf.x), gy = f2i_rd(cf.y), gz = f2i_rd(cf.z);
  if (!tri32_ok(v, gx, gy, gz)) return NAN;
  const float a = cf.x - (float)gx, b = cf.y - (float)gy, c = cf.z - (float)gz;
  const float t000 = (float)r[0] * kDivShortMax, t001 = (float)r[1] * kDivShortMax;
  const float t010 = (float)r[2] * kDivShortMax, t011 = (float)r[3] * kDivShortMax;
  const float t100 = (float)r[4] * kDivShortMax, t101 = (float)r[5] * kDivShortMax;
  const float t110 = (float)r[6] * kDivShortMax, t111 = (float)r[7] * kDivShortMax;
  float s = 0.f;
  s += t000 * (1 - a) * (1 - b) * (1 - c);
  s += t001 * (1 - a) * (1 - b) * c;
  s += t010 * (1 - a) * b * (1 - c);
  s += t011 * (1 - a) * b * c;
  s += t100 * a * (1 - b) * (1 - c);
  s += t101 * a * (1 - b) * c;
  s += t110 * a * b * (1 - c);
  s += t111 * a * b * c;
  return s;
}

// The 6 trilinear interpolations of a normal.  kIdx32 volumes take them in
// two round trips of three: index math, then 24 corner loads back to back,
// then the three weighted sums in the reference's order (the registers for
// the second trip's loads are the first trip's: DESIGN.md §14).  64-bit
// indices: one round trip of 8 loads per interpolation (interp).
template <bool kIdx32 = false>
__device__ f3 compute_normal(const VolView &v, const RayConsts &rc, f3 p) {
  f3 n;
  if (kIdx32) {
    const __amdgpu_buffer_rsrc_t t = make_rsrc(v.tsdf, (unsigned)(2 * v.local_voxels()));
    int16_t r[24];
    float f[3];
    {
      // (tri32_at and tri32_sum must see the same c0..c2: the sum takes the
      // cell and weights from them again, bit for bit what the loads used)
      const f3 c0 = mulc({p.x + rc.gd.x, p.y, p.z}, rc.vs_inv), c1 = mulc({p.x - rc.gd.x, p.y, p.z}, rc.vs_inv),
               c2 = mulc({p.x, p.y + rc.gd.y, p.z}, rc.vs_inv);
      tri32_load(t, tri32_at(v, c0), r), tri32_load(t, tri32_at(v, c1), r + 8), tri32_load(t, tri32_at(v, c2), r + 16);
      f[0] = tri32_sum(v, c0, r), f[1] = tri32_sum(v, c1, r + 8), f[2] = tri32_sum(v, c2, r + 16);
    }
    n.x = (f[0] - f[1]) / rc.gd.x;
    const float fy1 = f[2];
    {
      const f3 c0 = mulc({p.x, p.y - rc.gd.y, p.z}, rc.vs_inv), c1 = mulc({p.x, p.y, p.z + rc.gd.z}, rc.vs_inv),
               c2 = mulc({p.x, p.y, p.z - rc.gd.z}, rc.vs_inv);
      tri32_load(t, tri32_at(v, c0), r), tri32_load(t, tri32_at(v, c1), r + 8), tri32_load(t, tri32_at(v, c2), r + 16);
      f[0] = tri32_sum(v, c0, r), f[1] = tri32_sum(v, c1, r + 8), f[2] = tri32_sum(v, c2, r + 16);
    }
    n.y = (fy1 - f[0]) / rc.gd.y;
    n.z = (f[1] - f[2]) / rc.gd.z;
    return normalized(n);
  }
  auto ip = [&](f3 q) { return interp(v, mulc(q, rc.vs_inv)); };
  const float fx1 = ip({p.x + rc.gd.x, p.y, p.z});
  const float fx2 = ip({p.x - rc.gd.x, p.y, p.z});
  n.x = (fx1 - fx2) / rc.gd.x;
  const float fy1 = ip({p.x, p.y + rc.gd.y, p.z});
  const float fy2 = ip({p.x, p.y - rc.gd.y, p.z});
  n.y = (fy1 - fy2) / rc.gd.y;
  const float fz1 = ip({p.x, p.y, p.z + rc.gd.z});
  const float fz2 = ip({p.x, p.y, p.z - rc.gd.z});
  n.z = (fz1 - fz2) / rc.gd.z;
  return normalized(n);
}

// Samples a ray may replay from voxel position c while every sample stays in
// the box that a clear dilated (super)brick run guarantees non-negative or
// NaN: per axis [B*b - B, B*b + 2B - 1] (open at the volume's edge columns),
// z [zl, zh]; each face with 0.2 voxel of margin (rint reaches a voxel only
// within 0.5 of it, the accumulated rounding of <= 511 adds stays below 0.1).
__device__ __forceinline__ float axis_limit(float c, float d, float id, float lo, float hi) {
  return d > 0.f ? (hi + 0.2f - c) * id : (d < 0.f ? (c - lo + 0.2f) * id : kInf);
}
__device__ __forceinline__ float box_limit(int B, int bx, int by, int nbx, int nby, float zl, float zh,
                                           float cx, float cy, float cz, f3 dv, f3 idv) {
  const float xl = bx > 0 ? (float)(B * bx - B) : -kInf, xh = bx < nbx - 1 ? (float)(B * bx + 2 * B - 1) : kInf;
  const float yl = by > 0 ? (float)(B * by - B) : -kInf, yh = by < nby - 1 ? (float)(B * by + 2 * B - 1) : kInf;
  return fminf(fminf(axis_limit(cx, dv.x, idv.x, xl, xh), axis_limit(cy, dv.y, idv.y, yl, yh)),
               axis_limit(cz, dv.z, idv.z, zl, zh));
}

// The brick box's lateral (x / y) exit from voxel position (cx, cy) in cell (bx, by).
__device__ __forceinline__ float brick_lateral_exit(const VolView &v, int bx, int by, float cx, float cy, f3 dv, f3 idv) {
  const float xl = bx > 0 ? (float)(8 * bx - 8) : -kInf, xh = bx < v.tiles_x - 1 ? (float)(8 * bx + 15) : kInf;
  const float yl = by > 0 ? (float)(8 * by - 8) : -kInf, yh = by < v.tiles_y - 1 ? (float)(8 * by + 15) : kInf;
  return fminf(axis_limit(cx, dv.x, idv.x, xl, xh), axis_limit(cy, dv.y, idv.y, yl, yh));
}
// The clear box of a brick column word at voxel position (cx, cy, cz) of cell
// (bx, by, lbz): the cell's 3x3 tile box with the dilated z run of clear cells
// in the direction of travel (lim < 1: blocked).
__device__ __forceinline__ float run_box(const VolView &v, unsigned long long w, int nbits, int b, int lc, int ncell,
                                         int c0, int B, int bx, int by, int nbx, int nby, float cx, float cy, float cz,
                                         f3 dv, f3 idv) {
  float zl = -kInf, zh = kInf;
  if (dv.z > 0.f) {
    const unsigned long long up = w >> b;
    const int top = lc + (up ? __builtin_ctzll(up) : nbits - b) - 1;
    if (top < ncell - 1) zh = (float)(B * (top + c0) + 2 * B - 1);
  } else {
    const unsigned long long dn = w << (63 - b);
    const int bot = lc - (dn ? __builtin_clzll(dn) : b + 1) + 1;
    if (bot > 0) zl = (float)(B * (bot + c0) - B);
  }
  return box_limit(B, bx, by, nbx, nby, zl, zh, cx, cy, cz, dv, idv);
}
// Samples a ray may replay from voxel position (cx, cy, cz) (< 1: blocked).
// The super-brick's box when its cell is clear (its 3x3 box contains the
// brick's laterally; tools/raysim: the brick box alone adds < 1 % of lookups
// there), else the brick's.  Two boxes per round trip: the words of the column at the
// brick box's lateral exit point (known before any word is back) are loaded
// in the same round trip, and that column's brick box extends the run when
// the point lies inside it (a ray along a tilted surface leaves the boxes
// sideways one after another: tools/raysim variant 8, C2's slowest wave 54
// -> 36 lookup rounds).  Every sample of the run lies in one of the boxes at
// model positions c + t dv: the same 0.2-voxel margins as one box.
__device__ __forceinline__ float skip_limit(const VolView &v, float cx, float cy, float cz, f3 dv, f3 idv) {
  const int ix = (int)floorf(cx), iy = (int)floorf(cy), iz = (int)floorf(cz);
  const int bx = min(max(ix >> 3, 0), v.tiles_x - 1), by = min(max(iy >> 3, 0), v.tiles_y - 1);
  const int lbz = min(max((iz >> 3) - v.bz0, 0), v.nbz - 1);
  const int sx = min(max(ix >> 5, 0), v.stx - 1), sy = min(max(iy >> 5, 0), v.sty - 1);
  const int lsz = min(max((iz >> 5) - v.sz0, 0), v.nsz - 1);
  const unsigned long long bwd = v.bocc[(size_t)(by * v.tiles_x + bx) * v.bw + (lbz >> 6)];
  const uint32_t swd = v.socc[(size_t)(sy * v.stx + sx) * v.sw + (lsz >> 5)];
  const float t1r = brick_lateral_exit(v, bx, by, cx, cy, dv, idv);
  const float t1 = t1r < 1.0e6f ? t1r : 0.f;  // (no lateral exit: the same column, unused)
  const float c1x = cx + t1 * dv.x, c1y = cy + t1 * dv.y, c1z = cz + t1 * dv.z;
  const int ix1 = (int)floorf(c1x), iy1 = (int)floorf(c1y), iz1 = (int)floorf(c1z);
  const int bx1 = min(max(ix1 >> 3, 0), v.tiles_x - 1), by1 = min(max(iy1 >> 3, 0), v.tiles_y - 1);
  const int lbz1 = min(max((iz1 >> 3) - v.bz0, 0), v.nbz - 1);
  const unsigned long long bwd1 = v.bocc[(size_t)(by1 * v.tiles_x + bx1) * v.bw + (lbz1 >> 6)];
  const int bb = lbz & 63, sb = lsz & 31;
  const bool sclear = !((swd >> sb) & 1u), bclear = !((bwd >> bb) & 1ull);
  float lim = 0.f;
  if (sclear || bclear) {
    lim = run_box(v, sclear ? (unsigned long long)swd : bwd, sclear ? 32 : 64, sclear ? sb : bb, sclear ? lsz : lbz,
                  sclear ? v.nsz : v.nbz, sclear ? v.sz0 : v.bz0, sclear ? 32 : 8, sclear ? sx : bx, sclear ? sy : by,
                  sclear ? v.stx : v.tiles_x, sclear ? v.sty : v.tiles_y, cx, cy, cz, dv, idv);
    const int bb1 = lbz1 & 63;
    if (t1 > 0.f && t1 <= lim && !((bwd1 >> bb1) & 1ull)) {
      const float lim1 = run_box(v, bwd1, 64, bb1, lbz1, v.nbz, v.bz0, 8, bx1, by1, v.tiles_x, v.tiles_y, c1x, c1y, c1z,
                                 dv, idv);
      if (lim1 >= 1.f) lim = fmaxf(lim, t1 + lim1);
    }
  }
  return lim;
}

}  // namespace
}  // namespace kfx
