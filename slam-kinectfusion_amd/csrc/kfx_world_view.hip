// kfx_world_view.hip — free-viewpoint render of a world (kfx_world_view,
// DESIGN.md §25): the view's march (kfx_view_march.h) over a
// sparse list of kfx_brick records instead of the dense window.  Only the voxel
// source is this file's: a lookup in a dense grid of the box's bricks (record
// number + 1, 0: absent), then a read from the record.  An absent brick reads
// as 0 without a second access.  The load kernels build that grid and §4's
// dilated occupancy maps from the records, in a VolView-shaped descriptor, so
// kfx_ray.h's skip_limit runs unchanged (it only replays nextp additions: exact).
#include <climits>

#include "kfx_view_march.h"

namespace kfx {
namespace {

constexpr unsigned kRecBytes = 3600;  // sizeof(kfx_brick): 16 header, 1024 tsdf, 512 weight, 2048 colour
constexpr unsigned kRecTsdf = 16, kRecRgb = 16 + 1024 + 512;

// Voxel reads through the grid.  cell(): the grid word of voxel (x, y, z)'s
// brick (0: absent, or a rejected sample); tsdf() / rgb(): the record's value
// at the voxel's place in its brick (cell 0: 0, no access).  kIdx32 (records
// below 2^32 bytes): buffer loads with 32-bit byte offsets, a rejected lane
// reads 0 past the end without a memory access; else 64-bit pointers.
__device__ __forceinline__ unsigned in_brick(int x, int y, int z) {
  return (((unsigned)z & 7u) << 6) | (((unsigned)y & 7u) << 3) | ((unsigned)x & 7u);
}
template <bool kIdx32>
struct WorldMem;
template <>
struct WorldMem<true> {
  __amdgpu_buffer_rsrc_t g, r;
  unsigned gx, gz;
  __device__ WorldMem(const VolView &v, const WorldGrid &w)
      : g(make_rsrc(w.grid, (unsigned)(4 * w.cells))), r(make_rsrc(w.recs, (unsigned)(w.n * kRecBytes))),
        gx((unsigned)v.tiles_x), gz((unsigned)v.nbz) {}
  __device__ unsigned cell(bool valid, int x, int y, int z) const {
    const unsigned col = __umul24((unsigned)y >> 3, gx) + ((unsigned)x >> 3);
    const unsigned idx = col * gz + ((unsigned)z >> 3);
    return (unsigned)__builtin_amdgcn_raw_buffer_load_b32(g, valid ? idx * 4u : kOob, 0, 0);
  }
  __device__ int16_t tsdf(unsigned c, unsigned io) const {
    return (int16_t)__builtin_amdgcn_raw_buffer_load_b16(r, c ? __umul24(c - 1u, kRecBytes) + kRecTsdf + 2u * io : kOob, 0, 0);
  }
  __device__ uint32_t rgb(unsigned c, unsigned io) const {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, c ? __umul24(c - 1u, kRecBytes) + kRecRgb + 4u * io : kOob, 0, 0);
  }
};
template <>
struct WorldMem<false> {
  const uint32_t *g;
  const char *r;
  int gx, gz;
  __device__ WorldMem(const VolView &v, const WorldGrid &w) : g(w.grid), r((const char *)w.recs), gx(v.tiles_x), gz(v.nbz) {}
  __device__ unsigned cell(bool valid, int x, int y, int z) const {
    return valid ? g[((size_t)(y >> 3) * gx + (x >> 3)) * (size_t)gz + (z >> 3)] : 0u;
  }
  __device__ int16_t tsdf(unsigned c, unsigned io) const {
    return c ? *(const int16_t *)(r + (size_t)(c - 1u) * kRecBytes + kRecTsdf + 2u * io) : (int16_t)0;
  }
  __device__ uint32_t rgb(unsigned c, unsigned io) const {
    return c ? *(const uint32_t *)(r + (size_t)(c - 1u) * kRecBytes + kRecRgb + 4u * io) : 0u;
  }
};

// kfx_ray.h's voxel2tsdf through the grid (the same bounds: a volume's
// outermost voxel layer is never read)
template <bool kIdx32>
__device__ __forceinline__ float wv_voxel2tsdf(const VolView &v, const WorldMem<kIdx32> &m, const RayConsts &rc, f3 p) {
  const int x = f2i_rn(p.x * rc.vs_inv.x);
  const int y = f2i_rn(p.y * rc.vs_inv.y);
  const int z = f2i_rn(p.z * rc.vs_inv.z);
  if (x >= v.X - 1 || y >= v.Y - 1 || z >= v.Z - 1 || x < 1 || y < 1 || z < 1) return NAN;
  return (float)m.tsdf(m.cell(true, x, y, z), in_brick(x, y, z)) * kDivShortMax;
}

// compute_normal's two trips of three interpolations (kfx_ray.h): per trip the
// 24 corners' grid words back to back, then their 24 tsdf loads, then the three
// weighted sums in the reference's order (tri32_sum: r[4 dx + 2 dy + dz]).
template <bool kIdx32>
__device__ __forceinline__ void wv_trip(const VolView &v, const WorldMem<kIdx32> &m, const f3 (&cf)[3], float (&f)[3]) {
  unsigned c[24];
  int16_t r[24];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int gx = f2i_rd(cf[q].x), gy = f2i_rd(cf[q].y), gz = f2i_rd(cf[q].z);
    const bool ok = tri32_ok(v, gx, gy, gz);
#pragma unroll
    for (int k = 0; k < 8; ++k) c[8 * q + k] = m.cell(ok, gx + (k >> 2), gy + ((k >> 1) & 1), gz + (k & 1));
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int gx = f2i_rd(cf[q].x), gy = f2i_rd(cf[q].y), gz = f2i_rd(cf[q].z);
#pragma unroll
    for (int k = 0; k < 8; ++k) r[8 * q + k] = m.tsdf(c[8 * q + k], in_brick(gx + (k >> 2), gy + ((k >> 1) & 1), gz + (k & 1)));
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) f[q] = tri32_sum(v, cf[q], r + 8 * q);
}
template <bool kIdx32>
__device__ f3 wv_normal(const VolView &v, const WorldMem<kIdx32> &m, const RayConsts &rc, f3 p) {
  f3 n;
  float f[3];
  {
    const f3 cf[3] = {mulc({p.x + rc.gd.x, p.y, p.z}, rc.vs_inv), mulc({p.x - rc.gd.x, p.y, p.z}, rc.vs_inv),
                      mulc({p.x, p.y + rc.gd.y, p.z}, rc.vs_inv)};
    wv_trip(v, m, cf, f);
  }
  n.x = (f[0] - f[1]) / rc.gd.x;
  const float fy1 = f[2];
  {
    const f3 cf[3] = {mulc({p.x, p.y - rc.gd.y, p.z}, rc.vs_inv), mulc({p.x, p.y, p.z + rc.gd.z}, rc.vs_inv),
                      mulc({p.x, p.y, p.z - rc.gd.z}, rc.vs_inv)};
    wv_trip(v, m, cf, f);
  }
  n.y = (fy1 - f[0]) / rc.gd.y;
  n.z = (f[1] - f[2]) / rc.gd.z;
  return normalized(n);
}

// The brick grid as the march's voxel source (kfx_view_march.h).  "Lies in the
// volume" reads as "lies in the box": no slab, so no slab checks beyond the
// ones tri32_ok makes with zb = 0, zn = Z.
template <bool kIdx32>
struct BrickSrc {
  const VolView &v;
  const RayConsts &rc;
  const WorldMem<kIdx32> mem;
  __device__ __forceinline__ BrickSrc(const VolView &vv, const RayConsts &r, const WorldGrid &w) : v(vv), rc(r), mem(vv, w) {}
  __device__ __forceinline__ float tsdf(f3 p) const { return wv_voxel2tsdf(v, mem, rc, p); }
  // Two round trips per batch: the kR grid words, then the kR tsdf loads, the
  // samples' places in their bricks carried two per register between them.
  // Both index widths take the interior path.  No sign masks: a rejected
  // sample's word is 0, which reads 0 (sign 0) without a second access.
  __device__ __forceinline__ void batch(bool live, int left, bool interior, f3 hi, f3 vstep, f3 &nextp,
                                        int16_t (&raw)[kViewKR], unsigned &pm, unsigned &nm, unsigned &am) const {
    constexpr int kR = kViewKR;
    unsigned cl[kR];            // the samples' grid words
    unsigned io[(kR + 1) / 2];  // their places in the brick, two per register
#pragma unroll
    for (int j = 0; j < (kR + 1) / 2; ++j) io[j] = 0u;
    if (__all(interior)) {
#pragma unroll
      for (int j = 0; j < kR; ++j) {
        nextp = add(nextp, vstep);
        const int ix = (int)rintf(nextp.x * rc.vs_inv.x);
        const int iy = (int)rintf(nextp.y * rc.vs_inv.y);
        const int iz = (int)rintf(nextp.z * rc.vs_inv.z);
        cl[j] = mem.cell(live, ix, iy, iz);  // dead lanes: no access, 0
        io[j >> 1] |= in_brick(ix, iy, iz) << (16 * (j & 1));
      }
      am = (1u << kR) - 1u;
    } else {
#pragma unroll
      for (int j = 0; j < kR; ++j) {
        const bool in = j < left;  // lanes past kend or dead keep stepping, masked off
        nextp = add(nextp, vstep);
        const float fx = rintf(nextp.x * rc.vs_inv.x);
        const float fy = rintf(nextp.y * rc.vs_inv.y);
        const float fz = rintf(nextp.z * rc.vs_inv.z);
        const bool val = in & (fx >= 1.f) & (fx <= hi.x) & (fy >= 1.f) & (fy <= hi.y) & (fz >= 1.f) & (fz <= hi.z);
        cl[j] = mem.cell(val, (int)fx, (int)fy, (int)fz);
        io[j >> 1] |= in_brick((int)fx, (int)fy, (int)fz) << (16 * (j & 1));
      }
      am = (1u << left) - 1u;
    }
#pragma unroll
    for (int j = 0; j < kR; ++j) {
      raw[j] = mem.tsdf(cl[j], (io[j >> 1] >> (16 * (j & 1))) & 0x1FFu);
      pm |= raw[j] > 0 ? (1u << j) : 0u;
      nm |= raw[j] < 0 ? (1u << j) : 0u;
    }
  }
  __device__ __forceinline__ f3 normal(f3 p) const { return wv_normal(v, mem, rc, p); }
  __device__ __forceinline__ void corners(int gx, int gy, int gz, uint32_t (&c)[8]) const {
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // the 8 grid words back to back
      const int x = gx + (k >> 2), y = gy + ((k >> 1) & 1), z = gz + (k & 1);
      const bool in = (unsigned)x < (unsigned)v.X && (unsigned)y < (unsigned)v.Y && (unsigned)z < (unsigned)v.Z;
      c[k] = mem.cell(in, x, y, z);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)  // then the 8 gathers
      c[k] = mem.rgb(c[k], in_brick(gx + (k >> 2), gy + ((k >> 1) & 1), gz + (k & 1))) & 0xFFFFFFu;
  }
};

template <bool kIdx32>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KFX_RAY_SLAB_OCC)))
void k_world_view(VolView v, ViewArgs a, RayConsts rc, WorldGrid wg) {
  view_march(v, a, rc, BrickSrc<kIdx32>(v, rc, wg));
}

// ---------------------------------------------------------------------------
// Load: one wave per record.  A record whose brick lies in the box enters the
// grid (lane 0) and, where it holds a negative tsdf, marks the dilated
// occupancy maps as integrate does for a window brick (occ_mark; voxels past
// the box may mark too: the maps are supersets).  Grid and maps were cleared.
__global__ __launch_bounds__(256) void k_wv_load(VolView v, WorldGrid wg, int ob0, int ob1, int ob2) {
  const int lane = threadIdx.x & 63;
  const size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= wg.n) return;
  const char *rec = (const char *)wg.recs + i * kRecBytes;
  const int4 h = *(const int4 *)rec;
  const long long q0 = (long long)h.x - ob0, q1 = (long long)h.y - ob1, q2 = (long long)h.z - ob2;
  if (q0 < 0 || q0 >= v.tiles_x || q1 < 0 || q1 >= v.tiles_y || q2 < 0 || q2 >= v.nbz) return;  // (wave-uniform)
  const int bx = (int)q0, by = (int)q1, bz = (int)q2;
  if (lane == 0) wg.grid[((size_t)by * v.tiles_x + bx) * (size_t)v.nbz + bz] = (uint32_t)(i + 1);
  const uint4 tq = *(const uint4 *)(rec + kRecTsdf + 16 * lane);  // voxels 8 lane .. 8 lane + 7: slice dz = lane >> 3
  const bool neg = (int16_t)tq.x < 0 || (int16_t)(tq.x >> 16) < 0 || (int16_t)tq.y < 0 || (int16_t)(tq.y >> 16) < 0 ||
                   (int16_t)tq.z < 0 || (int16_t)(tq.z >> 16) < 0 || (int16_t)tq.w < 0 || (int16_t)(tq.w >> 16) < 0;
  const int z = 8 * bz + (lane >> 3);
  if (__any(neg)) occ_mark_wave(v, by * v.tiles_x + bx, neg ? z : INT_MAX, neg ? z : -1, lane);
}

}  // namespace

void launch_world_view_load(hipStream_t s, VolView v, WorldGrid wg, const int origin[3]) {
  (void)hipMemsetAsync(wg.grid, 0, 4 * wg.cells, s);
  (void)hipMemsetAsync(v.bocc, 0, v.bocc_bytes(), s);
  (void)hipMemsetAsync(v.socc, 0, v.socc_bytes(), s);
  hipLaunchKernelGGL(k_wv_load, dim3((unsigned)((wg.n + 3) / 4)), dim3(256), 0, s, v, wg, origin[0] / 8, origin[1] / 8,
                     origin[2] / 8);
}

void launch_world_view(hipStream_t s, VolView v, WorldGrid wg, LevelGeom g, DevPose cam2vol, const float eye[3], int type,
                       uint8_t *out, float *vmap, float *nmap, float *ts) {
  RayConsts rc;
  ViewArgs a;
  const dim3 grd = view_fill(v, g, cam2vol, eye, type, out, vmap, nmap, ts, rc, a);
  // 32-bit byte offsets into the records (24-bit operands: the record number, the column products)
  const bool idx32 = !v.force64 && wg.n * (size_t)kRecBytes < (1ull << 32) && wg.n < (1u << 24) &&
                     (size_t)v.tiles_x * v.tiles_y < (1ull << 24);
  if (idx32) hipLaunchKernelGGL((k_world_view<true>), grd, dim3(256), 0, s, v, a, rc, wg);
  else hipLaunchKernelGGL((k_world_view<false>), grd, dim3(256), 0, s, v, a, rc, wg);
}

}  // namespace kfx
