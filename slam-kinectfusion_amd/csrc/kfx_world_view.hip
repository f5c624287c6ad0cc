// kfx_world_view.hip — free-viewpoint render of a world (kfx_world_view,
// DESIGN.md §25): k_view's raycast (kfx_view.hip) over a sparse
// list of kfx_brick records instead of the dense window.  The march, the normal
// pass, the shading and the store are k_view's; only the voxel fetch differs:
// a lookup in a dense grid of the box's bricks (record number + 1, 0: absent),
// then a read from the record.  An absent brick reads as 0 without a second
// access.  The load kernels build that grid and §4's dilated occupancy maps
// from the records, in a VolView-shaped descriptor, so kfx_ray.h's skip_limit
// runs unchanged (it only replays nextp additions: exact).
//
// shade_*, fused_colour's arithmetic and the store are a second copy of
// kfx_view.hip's: that file and its ISA stay as they are.
#include <algorithm>
#include <climits>
#include <cmath>

#include "kfx_internal.h"
#include "kfx_device.h"
#include "kfx_ffadd.h"
#include "kfx_ray.h"
#include "kfx_raystep.h"

namespace kfx {
namespace {

constexpr unsigned kRecBytes = 3600;  // sizeof(kfx_brick): 16 header, 1024 tsdf, 512 weight, 2048 colour
constexpr unsigned kRecTsdf = 16, kRecRgb = 16 + 1024 + 512;

struct ViewArgs {
  LevelGeom g;     // the view's intrinsics
  DevPose c2v;     // cam2vol = box_pose^-1 * cam_pose (Rinv = its R transposed)
  float eye[3];    // cam_pose.t: the Phong shader's eye
  int type;        // KFX_VIEW_*
  uint8_t *out;    // w * h uchar3
  float *vmap, *nmap, *ts;  // optional (null: not stored)
};

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

// kernel_renderPhong / kernel_renderNormals on one pixel's maps (kfx_view.hip's, copied)
__device__ __forceinline__ unsigned shade_normal(f3 nv) {
  return (unsigned)render_u8(fabsf(nv.x) * 255) | ((unsigned)render_u8(fabsf(nv.y) * 255) << 8) |
         ((unsigned)render_u8(fabsf(nv.z) * 255) << 16);
}
__device__ __forceinline__ unsigned shade_phong(f3 nv, f3 vv, f3 eye) {
  if ((nv.x == 0 && nv.y == 0 && nv.z == 0) || (vv.x == 0 && vv.y == 0 && vv.z == 0)) return 0u;
  const f3 kd = {0.3843f, 0.4745f, 0.580f};
  const float intensity = 0.9f;
  const f3 e = normalized_ieee(sub(eye, vv));
  const f3 l = normalized_ieee(sub({500.f, 500.f, -500.f}, vv));
  float lc = dot(nv, l);
  if (lc <= 0) lc = -lc;
  float coef = intensity * lc;
  const f3 diffuse = scl(kd, coef);
  const f3 hv = normalized_ieee(add(l, e));
  float hc = dot(nv, hv);
  if (hc < 0) hc = -hc;
  const float h2 = hc * hc, h4 = h2 * h2, h8 = h4 * h4;
  coef = intensity * (h8 * h2);
  const double spec = 0.5 * (double)coef;
  const unsigned o0 = render_u8((float)fmin(1.0, (double)(0.1f + diffuse.x) + spec) * 255);
  const unsigned o1 = render_u8((float)fmin(1.0, (double)(0.1f + diffuse.y) + spec) * 255);
  const unsigned o2 = render_u8((float)fmin(1.0, (double)(0.1f + diffuse.z) + spec) * 255);
  return o0 | (o1 << 8) | (o2 << 16);
}

// The fused colour at box position P ("lies in the volume" read
// as "lies in the box"): kfx_view.hip's blend, the corners read through the grid.
template <bool kIdx32>
__device__ __forceinline__ bool wv_colour(const VolView &v, const WorldMem<kIdx32> &m, const RayConsts &rc, f3 P,
                                          unsigned &pix) {
  const f3 cf = mulc(P, rc.vs_inv);
  const int gx = f2i_rd(cf.x), gy = f2i_rd(cf.y), gz = f2i_rd(cf.z);
  const int qx = (int)((cf.x - (float)gx) * 256.f), qy = (int)((cf.y - (float)gy) * 256.f),
            qz = (int)((cf.z - (float)gz) * 256.f);
  uint32_t c[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {  // the 8 grid words back to back
    const int x = gx + (k >> 2), y = gy + ((k >> 1) & 1), z = gz + (k & 1);
    const bool in = (unsigned)x < (unsigned)v.X && (unsigned)y < (unsigned)v.Y && (unsigned)z < (unsigned)v.Z;
    c[k] = m.cell(in, x, y, z);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k)  // then the 8 gathers
    c[k] = m.rgb(c[k], in_brick(gx + (k >> 2), gy + ((k >> 1) & 1), gz + (k & 1))) & 0xFFFFFFu;
  unsigned sw = 0u, s0 = 0u, s1 = 0u, s2 = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const unsigned wx = (k >> 2) ? qx : 256 - qx, wy = ((k >> 1) & 1) ? qy : 256 - qy, wz = (k & 1) ? qz : 256 - qz;
    const unsigned W = c[k] ? wx * wy * wz : 0u;
    sw += W;
    s0 += W * (c[k] & 0xFFu);
    s1 += W * ((c[k] >> 8) & 0xFFu);
    s2 += W * ((c[k] >> 16) & 0xFFu);
  }
  if (sw == 0u) return false;
  const unsigned h = sw >> 1;
  pix = ((s0 + h) / sw) | (((s1 + h) / sw) << 8) | (((s2 + h) / sw) << 16);
  return true;
}

// (k_view's view_ray_len: out of line, and this file's own copy)
__device__ __attribute__((noinline)) float wv_ray_len(float L0, float step, int n) { return ff_add(L0, step, n); }

#ifndef KFX_WV_KR
#define KFX_WV_KR KFX_RAY_KR  // samples per batch: a grid word and a tsdf load in flight per sample
#endif

// k_view over the grid (kfx_view.hip has the march's commentary).  Per batch
// two round trips: the kR grid words, then the kR tsdf loads.
template <bool kIdx32>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KFX_RAY_SLAB_OCC)))
void k_world_view(VolView v, ViewArgs a, RayConsts rc, WorldGrid wg) {
  const LevelGeom g = a.g;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nbx = (g.w + 15) / 16;
  const int t = xcd_remap(blockIdx.x, gridDim.x);
  const int tx0 = (t % nbx) * 16 + (wv & 1) * 8, ty0 = (t / nbx) * 16 + (wv >> 1) * 8;  // the wave's tile
  const int x = tx0 + (lane & 7), y = ty0 + (lane >> 3);
  const bool inimg = x < g.w && y < g.h;
  const size_t o = (size_t)y * g.w + x;
  f3 vout = {0.f, 0.f, 0.f}, nout = {0.f, 0.f, 0.f}, hvert = {0.f, 0.f, 0.f};
  float hts = 0.f;
  bool hit = false;
  const WorldMem<kIdx32> mem(v, wg);
  {
    const f3 org = {a.c2v.t[0], a.c2v.t[1], a.c2v.t[2]};
    float da[3];
    ray_dir(a.c2v.R, g, x, y, da);
    const f3 dir = {da[0], da[1], da[2]};
    const f3 invR = {1.f / dir.x, 1.f / dir.y, 1.f / dir.z};
    const f3 tbot = mulc(invR, sub({0.f, 0.f, 0.f}, org));
    const f3 ttop = mulc(invR, sub({v.range[0], v.range[1], v.range[2]}, org));
    const f3 tmin = {fminf(ttop.x, tbot.x), fminf(ttop.y, tbot.y), fminf(ttop.z, tbot.z)};
    const f3 tmax = {fmaxf(ttop.x, tbot.x), fmaxf(ttop.y, tbot.y), fmaxf(ttop.z, tbot.z)};
    const float tnear = fmaxf(fmaxf(tmin.x, tmin.y), fmaxf(tmin.x, tmin.z));
    const float tfar = fminf(fminf(tmax.x, tmax.y), fminf(tmax.x, tmax.z));
    const float ray0 = fmaxf(tnear, 0.f);
    bool live = inimg && ray0 < tfar;
    const f3 vstep = mulc(dir, rc.vs);
    const float L0 = ray0 + rc.step;
    const uint32_t kend = 1u + (uint32_t)ray_sample_end(L0, rc.step, live ? tfar : L0);
    f3 nextp = add(org, scl(dir, L0));
    float tprev = live ? wv_voxel2tsdf(v, mem, rc, nextp) : NAN;
    constexpr int kR = KFX_WV_KR;
    int sprev = isnan(tprev) ? 0 : (tprev > 0.f ? 1 : (tprev < 0.f ? -1 : 0));
    uint32_t kbase = 1u;  // loop sample index of the batch's first sample
    const float hx = (float)(v.X - 2), hy = (float)(v.Y - 2), hz = (float)(v.Z - 2);
    bool cand = false;
    f3 r_nextp = nextp;
    float cq = 0.f;  // the candidate's Ts = its sample's ray_len - cq
    float r_tprev = 0.f;
    uint32_t ckey = 0u;  // the candidate's sample index
    const f3 dv = mulc(vstep, rc.vs_inv);  // per-sample displacement in voxels
    const f3 idv = {1.f / fabsf(dv.x), 1.f / fabsf(dv.y), 1.f / fabsf(dv.z)};
    const bool can_skip = !isnan(dv.x + dv.y + dv.z);
    while (__any(live || cand)) {
      while (__any(live)) {
        // empty-space skip (exact): absent bricks and bricks without a negative
        // tsdf are clear in the maps the load built
        if (can_skip && live && sprev >= 0) {
          uint32_t nsk = 0;
          for (;;) {
            const float cx = nextp.x * rc.vs_inv.x, cy = nextp.y * rc.vs_inv.y, cz = nextp.z * rc.vs_inv.z;
            const float lim = skip_limit(v, cx, cy, cz, dv, idv);
            if (!(lim >= 1.f)) break;
            const int n = (int)fminf(lim, rc.skip_cap);
            const int rem = (int)(kend - kbase - nsk);  // samples the loop has left
            if (rem <= n) {  // all of them in the clear box: no event follows
              live = false;
              break;
            }
            int i = 0;
            for (; i + 8 <= n; i += 8) {
#pragma unroll
              for (int u = 0; u < 8; ++u) nextp = add(nextp, vstep);
            }
            for (; i < n; ++i) nextp = add(nextp, vstep);
            nsk += (uint32_t)n;
          }
          if (nsk != 0u && live) {
            kbase += nsk;
            tprev = wv_voxel2tsdf(v, mem, rc, nextp);
            sprev = isnan(tprev) ? 0 : (tprev > 0.f ? 1 : (tprev < 0.f ? -1 : 0));
          }
        }
        if (!__any(live)) break;
        int16_t raw[kR];
        unsigned cl[kR];             // the samples' grid words
        unsigned io[(kR + 1) / 2];   // their places in the brick, two per register
        unsigned pm = 0u, nm = 0u, am = 0u;
        const int left = live ? (int)min(kend - kbase, (uint32_t)kR) : 0;  // samples of this batch below kend
        const f3 p0 = nextp;  // position before the batch's first sample
        bool interior = !live;
        if (live) {
          const f3 ua = mulc(add(p0, vstep), rc.vs_inv);
          const f3 ub = mulc(add(p0, scl(vstep, (float)kR)), rc.vs_inv);
          interior = left == kR && fminf(ua.x, ub.x) >= 1.f && fmaxf(ua.x, ub.x) <= hx && fminf(ua.y, ub.y) >= 1.f &&
                     fmaxf(ua.y, ub.y) <= hy && fminf(ua.z, ub.z) >= 1.f && fmaxf(ua.z, ub.z) <= hz;
        }
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
            const bool val = in & (fx >= 1.f) & (fx <= hx) & (fy >= 1.f) & (fy <= hy) & (fz >= 1.f) & (fz <= hz);
            cl[j] = mem.cell(val, (int)fx, (int)fy, (int)fz);
            io[j >> 1] |= in_brick((int)fx, (int)fy, (int)fz) << (16 * (j & 1));
          }
          am = (1u << left) - 1u;
        }
#pragma unroll
        for (int j = 0; j < kR; ++j) {  // a rejected sample's word is 0: it reads 0, sign 0
          raw[j] = mem.tsdf(cl[j], (io[j >> 1] >> (16 * (j & 1))) & 0x1FFu);
          pm |= raw[j] > 0 ? (1u << j) : 0u;
          nm |= raw[j] < 0 ? (1u << j) : 0u;
        }
        const int je = __builtin_ctz(~am);  // first sample outside [.., kend) (kR if none)
        const unsigned pprev = (pm << 1) | (sprev > 0 ? 1u : 0u);
        const unsigned nprev = (nm << 1) | (sprev < 0 ? 1u : 0u);
        const unsigned hitm = pprev & nm;
        const unsigned ev = live ? (hitm | (nprev & pm)) : 0u;
        const float tfirst = tprev;
        sprev = ((pm >> (kR - 1)) & 1u) ? 1 : (((nm >> (kR - 1)) & 1u) ? -1 : 0);
        tprev = (float)raw[kR - 1] * kDivShortMax;
        if (ev != 0u) {
          const int j0 = __ffs(ev) - 1;
          if ((hitm >> j0) & 1u) {
            float tc = tfirst, tn = 0.f;
#pragma unroll
            for (int j = 0; j < kR; ++j) {
              const float tj = (float)raw[j] * kDivShortMax;
              if (j + 1 == j0) tc = tj;
              if (j == j0) tn = tj;
            }
            cq = (v.vs[0] * tc) / (tc - tn);  // Ts = ray_len - cq
            cand = true;
            ckey = kbase + (uint32_t)j0;
            f3 pj = p0;  // resume state: sample j0 was processed, the next is j0 + 1
#pragma unroll
            for (int j = 0; j < kR; ++j)
              if (j <= j0) pj = add(pj, vstep);
            r_nextp = pj;
            r_tprev = tn;
          }
          live = false;  // a candidate, or tsdf_cur < 0 && tsdf_next > 0: stop, no surface
        }
        if (je < kR) live = false;  // left [.., kend) inside this batch
        kbase += kR;
      }
      bool resume = false;
      if (cand) {  // the wave's normal pass
        cand = false;
        const float Ts = wv_ray_len(L0, rc.step, (int)ckey - 1) - cq;
        const f3 cvert = add(org, scl(dir, Ts));
        const f3 n = wv_normal(v, mem, rc, cvert);
        if (!isnan(n.x * n.y * n.z)) {
          nout = n;
          hts = Ts;
          hit = true;
        } else {  // NaN normal: keep marching after the candidate
          resume = true;
        }
      }
      live = resume;
      nextp = r_nextp;
      kbase = ckey + 1u;
      sprev = -1;
      tprev = r_tprev;
    }
    if (hit) {
      float ri[9];  // Rinv = cam2vol's R transposed (scalar loads)
#pragma unroll
      for (int q = 0; q < 9; ++q) ri[q] = a.c2v.R[3 * (q % 3) + q / 3];
      hvert = add(org, scl(dir, hts));
      nout = rmul(ri, nout);
      vout = rmul(ri, sub(hvert, org));
    }
  }
  // shade: a miss (or a lane outside the image) is 0
  unsigned pix = 0u;
  if (hit) {
    const f3 eye = {a.eye[0], a.eye[1], a.eye[2]};
    if (a.type == 1) {
      pix = shade_normal(nout);
    } else if (a.type == 0 || !wv_colour(v, mem, rc, hvert, pix)) {
      pix = shade_phong(nout, vout, eye);
    }
  }
  if (inimg) {
    if (a.vmap) st3(a.vmap, o, vout);
    if (a.nmap) st3(a.nmap, o, nout);
    if (a.ts) a.ts[o] = hts;
  }
  // Store (k_view's): lane (r, k) assembles the aligned dword k of row r's
  // 24-byte segment from the row's packed pixels and stores it whole; a dword
  // that hangs over an end of the segment is stored as its bytes.
  {
    const int r = lane >> 3, k = lane & 7;
    const int ry = ty0 + r;
    const int nb = (ry < g.h && tx0 < g.w) ? 3 * min(8, g.w - tx0) : 0;  // bytes of the row segment
    const size_t gb = ((size_t)ry * g.w + tx0) * 3;                      // its first byte in the image
    const int head = (int)(gb & 3);
    unsigned word = 0u, okm = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rb = 4 * k - head + j;  // byte of the row segment
      const bool ok = rb >= 0 && rb < nb;
      const int rc3 = ok ? rb : 0;
      const int px = rc3 / 3, ch = rc3 - 3 * px;
      const unsigned p = (unsigned)__shfl((int)pix, (r << 3) | px);
      word |= ((p >> (8 * ch)) & 0xFFu) << (8 * j);
      okm |= ok ? (1u << j) : 0u;
    }
    uint8_t *dst = a.out + (gb - head) + 4 * (size_t)k;
    if (okm == 0xFu) {
      *reinterpret_cast<uint32_t *>(dst) = word;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((okm >> j) & 1u) dst[j] = (uint8_t)(word >> (8 * j));
    }
  }
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
  rc.vs = {v.vs[0], v.vs[1], v.vs[2]};
  rc.vs_inv = {1.f / v.vs[0], 1.f / v.vs[1], 1.f / v.vs[2]};
  rc.gd = {v.vs[0] * 0.5f, v.vs[1] * 0.5f, v.vs[2] * 0.5f};
  rc.step = v.vs[0];
  // half an ulp of a position inside the box is <= max_dim * 2^-23 voxels (launch_view)
  rc.skip_cap = std::min(511.f, std::floor(0.1f * 8388608.f / (float)std::max(v.X, std::max(v.Y, v.Z))));
  ViewArgs a{};
  a.g = g;
  a.c2v = cam2vol;
  for (int i = 0; i < 3; ++i) a.eye[i] = eye[i];
  a.type = type;
  a.out = out;
  a.vmap = vmap;
  a.nmap = nmap;
  a.ts = ts;
  const dim3 grd(((g.w + 15) / 16) * ((g.h + 15) / 16));
  // 32-bit byte offsets into the records (24-bit operands: the record number, the column products)
  const bool idx32 = !v.force64 && wg.n * (size_t)kRecBytes < (1ull << 32) && wg.n < (1u << 24) &&
                     (size_t)v.tiles_x * v.tiles_y < (1ull << 24);
  if (idx32) hipLaunchKernelGGL((k_world_view<true>), grd, dim3(256), 0, s, v, a, rc, wg);
  else hipLaunchKernelGGL((k_world_view<false>), grd, dim3(256), 0, s, v, a, rc, wg);
}

}  // namespace kfx
