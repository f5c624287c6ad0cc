// kfx_view_march.h — the free-viewpoint render as code that
// exists once: the kernels' argument block, the pixel and ray set-up, the two
// shaders, the fused-colour blend, the out-of-line ray_len helper, the packed
// store, the launchers' fill, and view_march<Src>: the whole march over a voxel
// source.  k_world_view (kfx_world_view.hip, §25) is view_march over the brick
// grid.  k_view (kfx_view.hip) uses the same pieces around a march loop of its
// own: at 5 waves per SIMD it does not hold the parent's time under the shared
// loop (§18).
//
// A voxel source answers four questions and nothing else:
//   float tsdf(f3 p)            the tsdf at position p (voxel2tsdf), NaN: outside;
//   void batch(live, left, interior, hi, vstep, nextp, raw, pm, nm, am)
//                               the raw values of one batch of kViewKR samples:
//                               steps nextp (on entry p0, the position before the
//                               batch's first sample) by vstep per sample; raw[j]
//                               = sample j's stored tsdf (0: rejected), pm / nm =
//                               the samples with a positive / negative value, am =
//                               the samples below kend (`left` of them; all where
//                               the whole wave's batch is interior);
//   f3 normal(f3 p)             the normal at p (compute_normal), NaN: none;
//   void corners(gx, gy, gz, c) the 24-bit colours of the 8 corners of cell
//                               (gx, gy, gz), c[4 dx + 2 dy + dz]; 0: no colour.
// As kfx_ray.h, everything lives in an unnamed namespace.
#pragma once
#include <algorithm>
#include <cmath>

#include "kfx_internal.h"
#include "kfx_device.h"
#include "kfx_ffadd.h"
#include "kfx_ray.h"
#include "kfx_raystep.h"

namespace kfx {
namespace {

struct ViewArgs {
  LevelGeom g;     // the view's intrinsics
  DevPose c2v;     // cam2vol = volume_pose^-1 * cam_pose (Rinv = its R transposed); a world: box_pose^-1 * cam_pose
  float eye[3];    // cam_pose.t: the Phong shader's eye
  int type;        // KFX_VIEW_*
  uint8_t *out;    // w * h uchar3
  float *vmap, *nmap, *ts;  // optional (null: not stored)
};

constexpr int kViewKR = KFX_RAY_KR;  // samples per batch (loads in flight per lane)

// A lane's pixel: a wave is an 8x8 pixel tile at (tx0, ty0), a block 16x16,
// tiles dealt in XCD bands (k_raycast's shape).  o: the pixel's index in the maps.
struct ViewPix {
  int lane, tx0, ty0, x, y;
  bool inimg;
  size_t o;
};
__device__ __forceinline__ ViewPix view_pix(const LevelGeom &g) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nbx = (g.w + 15) / 16;
  const int t = xcd_remap(blockIdx.x, gridDim.x);
  const int tx0 = (t % nbx) * 16 + (wv & 1) * 8, ty0 = (t / nbx) * 16 + (wv >> 1) * 8;  // the wave's tile
  const int x = tx0 + (lane & 7), y = ty0 + (lane >> 3);
  return {lane, tx0, ty0, x, y, x < g.w && y < g.h, (size_t)y * g.w + x};
}

// The pixel's ray in volume coordinates and its slab test against the volume
// box [0, range] (tsdf_volume.cu:215-233): marched over (ray0, tfar) if live.
struct ViewRay {
  f3 org, dir;
  float ray0, tfar;
  bool live;
};
__device__ __forceinline__ ViewRay view_ray(const DevPose &c2v, const LevelGeom &g, const VolView &v, const ViewPix &px) {
  const f3 org = {c2v.t[0], c2v.t[1], c2v.t[2]};
  float da[3];
  ray_dir(c2v.R, g, px.x, px.y, da);
  const f3 dir = {da[0], da[1], da[2]};
  const f3 invR = {1.f / dir.x, 1.f / dir.y, 1.f / dir.z};
  const f3 tbot = mulc(invR, sub({0.f, 0.f, 0.f}, org));
  const f3 ttop = mulc(invR, sub({v.range[0], v.range[1], v.range[2]}, org));
  const f3 tmin = {fminf(ttop.x, tbot.x), fminf(ttop.y, tbot.y), fminf(ttop.z, tbot.z)};
  const f3 tmax = {fmaxf(ttop.x, tbot.x), fmaxf(ttop.y, tbot.y), fmaxf(ttop.z, tbot.z)};
  const float tnear = fmaxf(fmaxf(tmin.x, tmin.y), fmaxf(tmin.x, tmin.z));
  const float tfar = fminf(fminf(tmax.x, tmax.y), fminf(tmax.x, tmax.z));
  const float ray0 = fmaxf(tnear, 0.f);
  return {org, dir, ray0, tfar, px.inimg && ray0 < tfar};
}

// kernel_renderPhong / kernel_renderNormals on one pixel's maps: k_render's
// arithmetic (kfx_extract.hip) with the eye passed in.  Packed c0 | c1 << 8 | c2 << 16.
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

// The fused colour at position P: trilinear blend of the
// coloured corners in 8-bit fixed-point weights, all in integers.  Returns
// false when no corner counts (outside the source, or never coloured: packed
// 24-bit colour 0).
template <class Corners>
__device__ __forceinline__ bool fused_colour(const RayConsts &rc, f3 P, unsigned &pix, Corners corners) {
  const f3 cf = mulc(P, rc.vs_inv);
  const int gx = f2i_rd(cf.x), gy = f2i_rd(cf.y), gz = f2i_rd(cf.z);
  const int qx = (int)((cf.x - (float)gx) * 256.f), qy = (int)((cf.y - (float)gy) * 256.f),
            qz = (int)((cf.z - (float)gz) * 256.f);
  uint32_t c[8];
  corners(gx, gy, gz, c);  // c[4 dx + 2 dy + dz]: the corner's 24-bit colour, 0 where it does not count
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

// A candidate sample's ray_len: n adds of step to L0, exactly (kfx_ffadd.h).
// Out of line, once per normal pass: inlined, the loop's temporaries spill
// k_view<true> at 5 waves per SIMD (68 bytes of scratch per lane).  The view's
// own, so that a view file adds no second body of kfx::ff_add_call.
__device__ __attribute__((noinline)) float view_ray_len(float L0, float step, int n) { return ff_add(L0, step, n); }

// The packed store of a wave's tile: a tile row is 8 pixels = 24 bytes of one
// image row.  Lane (r, k) = (lane >> 3, lane & 7) assembles the aligned dword k
// of row r's segment from the row's packed pixels with four lane reads
// (ds_bpermute: no LDS allocation, no barrier) and stores it whole; only a
// dword that hangs over an end of the segment (an unaligned row start, the
// image's right edge) is stored as its bytes.  Rows below the image and dwords
// outside the segment store nothing.
__device__ __forceinline__ void view_store(uint8_t *out, const LevelGeom &g, int tx0, int ty0, int lane, unsigned pix) {
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
  uint8_t *dst = out + (gb - head) + 4 * (size_t)k;
  if (okm == 0xFu) {
    *reinterpret_cast<uint32_t *>(dst) = word;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((okm >> j) & 1u) dst[j] = (uint8_t)(word >> (8 * j));
  }
}

// One pixel per lane: a wave is an 8x8 pixel tile, a block 16x16 (k_raycast's
// shape: XCD-banded tile order, the same march: sample-index bound, batches of
// kViewKR samples, empty-space skip over bocc / socc, one normal pass per wave).
// The pose and intrinsics are kernel arguments (scalar loads); no DevState, no
// resize, no slab code, no block barrier.  v: the window, or the descriptor of
// a world's box (its dims, voxel size, range and occupancy maps).
template <class Src>
__device__ __forceinline__ void view_march(const VolView &v, const ViewArgs &a, const RayConsts &rc, const Src &src) {
  const LevelGeom g = a.g;
  const ViewPix px = view_pix(g);
  const int lane = px.lane, tx0 = px.tx0, ty0 = px.ty0;
  const bool inimg = px.inimg;
  const size_t o = px.o;
  f3 vout = {0.f, 0.f, 0.f}, nout = {0.f, 0.f, 0.f}, hvert = {0.f, 0.f, 0.f};
  float hts = 0.f;
  bool hit = false;
  {
    const ViewRay ray = view_ray(a.c2v, g, v, px);
    const f3 org = ray.org, dir = ray.dir;
    const float tfar = ray.tfar, ray0 = ray.ray0;
    bool live = ray.live;
    const f3 vstep = mulc(dir, rc.vs);
    // samples 1 .. kend - 1 of the reference's loop (kfx_raystep.h); a hit
    // candidate's ray_len is ff_add(L0, step, k - 1)
    const float L0 = ray0 + rc.step;
    const uint32_t kend = 1u + (uint32_t)ray_sample_end(L0, rc.step, live ? tfar : L0);
    f3 nextp = add(org, scl(dir, L0));
    float tprev = live ? src.tsdf(nextp) : NAN;
    constexpr int kR = kViewKR;
    int sprev = isnan(tprev) ? 0 : (tprev > 0.f ? 1 : (tprev < 0.f ? -1 : 0));
    uint32_t kbase = 1u;  // loop sample index of the batch's first sample
    const f3 hi = {(float)(v.X - 2), (float)(v.Y - 2), (float)(v.Z - 2)};  // the last voxel a sample may round to
    // hit candidates (+/- events) are resolved once no lane of the wave is
    // marching, all in one normal pass; a NaN normal resumes the march after
    // the candidate sample from the saved state (k_raycast)
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
        // empty-space skip (exact, k_raycast): with the last sample
        // non-negative or NaN, the samples inside the clear box are only
        // replayed (a world: absent bricks and bricks without a negative tsdf
        // are clear in the maps the load built)
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
            tprev = src.tsdf(nextp);
            sprev = isnan(tprev) ? 0 : (tprev > 0.f ? 1 : (tprev < 0.f ? -1 : 0));
          }
        }
        if (!__any(live)) break;
        int16_t raw[kR];
        unsigned pm = 0u, nm = 0u, am = 0u;
        const int left = live ? (int)min(kend - kbase, (uint32_t)kR) : 0;  // samples of this batch below kend
        const f3 p0 = nextp;  // position before the batch's first sample
        // interior batch: first and (estimated) last sample round into the
        // valid voxel box with half a voxel of margin and the batch ends before kend
        bool interior = !live;
        if (live) {
          const f3 ua = mulc(add(p0, vstep), rc.vs_inv);
          const f3 ub = mulc(add(p0, scl(vstep, (float)kR)), rc.vs_inv);
          interior = left == kR && fminf(ua.x, ub.x) >= 1.f && fmaxf(ua.x, ub.x) <= hi.x && fminf(ua.y, ub.y) >= 1.f &&
                     fmaxf(ua.y, ub.y) <= hi.y && fminf(ua.z, ub.z) >= 1.f && fmaxf(ua.z, ub.z) <= hi.z;
        }
        src.batch(live, left, interior, hi, vstep, nextp, raw, pm, nm, am);
        const int je = __builtin_ctz(~am);  // first sample outside [.., kend) (kR if none)
        // an event at j: opposite signs at samples j - 1, j (NaN = sign 0);
        // +/- is a hit candidate, -/+ a stop
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
            cq = (v.vs[0] * tc) / (tc - tn);  // Ts = ray_len - cq (A3 (R))
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
        const float Ts = view_ray_len(L0, rc.step, (int)ckey - 1) - cq;
        const f3 cvert = add(org, scl(dir, Ts));
        const f3 n = src.normal(cvert);
        if (!isnan(n.x * n.y * n.z)) {
          // the march keeps only Ts and the normal: the vertex follows from Ts
          // again after it (the same float operations on the same values)
          nout = n;
          hts = Ts;
          hit = true;
        } else {  // NaN normal: keep marching after the candidate (tsdf_volume.cu:251)
          resume = true;
        }
      }
      // only a resumed lane marches again (sample ckey was processed; it is negative)
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
      hvert = add(org, scl(dir, hts));  // tsdf_volume.cu:247
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
    } else if (a.type == 0 || !fused_colour(rc, hvert, pix, [&](int gx, int gy, int gz, uint32_t (&c)[8]) { src.corners(gx, gy, gz, c); })) {
      // colour: only hit lanes gather, after the normal was accepted; a hit
      // with no coloured corner keeps its Phong value
      pix = shade_phong(nout, vout, eye);
    }
  }
  if (inimg) {
    if (a.vmap) st3(a.vmap, o, vout);
    if (a.nmap) st3(a.nmap, o, nout);
    if (a.ts) a.ts[o] = hts;
  }
  view_store(a.out, g, tx0, ty0, lane, pix);
}

// What both launchers pass: the march's constants for the voxel size and dims
// of v (the window, or a world's box) and the kernel's arguments.  Returns the
// grid: a block per 16x16 pixel tile.
inline dim3 view_fill(const VolView &v, LevelGeom g, DevPose cam2vol, const float eye[3], int type, uint8_t *out,
                      float *vmap, float *nmap, float *ts, RayConsts &rc, ViewArgs &a) {
  rc.vs = {v.vs[0], v.vs[1], v.vs[2]};
  rc.vs_inv = {1.f / v.vs[0], 1.f / v.vs[1], 1.f / v.vs[2]};
  rc.gd = {v.vs[0] * 0.5f, v.vs[1] * 0.5f, v.vs[2] * 0.5f};
  rc.step = v.vs[0];
  // half an ulp of a position inside the volume is <= max_dim * 2^-23 voxels
  rc.skip_cap = std::min(511.f, std::floor(0.1f * 8388608.f / (float)std::max(v.X, std::max(v.Y, v.Z))));
  a = ViewArgs{};
  a.g = g;
  a.c2v = cam2vol;
  for (int i = 0; i < 3; ++i) a.eye[i] = eye[i];
  a.type = type;
  a.out = out;
  a.vmap = vmap;
  a.nmap = nmap;
  a.ts = ts;
  return dim3(((g.w + 15) / 16) * ((g.h + 15) / 16));
}

}  // namespace
}  // namespace kfx
