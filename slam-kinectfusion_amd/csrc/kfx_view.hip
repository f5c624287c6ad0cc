// kfx_view.hip — free-viewpoint render of the volume (kfx_render_view,
// DESIGN.md §18): the reference raycast (tsdf_volume.cu:210-260) from any
// camera through any intrinsics, shaded in the same launch (k_render's Phong
// or normal colours, or the fused colour) and stored as uchar3.  One launch
// per view; it reads the volume and its occupancy maps and writes only the
// view's own buffers.
#include "kfx_view_march.h"

namespace kfx {
namespace {

// The window's colour corners for fused_colour (kfx_view_march.h): a corner
// counts if it lies in the volume and on this slab.
__device__ __forceinline__ void window_corners(const VolView &v, int gx, int gy, int gz, uint32_t (&c)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {  // the 8 gathers back to back
    const int x = gx + (k >> 2), y = gy + ((k >> 1) & 1), z = gz + (k & 1);
    const bool in = (unsigned)x < (unsigned)v.X && (unsigned)y < (unsigned)v.Y && z >= 0 && z < v.Z &&
                    (unsigned)(z - v.zb) < (unsigned)v.zn;
    c[k] = in ? (v.rgb[vox_index(v, x, y, z)] & 0xFFFFFFu) : 0u;
  }
}

// A wave is an 8x8 pixel tile, a block 16x16 (k_raycast's shape: XCD-banded
// tile order, the same march: sample-index bound, batches of kR samples,
// empty-space skip over bocc / socc, one normal pass per wave with the
// two-trip normal).  The pose and intrinsics are kernel arguments (scalar
// loads); no DevState, no resize, no slab code, no block barrier.
//
// Set-up, shading, blend and store are kfx_view_march.h's pieces.  The loop in
// between is view_march's, written out here over the window: under the shared
// function this kernel, at 5 waves per SIMD, loses to its parent (DESIGN.md
// §18).  Any change to the loop goes into view_march as well.  What the window
// does differently from the brick grid on purpose: one round trip per batch;
// the __all(interior) fast path only with 32-bit indices (kIdx32); the edge
// path masks pm / nm with the sample's validity; the slab checks apply (zb / zn
// in voxel2tsdf, tri32_ok, the colour corners' test).
template <bool kIdx32>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kIdx32 ? KFX_RAY_OCC : KFX_RAY_SLAB_OCC)))
void k_view(VolView v, ViewArgs a, RayConsts rc) {
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
    float tprev = live ? voxel2tsdf(v, rc, nextp) : NAN;
    constexpr int kR = KFX_RAY_KR;
    int sprev = isnan(tprev) ? 0 : (tprev > 0.f ? 1 : (tprev < 0.f ? -1 : 0));
    uint32_t kbase = 1u;  // loop sample index of the batch's first sample
    const RayMem<kIdx32> mem(v);
    const float hx = (float)(v.X - 2), hy = (float)(v.Y - 2), hz = (float)(v.Z - 2);
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
        // non-negative or NaN, the samples inside the clear box are only replayed
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
            tprev = voxel2tsdf(v, rc, nextp);
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
          interior = left == kR && fminf(ua.x, ub.x) >= 1.f && fmaxf(ua.x, ub.x) <= hx && fminf(ua.y, ub.y) >= 1.f &&
                     fmaxf(ua.y, ub.y) <= hy && fminf(ua.z, ub.z) >= 1.f && fmaxf(ua.z, ub.z) <= hz;
        }
        if (kIdx32 && __all(interior)) {
#pragma unroll
          for (int j = 0; j < kR; ++j) {
            nextp = add(nextp, vstep);
            const float fx = rintf(nextp.x * rc.vs_inv.x);
            const float fy = rintf(nextp.y * rc.vs_inv.y);
            const float fz = rintf(nextp.z * rc.vs_inv.z);
            raw[j] = mem.ld(live, (int)fx, (int)fy, (int)fz);  // dead lanes: no access, 0
            pm |= raw[j] > 0 ? (1u << j) : 0u;
            nm |= raw[j] < 0 ? (1u << j) : 0u;
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
            raw[j] = mem.ld(val, (int)fx, (int)fy, (int)fz);
            pm |= (val && raw[j] > 0) ? (1u << j) : 0u;
            nm |= (val && raw[j] < 0) ? (1u << j) : 0u;
          }
          am = (1u << left) - 1u;
        }
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
        const f3 n = compute_normal<kIdx32>(v, rc, cvert);
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
    } else if (a.type == 0 || !fused_colour(rc, hvert, pix, [&](int gx, int gy, int gz, uint32_t (&c)[8]) { window_corners(v, gx, gy, gz, c); })) {
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

}  // namespace

void launch_view(hipStream_t s, VolView v, LevelGeom g, DevPose cam2vol, const float eye[3], int type, uint8_t *out,
                 float *vmap, float *nmap, float *ts) {
  RayConsts rc;
  ViewArgs a;
  const dim3 grd = view_fill(v, g, cam2vol, eye, type, out, vmap, nmap, ts, rc, a);
  // 32-bit tsdf byte offsets (24-bit operands of the tile * zn products), as launch_raycast
  const bool idx32 = !v.force64 && v.local_voxels() < (1ull << 31) && (size_t)v.tiles_x * v.tiles_y < (1ull << 24) &&
                     v.zn < (1 << 24);
  if (idx32) hipLaunchKernelGGL((k_view<true>), grd, dim3(256), 0, s, v, a, rc);
  else hipLaunchKernelGGL((k_view<false>), grd, dim3(256), 0, s, v, a, rc);
}

}  // namespace kfx
