// kfx_quality.hip — the ICP residual map and the tracking-quality record
// (kfx_stage_icp_residuals, kfx_score_poses, kfx_frame_quality, kfx_score_view;
// DESIGN.md §26).  The correspondence gates of k_icp_acc (kfx_kernels.hip
// icp_lane; rigid_icp.cu:46-113) stated again for one pixel, with the outcome
// handed out per pixel instead of folded into the 27 sums: a label byte (the
// first gate that rejects, or accept), the accepted residual, and per pose a
// 64-byte record of six counts, the fixed-point sum of r^2 and max |r|.
// Plain launches only: no grid barrier, no wait loop, no cooperative launch.
#include <algorithm>

#include "../../include/kfx.h"
#include "kfx_internal.h"
#include "kfx_device.h"
#include "kfx_ray.h"
#include "kfx_sqrtbound.h"

namespace kfx {
namespace {

constexpr int kQThreads = 256;
constexpr int kQWaves = kQThreads / 64;
constexpr int kQPix = 4;                       // consecutive pixels of the image per lane: one label dword
constexpr int kQBlockPix = kQThreads * kQPix;  // pixels per block
constexpr int kQMaxChunk = 16;                 // poses one block walks at the most
constexpr int kQFillBlocks = 512;              // the grid a batch aims for: two blocks on each of 256 CUs

// the record as the device adds into it: kfx_icp_quality with max_abs_r as its bits (the host sets the level)
struct QRec {
  unsigned long long n[6];
  unsigned long long sum_r2;
  unsigned max_bits;  // max |r| as its float bits (non-negative floats order as unsigned)
  int level;
};
static_assert(sizeof(QRec) == sizeof(kfx_icp_quality), "the device record is the public one");

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off);
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off));
  return v;
}
__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)v >> 32), off);
    v += (long long)(((unsigned long long)hi << 32) | lo);
  }
  return v;
}

// One block: kQBlockPix consecutive pixels of the whole image (pixel block
// blockIdx.x % pb), lane L the four pixels 4 L .. 4 L + 3 of them, against
// poses [c * chunk, + chunk) of the batch, c = blockIdx.x / pb.  The lane's
// current-frame vertex and normal stay in registers over the chunk; a pose is
// wave-uniform (scalar loads), so the gather of the model maps at the
// projection is the only per-pose memory traffic.  Per pose the block adds
// once into the pose's record: counts and sum_r2 with 64-bit integer adds,
// max |r| with an unsigned max on the float's bits; all order-independent.
// kStore (one pose): labels as one dword and residuals as one 16-byte store per
// lane; a lane whose four pixels hang over the image's end stores them singly.
template <bool kStore>
__global__ __launch_bounds__(kQThreads) void k_quality(LevelGeom g, int xe, int ye, const float *__restrict__ cv,
                                                       const float *__restrict__ cn, const float *__restrict__ pv,
                                                       const float *__restrict__ pn, float dist2_max, float sine2_max,
                                                       const DevPose *__restrict__ poses, int n, int chunk, int pb,
                                                       QRec *__restrict__ rec, float *__restrict__ residual,
                                                       uint8_t *__restrict__ label) {
  const int npix = g.w * g.h;
  const int pblk = blockIdx.x % pb;
  const int i0 = (pblk * kQThreads + threadIdx.x) * kQPix;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  f3 n0[kQPix], v0[kQPix];
  bool in[kQPix], cov[kQPix];
  if (i0 + kQPix <= npix) {
    // 48 consecutive bytes of each map, 16-byte aligned (the maps are device allocations, i0 a multiple of 4)
    float a[12], b[12];
    typedef float nf4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) nf4 *gf4;
    gf4 an = (gf4)(cn + 3 * (size_t)i0), av = (gf4)(cv + 3 * (size_t)i0);
    // (the empty statement keeps these six 16-byte loads from being merged with the other branch's per-pixel loads)
    asm volatile("" : "+v"(an), "+v"(av));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const nf4 x = an[k], y = av[k];
      a[4 * k] = x.x, a[4 * k + 1] = x.y, a[4 * k + 2] = x.z, a[4 * k + 3] = x.w;
      b[4 * k] = y.x, b[4 * k + 1] = y.y, b[4 * k + 2] = y.z, b[4 * k + 3] = y.w;
    }
#pragma unroll
    for (int q = 0; q < kQPix; ++q) {
      n0[q] = {a[3 * q], a[3 * q + 1], a[3 * q + 2]};
      v0[q] = {b[3 * q], b[3 * q + 1], b[3 * q + 2]};
      in[q] = true;
    }
  } else {
#pragma unroll
    for (int q = 0; q < kQPix; ++q) {
      in[q] = i0 + q < npix;
      const size_t idx = in[q] ? (size_t)(i0 + q) : 0;
      n0[q] = ld3(cn, idx);
      v0[q] = ld3(cv, idx);
    }
  }
  int y = i0 / g.w, x = i0 - y * g.w;
#pragma unroll
  for (int q = 0; q < kQPix; ++q) {
    cov[q] = in[q] && x < xe && y < ye;  // the floor-covered region (A2); outside it: KFX_ICP_UNCOVERED
    if (++x == g.w) x = 0, ++y;
  }
  // the waves' partials of two poses in turn, so that one barrier per pose is enough
  __shared__ unsigned s_cnt[2][kQWaves][2];
  __shared__ unsigned s_max[2][kQWaves];
  __shared__ long long s_sum[2][kQWaves];
  const int k0 = (blockIdx.x / pb) * chunk, k1 = min(n, k0 + chunk);
  for (int k = k0; k < k1; ++k) {
    const DevPose P = poses[k];  // wave-uniform
    const f3 t = {P.t[0], P.t[1], P.t[2]};
    f3 vcur[kQPix];
    int j[kQPix];
    bool ok[kQPix];
#pragma unroll
    for (int q = 0; q < kQPix; ++q) {
      vcur[q] = add(rmul(P.R, v0[q]), t);
      const int px = f2i_rn((vcur[q].x / vcur[q].z) * g.fx + g.cx);
      const int py = f2i_rn((vcur[q].y / vcur[q].z) * g.fy + g.cy);
      ok[q] = vcur[q].z > 0 && px >= 0 && py >= 0 && px < g.w && py < g.h;
      j[q] = (cov[q] && !isnan(n0[q].x) && ok[q]) ? py * g.w + px : 0;
    }
    // unconditional loads, issued together (a rejected pixel reads pixel 0), as icp_lane
    f3 vpre[kQPix], npre[kQPix];
#pragma unroll
    for (int q = 0; q < kQPix; ++q) {
      vpre[q] = ld3(pv, j[q]);
      npre[q] = ld3(pn, j[q]);
    }
    // counts of labels 1..3 and 4..5 in 9-bit fields (a wave has 256 pixels); label 0's follows from the total
    unsigned c123 = 0u, c45 = 0u, mx = 0u, lab4 = 0u;
    long long s2 = 0;
    float res[kQPix];
#pragma unroll
    for (int q = 0; q < kQPix; ++q) {
      const f3 dd = sub(vcur[q], vpre[q]);
      const bool near = dot(dd, dd) <= dist2_max;  // NaN fails, as sqrtf(x) <= t does
      const f3 sa = cross(rmul(P.R, n0[q]), npre[q]);
      const bool aligned = dot(sa, sa) <= sine2_max;
      const float r = dot(npre[q], sub(vpre[q], vcur[q]));
      const unsigned lab = !cov[q]           ? KFX_ICP_UNCOVERED
                           : isnan(n0[q].x) ? KFX_ICP_NAN
                           : !ok[q]          ? KFX_ICP_PROJ
                           : !near           ? KFX_ICP_DIST
                           : !aligned        ? KFX_ICP_ANGLE
                                             : KFX_ICP_ACCEPT;
      const bool acc = lab == KFX_ICP_ACCEPT;
      res[q] = acc ? r : 0.f;
      if (in[q]) {
        c123 += (lab >= 1u && lab <= 3u) ? 1u << (9 * (lab - 1u)) : 0u;
        c45 += lab >= 4u ? 1u << (9 * (lab - 4u)) : 0u;
      }
      // rint(RN(r * r) * 2^32): the scaling is exact, |r| is a row entry (below 2^7: icp_exact_pixels), so < 2^46
      s2 += acc ? (long long)rintf((r * r) * 4294967296.0f) : 0ll;
      mx = max(mx, acc ? __float_as_uint(fabsf(r)) : 0u);
      lab4 |= lab << (8 * q);
    }
    if (kStore) {
      if (i0 + kQPix <= npix) {
        *reinterpret_cast<uint32_t *>(label + i0) = lab4;
        *reinterpret_cast<float4 *>(residual + i0) = make_float4(res[0], res[1], res[2], res[3]);
      } else {
#pragma unroll
        for (int q = 0; q < kQPix; ++q)
          if (in[q]) {
            label[i0 + q] = (uint8_t)(lab4 >> (8 * q));
            residual[i0 + q] = res[q];
          }
      }
    }
    c123 = wave_sum(c123);
    c45 = wave_sum(c45);
    mx = wave_max(mx);
    s2 = wave_sum64(s2);
    const int sl = k & 1;
    if (lane == 0) {
      s_cnt[sl][wv][0] = c123;
      s_cnt[sl][wv][1] = c45;
      s_max[sl][wv] = mx;
      s_sum[sl][wv] = s2;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
      // thread f adds field f of the record: n[0..5], sum_r2, max |r|
      const int f = threadIdx.x;
      unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
      long long sum = 0;
      unsigned m = 0u;
#pragma unroll
      for (int w = 0; w < kQWaves; ++w) {
        const unsigned a = s_cnt[sl][w][0], b = s_cnt[sl][w][1];
        cnt[1] += a & 511u, cnt[2] += (a >> 9) & 511u, cnt[3] += (a >> 18) & 511u;
        cnt[4] += b & 511u, cnt[5] += (b >> 9) & 511u;
        sum += s_sum[sl][w];
        m = max(m, s_max[sl][w]);
      }
      const int blockpix = min(kQBlockPix, npix - pblk * kQBlockPix);
      cnt[0] = (unsigned long long)blockpix - cnt[1] - cnt[2] - cnt[3] - cnt[4] - cnt[5];
      unsigned long long add = (unsigned long long)sum;
#pragma unroll
      for (int q = 0; q < 6; ++q) add = f == q ? cnt[q] : add;
      QRec *r = rec + k;
      if (f < 7) {
        if (add) __hip_atomic_fetch_add(f < 6 ? &r->n[f] : &r->sum_r2, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else if (m) {
        __hip_atomic_fetch_max(&r->max_bits, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

}  // namespace

int quality_chunk(int w, int h, long long n) {
  const long long pb = std::max(1ll, ((long long)w * h + kQBlockPix - 1) / kQBlockPix);
  const long long want = (kQFillBlocks + pb - 1) / pb;  // chunks that fill the grid
  return (int)std::max(1ll, std::min((long long)kQMaxChunk, n / want));
}

void launch_quality(hipStream_t s, const LevelGeom &g, const float *cv, const float *cn, const float *pv, const float *pn,
                    float dist_thr, float angle_thr, const DevPose *poses, int n, void *rec, float *residual,
                    uint8_t *label) {
  const int xe = (g.w / 32) * 32, ye = (g.h / 32) * 32;
  const int pb = std::max(1, (g.w * g.h + kQBlockPix - 1) / kQBlockPix);
  const float d2 = sqrt_le_bound(dist_thr), s2 = sqrt_le_bound(angle_thr);
  if (residual || label) {  // one pose, with the per-pixel stores
    hipLaunchKernelGGL((k_quality<true>), dim3(pb), dim3(kQThreads), 0, s, g, xe, ye, cv, cn, pv, pn, d2, s2, poses, 1,
                       1, pb, static_cast<QRec *>(rec), residual, label);
    return;
  }
  const int chunk = quality_chunk(g.w, g.h, n);
  hipLaunchKernelGGL((k_quality<false>), dim3(pb * ((n + chunk - 1) / chunk)), dim3(kQThreads), 0, s, g, xe, ye, cv, cn,
                     pv, pn, d2, s2, poses, n, chunk, pb, static_cast<QRec *>(rec), nullptr, nullptr);
}

}  // namespace kfx
