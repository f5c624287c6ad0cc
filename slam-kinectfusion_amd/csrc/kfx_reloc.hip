// kfx_reloc.hip — fern keyframes: the frame code under a table
// of randomized ferns (k_fern_encode) and the batched nearest-keyframe search
// over a word-major code table (k_fern_search, k_fern_merge).  Plain launches
// only: no grid barrier, no wait loop, no cooperative launch; blocks hand their
// results to the merge through the kernel boundary.
#include <algorithm>

#include "kfx_internal.h"
#include "kfx_reloc.h"

namespace kfx {
namespace {

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;
constexpr int kSThreads = kSearchBlockKeys;
constexpr int kSWaves = kSThreads / 64;
static_assert(kSWaves * kSearchMaxK == 64, "a wave merges the block's per-wave lists, one key per lane");

__device__ __forceinline__ u64 shfl_xor64(u64 v, int off) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_min64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, shfl_xor64(v, off));
  return v;
}

// One thread per fern; the 16 lanes of a word OR their nibbles together and
// the group's first lane stores the word.  m is a multiple of 16, so a group of
// 16 lanes is all ferns or none.
__global__ __launch_bounds__(64) void k_fern_encode(const kfx_fern *__restrict__ table, int m,
                                                   const uint8_t *__restrict__ bgr, int width,
                                                   const float *__restrict__ dmap, int wL, int sc, u64 *code, u64 *slot,
                                                   long long stride) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  unsigned nib = 0;
  if (f < m) {
    const kfx_fern fe = table[f];
    int sb = 0, sg = 0, sr = 0;
    for (int dy = 0; dy < sc; ++dy) {
      const uint8_t *p = bgr + 3 * ((size_t)(fe.y * sc + dy) * width + (size_t)fe.x * sc);
      for (int dx = 0; dx < sc; ++dx) {
        sb += p[3 * dx];
        sg += p[3 * dx + 1];
        sr += p[3 * dx + 2];
      }
    }
    const int a = sc * sc;
    const float d = dmap[(size_t)fe.y * wL + fe.x];
    nib = (sb > fe.tb * a ? 1u : 0u) | (sg > fe.tg * a ? 2u : 0u) | (sr > fe.tr * a ? 4u : 0u) | (d > fe.td ? 8u : 0u);
  }
  u64 v = (u64)nib << (4 * (threadIdx.x & 15));
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v |= shfl_xor64(v, off);
  if ((threadIdx.x & 15) == 0 && f < m) {
    code[f / 16] = v;
    if (slot) slot[(size_t)(f / 16) * stride] = v;
  }
}

// the k smallest keys of the wave's 64, ascending, to dst[0 .. k) (lane 0 stores): k rounds of the wave-wide
// minimum with the winner retired.  Keys are unique but for kNone, which only ever fills what is left.
__device__ __forceinline__ void wave_top_k(u64 key, int k, u64 *dst, int lane) {
  for (int j = 0; j < k; ++j) {
    const u64 m = wave_min64(key);
    if (key == m) key = kNone;
    if (lane == 0) dst[j] = m;
  }
}

// Block (b, c) of kb x chunks: lane t holds keyframe 256 b + t, its W words in
// registers (WT >= W of them, the rest zero), and walks queries
// [c * chunk, + chunk), whose words sit in LDS, zero-padded to WT (a wave reads
// one address: a broadcast).  Per query each wave leaves its k smallest keys in
// LDS; then wave w merges the four lists of queries w, w + 4, ... and stores
// the block's k keys of that query to part[(query * kb + b) * k ..].
template <int WT>
__global__ __launch_bounds__(kSThreads) void k_fern_search(const u64 *__restrict__ codes, long long stride, int n, int W,
                                                           const u64 *__restrict__ queries, int q, int chunk, int kb,
                                                           int k, u64 *__restrict__ part) {
  __shared__ u64 s_q[kSearchMaxChunk * WT];
  __shared__ u64 s_top[kSearchMaxChunk * kSWaves * kSearchMaxK];
  const int b = blockIdx.x % kb, c = blockIdx.x / kb;
  const int q0 = c * chunk, nq = min(chunk, q - q0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int id = b * kSThreads + tid;
  const bool live = id < n;
  u64 reg[WT];
#pragma unroll
  for (int w = 0; w < WT; ++w) reg[w] = (live && w < W) ? codes[(size_t)w * stride + id] : 0ull;
  for (int i = tid; i < nq * WT; i += kSThreads) {
    const int qi = i / WT, w = i % WT;
    s_q[i] = w < W ? queries[(size_t)(q0 + qi) * W + w] : 0ull;
  }
  __syncthreads();
  for (int qi = 0; qi < nq; ++qi) {
    int d = 0;
#pragma unroll
    for (int w = 0; w < WT; ++w) {
      const u64 x = reg[w] ^ s_q[qi * WT + w];
      d += __popcll((x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x1111111111111111ull);
    }
    const u64 key = live ? (((u64)(unsigned)d << 32) | (unsigned)id) : kNone;
    wave_top_k(key, k, &s_top[(qi * kSWaves + wave) * kSearchMaxK], lane);
  }
  __syncthreads();
  for (int qi = wave; qi < nq; qi += kSWaves) {
    const int j = lane & (kSearchMaxK - 1);
    const u64 key = j < k ? s_top[(qi * kSWaves + (lane >> 4)) * kSearchMaxK + j] : kNone;
    wave_top_k(key, k, &part[((size_t)(q0 + qi) * kb + b) * k], lane);
  }
}

// One wave per query: the k smallest of its kb * k block keys, ascending.  Keys
// are unique, so round j takes the smallest key above round j - 1's winner and
// nothing has to be retired in memory.
__global__ __launch_bounds__(64) void k_fern_merge(const u64 *__restrict__ part, int kb, int k, u64 *__restrict__ out) {
  const u64 *p = part + (size_t)blockIdx.x * kb * k;
  const int total = kb * k, lane = threadIdx.x;
  u64 prev = 0;
  for (int j = 0; j < k; ++j) {
    u64 best = kNone;
    for (int i = lane; i < total; i += 64) {
      const u64 v = p[i];
      if ((j == 0 || v > prev) && v < best) best = v;
    }
    prev = wave_min64(best);
    if (lane == 0) out[(size_t)blockIdx.x * k + j] = prev;
  }
}

template <int WT>
void search_launch(hipStream_t s, int grid, const u64 *codes, long long stride, int n, int W, const u64 *queries, int q,
                   int chunk, int kb, int k, u64 *part) {
  hipLaunchKernelGGL((k_fern_search<WT>), dim3(grid), dim3(kSThreads), 0, s, codes, stride, n, W, queries, q, chunk, kb, k,
                     part);
}

}  // namespace

void launch_fern_encode(hipStream_t s, const void *table, int m, const uint8_t *bgr, int width, const float *dmap, int wL,
                        int sc, unsigned long long *code, unsigned long long *slot, long long stride) {
  hipLaunchKernelGGL(k_fern_encode, dim3((m + 63) / 64), dim3(64), 0, s, static_cast<const kfx_fern *>(table), m, bgr, width,
                     dmap, wL, sc, code, slot, stride);
}

void launch_fern_search(hipStream_t s, const unsigned long long *codes, long long stride, int n, int W,
                        const unsigned long long *queries, int q, int k, unsigned long long *part,
                        unsigned long long *out) {
  const int kb = (int)search_key_blocks(n);
  const int chunk = search_chunk_rule(n, q);
  const int grid = kb * ((q + chunk - 1) / chunk);
  // the register copy of a keyframe is W rounded up to a power of two
  if (W <= 1) search_launch<1>(s, grid, codes, stride, n, W, queries, q, chunk, kb, k, part);
  else if (W <= 2) search_launch<2>(s, grid, codes, stride, n, W, queries, q, chunk, kb, k, part);
  else if (W <= 4) search_launch<4>(s, grid, codes, stride, n, W, queries, q, chunk, kb, k, part);
  else if (W <= 8) search_launch<8>(s, grid, codes, stride, n, W, queries, q, chunk, kb, k, part);
  else if (W <= 16) search_launch<16>(s, grid, codes, stride, n, W, queries, q, chunk, kb, k, part);
  else if (W <= 32) search_launch<32>(s, grid, codes, stride, n, W, queries, q, chunk, kb, k, part);
  else search_launch<64>(s, grid, codes, stride, n, W, queries, q, chunk, kb, k, part);
  hipLaunchKernelGGL(k_fern_merge, dim3(q), dim3(64), 0, s, part, kb, k, out);
}

}  // namespace kfx
