// kfx_extract.hip — point-cloud and marching-cubes extraction (one sweep
// kernel, pool copy, offset scans) and the rendered views of the model maps.
// Compiled like kfx_kernels.hip (-ffp-contract=off, the reference's evaluation
// order), so results are bit-identical to the CPU oracle.
#include <algorithm>

#include "kfx_extract_dev.h"
#include "kfx_scanws.h"

#ifndef KFX_XSWEEP_WAVES
#define KFX_XSWEEP_WAVES 65536  // extraction: units per wave grow (up to 64) while this many waves remain
#endif

namespace kfx {
namespace {

// ---------------------------------------------------------------------------
// Point-cloud extraction — FullScan6 (tsdf_volume.cu:307-481): for every voxel
// with W != 0 and F != 1 (A11: never 1), a zero crossing towards the +x, +y
// and +z neighbour (W != 0, F != 1, opposite signs) gives the point
// p = (V * |Fn| + Vn * |F|) / (|F| + |Fn|) along that edge, V the voxel
// centre ((i + 0.5) * vs), transformed by the volume pose (R * p + t).
//
// The reference appends points with warp atomics (nondeterministic order, a
// nondeterministic subset when the 10 M buffer fills).  Here the order is
// canonical (D): wave = one 8x8 column tile x kExtractZ slices; points are
// ordered by (slice chunk, tile, z, lane = (y&7)*8 + (x&7), edge x/y/z), so
// the output and its first `cap` points are deterministic.  Pass 1 counts
// per wave, a scan turns counts into offsets, pass 2 writes.
constexpr int kExtractZ = 8;

// The per-voxel functions (extract_voxel, vertex_attr, kVertexWords) live in
// kfx_extract_dev.h: the eviction kernels (kfx_shift.hip) share them.

// kEmit = false: counts[wave] = points of the wave; true: write them at
// offsets[wave] + rank (rank < cap only).  z in [zlo, zhi) (global slices,
// zhi <= Z - 1; a slab passes its owned range).
// Extraction waves own one tile x one 8-slice chunk (kExtractZ), i.e. one
// brick.  Every point needs a negative tsdf at the voxel or its +x/+y/+z
// neighbour, and every marching-cubes triangle a negative corner: all of them
// lie in the brick or a neighbouring one, so a clear (dilated) brick bit of
// the occupancy map proves the wave outputs nothing — it reads no voxel.
__device__ __forceinline__ bool brick_clear(const VolView &v, int tile, int c0) {
  const int lbz = (c0 >> 3) - v.bz0;
  if (lbz < 0 || lbz >= v.nbz) return false;
  return !((v.bocc[(size_t)tile * v.bw + (lbz >> 6)] >> (lbz & 63)) & 1ull);
}

// The brick sweeps of one wave (extract_wave, mesh_wave, mc_vertex) live in
// kfx_extract_dev.h too: the world extraction (kfx_world.hip) runs them on a
// staged brick.

// Extraction with ONE read of the volume (points or marching cubes).
// Pass A (k_extract_pool): each canonical wave counts its brick's items and,
// if it has any, reserves that many slots of a pool with one 64-bit atomic
// (high bits: the wave's entry in the list of non-empty waves, low bits: the
// pool offset) and writes its items there in its own canonical order (from
// the bricks it just read: cache hits).  The reserved slots are unordered
// across waves.  Then the offset scan of the per-wave counts (canonical
// order) and pass C (k_extract_copy): one wave per listed wave copies its
// items from the pool to their canonical position.  A pool too small for
// every item (the caller's cap) sets *overflow; the counts are still complete,
// and the host then runs the emit pass of the two-pass path instead.
constexpr int kPoolListShift = 40;
constexpr unsigned long long kPoolMask = (1ull << kPoolListShift) - 1ull;
enum XMode { kXCount = 0, kXEmit = 1, kXPool = 2 };
// The extraction passes.  A unit = one tile x one 8-slice chunk (the
// canonical order's (chunk, tile)); each wave sweeps 64 consecutive units of
// one chunk (K = 1..64, xsweep_units): lane l tests unit T0 + l's brick in
// the occupancy map, a clear brick's unit has no items (count 0, no voxel
// read), and the others are processed one after another by the whole wave
// (lane = column).  At 2048^3 (16.8 M units, mostly clear) a wave per unit
// is launch-bound (count pass 8.3 ms; 64 units per wave: 6.8 ms for count +
// pool emit); small volumes keep enough waves with a small K.
// kXCount: counts[unit]; kXEmit: items at offsets[unit] (first cap only);
// kXPool: counts[unit] and the items into the pool (above).
// kAttr (kXEmit / kXPool): attributed items, 7 words per point, 21 per
// triangle, in place of 3 / 9 floats (the count pass needs no attributes).
template <int kMode, bool kMesh, bool kAttr = false>
__global__ __launch_bounds__(256) void k_xsweep(VolView v, DevPose aff, int zlo, int zhi,
                                                const uint8_t *__restrict__ tab, unsigned *counts,
                                                const unsigned long long *offsets, float *out,
                                                unsigned long long cap, unsigned long long *ctr,
                                                unsigned long long *pool_at, unsigned *list, unsigned *overflow,
                                                int K) {
  const int lane = threadIdx.x & 63;
  const int ntiles = v.tiles_x * v.tiles_y;
  const int T0 = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)) * K;
  if (T0 >= ntiles) return;
  // chunks are aligned to global multiples of kExtractZ (slab boundaries are
  // too), so concatenating slabs in rank order reproduces the single volume
  const int c0 = (zlo / kExtractZ) * kExtractZ + (int)blockIdx.y * kExtractZ;
  const int z0 = max(zlo, c0), z1 = min(zhi, c0 + kExtractZ);
  static_assert(kExtractZ == 8, "one brick per unit");
  const size_t ubase = (size_t)blockIdx.y * ntiles;  // unit index = ubase + tile
  const int tl = T0 + lane;
  const bool mine = lane < K && tl < ntiles;
  const bool have = mine && !brick_clear(v, tl, c0);  // waves of clear bricks read nothing
  if (kMode != kXEmit && mine && !have) counts[ubase + tl] = 0u;
  unsigned long long work = __ballot(have);
  while (work) {  // wave-uniform
    const int t = __ffsll((long long)work) - 1;
    work &= work - 1ull;
    const int tile = T0 + t;
    const size_t unit = ubase + tile;
    const int x = (tile % v.tiles_x) * 8 + (lane & 7);
    const int y = (tile / v.tiles_x) * 8 + (lane >> 3);
    if (kMode == kXEmit) {
      if (kMesh)
        (void)mesh_wave<true, kAttr>(v, aff, tab, x, y, z0, z1, offsets[unit], out, cap);
      else
        (void)extract_wave<true, kAttr>(v, aff, x, y, z0, z1, offsets[unit], out, cap);
      continue;
    }
    const unsigned n = kMesh ? mesh_wave<false>(v, aff, tab, x, y, z0, z1, 0ull, out, 0ull)
                             : extract_wave<false>(v, aff, x, y, z0, z1, 0ull, out, 0ull);
    if (lane == 0) counts[unit] = n;
    if (kMode != kXPool || n == 0) continue;
    unsigned long long old = 0;
    if (lane == 0) old = atomicAdd(ctr, (1ull << kPoolListShift) | (unsigned long long)n);
    old = __shfl(old, 0);
    const unsigned long long base = old & kPoolMask;
    if (lane == 0) {
      list[old >> kPoolListShift] = (unsigned)unit;
      pool_at[unit] = base;
    }
    if (base + n > cap) {  // (cap = the pool's size here)
      if (lane == 0) atomicOr(overflow, 1u);
      continue;
    }
    // the items again from the brick just read (cache hits; staging them in
    // LDS during the count measured slower: occupancy)
    if (kMesh)
      (void)mesh_wave<true, kAttr>(v, aff, tab, x, y, z0, z1, base, out, cap);
    else
      (void)extract_wave<true, kAttr>(v, aff, x, y, z0, z1, base, out, cap);
  }
}
// Pass C: listed wave i's items from the pool to offsets[wave] (first cap
// items of the canonical order only); per = 32-bit words per item, copied as
// integers (an attributed item's colour word is no float).
__global__ __launch_bounds__(256) void k_extract_copy(const unsigned *__restrict__ list, unsigned nlist,
                                                      const unsigned *__restrict__ counts,
                                                      const unsigned long long *__restrict__ pool_at,
                                                      const unsigned long long *__restrict__ offsets,
                                                      const uint32_t *__restrict__ pool, uint32_t *out,
                                                      unsigned long long cap, int per) {
  const unsigned i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nlist) return;
  const int lane = threadIdx.x & 63;
  const unsigned w = list[i];
  const unsigned long long o = offsets[w];
  if (o >= cap) return;
  const unsigned long long n = min((unsigned long long)counts[w], cap - o);
  const uint32_t *src = pool + pool_at[w] * per;
  uint32_t *dst = out + o * per;
  for (unsigned long long k = lane; k < n * per; k += 64) dst[k] = src[k];
}

// Indexed mesh: the sweeps of k_xsweep over the chunks of ALL
// slices [0, Z) (the top slice owns the +x / +y edges cube z = Z - 2 uses), one
// unit numbering for both counted quantities.  A unit's vertices are the used
// edges its voxels own, its triangles those of its cubes (z < Z - 1).
//   kICount: vcounts[unit], tcounts[unit]
//   kIVerts: the vertices at voff[unit] + rank, their in-unit keys beside them
//   kITris:  3 indices per triangle at toff[unit] + rank, each looked up by key
//            among the vertices of the unit that owns the corner's edge
// A clear brick bit proves both counts 0: an owned edge has a negative end at
// the voxel or its + neighbour, which the dilated map covers as it does a
// cube's corners.
enum IMode { kICount = 0, kIVerts = 1, kITris = 2 };
struct WindowFind {
  const unsigned *__restrict__ vcounts;
  const unsigned long long *__restrict__ voff;
  const uint16_t *__restrict__ keys;
  int tiles_x, ntiles;
  __device__ __forceinline__ uint32_t operator()(int x, int y, int z, int a) const {
    const size_t u = (size_t)(z >> 3) * ntiles + (size_t)(y >> 3) * tiles_x + (x >> 3);
    return edge_find(keys, voff[u], vcounts[u], edge_key(x, y, z, a));
  }
};
template <int kMode>
__global__ __launch_bounds__(256) void k_isweep(VolView v, DevPose aff, const uint8_t *__restrict__ tab,
                                                unsigned *vcounts, unsigned *tcounts,
                                                const unsigned long long *voff, const unsigned long long *toff,
                                                uint32_t *verts, uint16_t *keys, uint32_t *tris, int K) {
  const int lane = threadIdx.x & 63;
  const int ntiles = v.tiles_x * v.tiles_y;
  const int T0 = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)) * K;
  if (T0 >= ntiles) return;
  const int c0 = (int)blockIdx.y * kExtractZ;
  const int zv = min(v.Z, c0 + kExtractZ), zt = min(v.Z - 1, c0 + kExtractZ);  // vertex / cube slices end here
  const size_t ubase = (size_t)blockIdx.y * ntiles;
  const int tl = T0 + lane;
  const bool mine = lane < K && tl < ntiles;
  const bool have = mine && !brick_clear(v, tl, c0);
  if (kMode == kICount && mine && !have) vcounts[ubase + tl] = tcounts[ubase + tl] = 0u;
  unsigned long long work = __ballot(have);
  while (work) {  // wave-uniform
    const int t = __ffsll((long long)work) - 1;
    work &= work - 1ull;
    const int tile = T0 + t;
    const size_t unit = ubase + tile;
    const int x = (tile % v.tiles_x) * 8 + (lane & 7);
    const int y = (tile / v.tiles_x) * 8 + (lane >> 3);
    if (kMode == kICount) {
      const unsigned nv = edge_wave<false>(v, aff, x, y, c0, zv, 0ull, verts, keys);
      const unsigned nt = mesh_wave<false>(v, aff, tab, x, y, c0, zt, 0ull, nullptr, 0ull);
      if (lane == 0) {
        vcounts[unit] = nv;
        tcounts[unit] = nt;
      }
    } else if (kMode == kIVerts) {
      if (vcounts[unit] != 0u) (void)edge_wave<true>(v, aff, x, y, c0, zv, voff[unit], verts, keys);
    } else if (tcounts[unit] != 0u) {
      const WindowFind find = {vcounts, voff, keys, v.tiles_x, ntiles};
      index_wave(v, tab, x, y, c0, zt, toff[unit], tris, find);
    }
  }
}

// Exclusive scan of n u32 counts into u64 offsets (one 1024-thread block per
// 4096 counts, then the block totals, then the fix-up); *total = the sum.
__global__ __launch_bounds__(1024) void k_scan_local(const unsigned *in, unsigned long long *out,
                                                     unsigned long long *bsum, size_t n) {
  __shared__ unsigned long long s[1024];
  const size_t b0 = (size_t)blockIdx.x * 4096 + threadIdx.x * 4;
  unsigned long long v[4], acc = 0;
  for (int k = 0; k < 4; ++k) {
    v[k] = (b0 + k < n) ? in[b0 + k] : 0ull;
    acc += v[k];
  }
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    const unsigned long long t = threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  unsigned long long run = s[threadIdx.x] - acc;
  for (int k = 0; k < 4; ++k) {
    if (b0 + k < n) out[b0 + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 1023) bsum[blockIdx.x] = s[1023];
}
__global__ __launch_bounds__(1024) void k_scan_blocks(unsigned long long *bsum, int nb,
                                                      unsigned long long *total) {
  // nb <= 1024 * 64: each thread scans a contiguous run, then one block scan
  __shared__ unsigned long long s[1024];
  const int per = (nb + 1023) / 1024;
  const int b0 = threadIdx.x * per;
  unsigned long long acc = 0;
  for (int k = 0; k < per; ++k)
    if (b0 + k < nb) acc += bsum[b0 + k];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const unsigned long long t = threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  unsigned long long run = s[threadIdx.x] - acc;
  for (int k = 0; k < per; ++k)
    if (b0 + k < nb) {
      const unsigned long long c = bsum[b0 + k];
      bsum[b0 + k] = run;
      run += c;
    }
  if (threadIdx.x == 1023) *total = s[1023];
}
__global__ void k_scan_add(unsigned long long *out, const unsigned long long *bsum, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] += bsum[i / 4096];
}

// kernel_renderNormals / kernel_renderPhong (image_process.cu:137-221) on the
// previous frame's level-0 maps, lit from the last pose's camera position
// (kinectfusion.cpp:33-47).  D as in the oracle (kfo_render): IEEE sqrt and
// division in __m_normalize, pow(h, 10) as h8 * h2, NaN → 0 in the uchar
// conversion (render_u8, normalized_ieee: kfx_device.h); `0.5*light_coffi`
// stays double as in the source.
__global__ __launch_bounds__(256) void k_render(const float *__restrict__ vmap, const float *__restrict__ nmap,
                                                int n, const DevState *st, const DevPose *log, int type,
                                                uint8_t *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const f3 nv = ld3(nmap, i), vv = ld3(vmap, i);
  uint8_t o[3] = {0, 0, 0};
  if (type == 1) {
    o[0] = render_u8(fabsf(nv.x) * 255);
    o[1] = render_u8(fabsf(nv.y) * 255);
    o[2] = render_u8(fabsf(nv.z) * 255);
  } else if (!(nv.x == 0 && nv.y == 0 && nv.z == 0) && !(vv.x == 0 && vv.y == 0 && vv.z == 0)) {
    const DevPose &P = log[st->n_poses - 1];
    const f3 kd = {0.3843f, 0.4745f, 0.580f};
    const float intensity = 0.9f;
    const f3 e = normalized_ieee(sub({P.t[0], P.t[1], P.t[2]}, vv));
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
    o[0] = render_u8((float)fmin(1.0, (double)(0.1f + diffuse.x) + spec) * 255);
    o[1] = render_u8((float)fmin(1.0, (double)(0.1f + diffuse.y) + spec) * 255);
    o[2] = render_u8((float)fmin(1.0, (double)(0.1f + diffuse.z) + spec) * 255);
  }
  out[3 * (size_t)i] = o[0];
  out[3 * (size_t)i + 1] = o[1];
  out[3 * (size_t)i + 2] = o[2];
}

}  // namespace

// ---------------------------------------------------------------------------
// Launchers

static int extract_chunks(int zlo, int zhi) {
  if (zhi <= zlo) return 0;
  const int a = (zlo / kExtractZ) * kExtractZ;
  return (zhi - a + kExtractZ - 1) / kExtractZ;
}
size_t extract_waves(const VolView &v, int zlo, int zhi) {
  return (size_t)v.tiles_x * v.tiles_y * (size_t)extract_chunks(zlo, zhi);
}
int xsweep_units(const VolView &v, int zlo, int zhi) {
  if (v.xunits) return v.xunits;  // kfx_debug_extract_units
  // units per wave: as many as keep >= 64 K waves (at least 1, at most 64)
  const size_t units = extract_waves(v, zlo, zhi);
  int K = 1;
  while (K < 64 && units / (size_t)(2 * K) >= (size_t)KFX_XSWEEP_WAVES) K *= 2;
  return K;
}
template <int kMode, bool kAttr = false>
static void launch_xsweep(hipStream_t s, const VolView &v, DevPose vpose, int zlo, int zhi, const uint8_t *tab,
                          unsigned *counts, const unsigned long long *offsets, float *out, unsigned long long cap,
                          unsigned long long *ctr, unsigned long long *pool_at, unsigned *list, unsigned *overflow) {
  const int nc = extract_chunks(zlo, zhi);
  if (nc == 0) return;
  const int tiles = v.tiles_x * v.tiles_y;
  const int K = xsweep_units(v, zlo, zhi);
  dim3 grd((tiles + 4 * K - 1) / (4 * K), nc);  // 4 waves of K units per block
  if (tab)
    hipLaunchKernelGGL((k_xsweep<kMode, true, kAttr>), grd, dim3(256), 0, s, v, vpose, zlo, zhi, tab, counts, offsets,
                       out, cap, ctr, pool_at, list, overflow, K);
  else
    hipLaunchKernelGGL((k_xsweep<kMode, false, kAttr>), grd, dim3(256), 0, s, v, vpose, zlo, zhi, tab, counts, offsets,
                       out, cap, ctr, pool_at, list, overflow, K);
}
void launch_extract(hipStream_t s, const VolView &v, DevPose vpose, int zlo, int zhi,
                    unsigned *counts, const unsigned long long *offsets, float *out,
                    unsigned long long cap, bool attr) {
  if (offsets && attr)
    launch_xsweep<kXEmit, true>(s, v, vpose, zlo, zhi, nullptr, counts, offsets, out, cap, nullptr, nullptr, nullptr,
                                nullptr);
  else if (offsets)
    launch_xsweep<kXEmit>(s, v, vpose, zlo, zhi, nullptr, counts, offsets, out, cap, nullptr, nullptr, nullptr, nullptr);
  else
    launch_xsweep<kXCount>(s, v, vpose, zlo, zhi, nullptr, counts, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
}
void launch_mesh(hipStream_t s, const VolView &v, DevPose vpose, int zlo, int zhi, const uint8_t *tab,
                 unsigned *counts, const unsigned long long *offsets, float *out, unsigned long long cap,
                 bool attr) {
  if (offsets && attr)
    launch_xsweep<kXEmit, true>(s, v, vpose, zlo, zhi, tab, counts, offsets, out, cap, nullptr, nullptr, nullptr,
                                nullptr);
  else if (offsets)
    launch_xsweep<kXEmit>(s, v, vpose, zlo, zhi, tab, counts, offsets, out, cap, nullptr, nullptr, nullptr, nullptr);
  else
    launch_xsweep<kXCount>(s, v, vpose, zlo, zhi, tab, counts, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
}
void launch_extract_pool(hipStream_t s, const VolView &v, DevPose vpose, int zlo, int zhi, const uint8_t *tab,
                         unsigned *counts, unsigned long long *ctr, unsigned long long *pool_at, unsigned *list,
                         float *pool, unsigned long long pool_cap, unsigned *overflow, bool attr) {
  if (attr)
    launch_xsweep<kXPool, true>(s, v, vpose, zlo, zhi, tab, counts, nullptr, pool, pool_cap, ctr, pool_at, list,
                                overflow);
  else
    launch_xsweep<kXPool>(s, v, vpose, zlo, zhi, tab, counts, nullptr, pool, pool_cap, ctr, pool_at, list, overflow);
}
void launch_extract_copy(hipStream_t s, const unsigned *list, unsigned nlist, const unsigned *counts,
                         const unsigned long long *pool_at, const unsigned long long *offsets, const float *pool,
                         float *out, unsigned long long cap, int per) {
  if (nlist == 0) return;
  hipLaunchKernelGGL(k_extract_copy, dim3((nlist + 3) / 4), dim3(256), 0, s, list, nlist, counts, pool_at, offsets,
                     reinterpret_cast<const uint32_t *>(pool), reinterpret_cast<uint32_t *>(out), cap, per);
}
size_t indexed_units(const VolView &v) { return extract_waves(v, 0, v.Z); }
void launch_indexed(hipStream_t s, const VolView &v, DevPose vpose, const uint8_t *tab, int pass, unsigned *vcounts,
                    unsigned *tcounts, const unsigned long long *voff, const unsigned long long *toff, void *verts,
                    uint16_t *keys, uint32_t *tris) {
  const int nc = extract_chunks(0, v.Z);
  if (nc == 0) return;
  const int tiles = v.tiles_x * v.tiles_y;
  const int K = xsweep_units(v, 0, v.Z);
  const dim3 grd((tiles + 4 * K - 1) / (4 * K), nc), blk(256);
  uint32_t *vw = static_cast<uint32_t *>(verts);
  if (pass == kICount)
    hipLaunchKernelGGL((k_isweep<kICount>), grd, blk, 0, s, v, vpose, tab, vcounts, tcounts, voff, toff, vw, keys, tris, K);
  else if (pass == kIVerts)
    hipLaunchKernelGGL((k_isweep<kIVerts>), grd, blk, 0, s, v, vpose, tab, vcounts, tcounts, voff, toff, vw, keys, tris, K);
  else
    hipLaunchKernelGGL((k_isweep<kITris>), grd, blk, 0, s, v, vpose, tab, vcounts, tcounts, voff, toff, vw, keys, tris, K);
}
void launch_scan(hipStream_t s, const unsigned *counts, unsigned long long *offsets,
                 unsigned long long *bsum, size_t n, unsigned long long *total) {
  const size_t nb = scan_blocks(n);
  hipLaunchKernelGGL(k_scan_local, dim3((unsigned)nb), dim3(1024), 0, s, counts, offsets, bsum, n);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, bsum, (int)nb, total);
  hipLaunchKernelGGL(k_scan_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, offsets, bsum, n);
}

void launch_render(hipStream_t s, const float *vmap, const float *nmap, int n, const DevState *st,
                   const DevPose *log, int type, uint8_t *out) {
  hipLaunchKernelGGL(k_render, dim3((n + 255) / 256), dim3(256), 0, s, vmap, nmap, n, st, log, type, out);
}

}  // namespace kfx
