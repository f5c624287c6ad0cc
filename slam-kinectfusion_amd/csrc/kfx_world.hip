// kfx_world.hip — the world map: attributed points and
// marching-cubes triangles from a sparse, sorted list of kfx_brick records
// (what the window holds merged with what the moving volume streamed out).
// The per-voxel work is kfx_extract_dev.h's, the dense extraction's own code,
// run on a brick and its halo staged in LDS.  Compiled like kfx_extract.hip
// (-ffp-contract=off), so an item has kfx_extract_*_attr's bytes wherever the
// two see the same voxels.
#include "kfx_extract_dev.h"

namespace kfx {
namespace {

constexpr int kBrickPieces = 225;  // a kfx_brick as 16-byte pieces: header, 64 tsdf, 32 weight, 128 colour
constexpr int kCoordBias = 1 << 20;  // |b_k| < 2^20: b_k + bias fills 21 bits

// ---------------------------------------------------------------------------
// Neighbour table.  The list ascends in (b[2], b[1], b[0]), so the 63-bit key
//   (b2 + 2^20) << 42 | (b1 + 2^20) << 21 | (b0 + 2^20)
// ascends with it and each of a brick's 27 neighbours is one binary search.
__device__ __forceinline__ unsigned long long world_key(int b0, int b1, int b2) {
  return ((unsigned long long)(unsigned)(b2 + kCoordBias) << 42) | ((unsigned long long)(unsigned)(b1 + kCoordBias) << 21) |
         (unsigned long long)(unsigned)(b0 + kCoordBias);
}

__global__ __launch_bounds__(256) void k_world_keys(const uint4 *__restrict__ recs, long long n,
                                                    unsigned long long *__restrict__ keys) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint4 h = recs[(size_t)i * kBrickPieces];
  keys[i] = world_key((int)h.x, (int)h.y, (int)h.z);
}

// neigh[i][slot], slot = ((oz + 1) * 3 + (oy + 1)) * 3 + (ox + 1): the list index
// of brick b_i + o, -1 where the list has none
__global__ __launch_bounds__(256) void k_world_neigh(const unsigned long long *__restrict__ keys, long long n,
                                                     int32_t *__restrict__ neigh) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * 27) return;
  const long long i = e / 27;
  const int slot = (int)(e % 27);
  if (slot == 13) {
    neigh[e] = (int32_t)i;
    return;
  }
  const unsigned long long k = keys[i];
  const int b0 = (int)(k & 0x1fffffu) - kCoordBias + slot % 3 - 1;
  const int b1 = (int)((k >> 21) & 0x1fffffu) - kCoordBias + (slot / 3) % 3 - 1;
  const int b2 = (int)(k >> 42) - kCoordBias + slot / 9 - 1;
  int32_t found = -1;
  if (abs(b0) < kCoordBias && abs(b1) < kCoordBias && abs(b2) < kCoordBias) {  // (else no brick may have it)
    const unsigned long long want = world_key(b0, b1, b2);
    long long lo = 0, hi = n;  // first index with keys[index] >= want
    while (lo < hi) {
      const long long mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    if (lo < n && keys[lo] == want) found = (int32_t)lo;
  }
  neigh[e] = found;
}

// ---------------------------------------------------------------------------
// The staged tile: a brick's 8^3 voxels and the halo its items read.  A cube
// corner lies at local 0..8 and its gradient reaches one further, so local
// -1 .. 9 per axis: 11^3 voxels x (2 + 1 + 4) bytes = 9317 B of LDS.  A voxel
// of a brick the list does not hold is unobserved: 0, 0, 0.
constexpr int kTile = 11, kTileVox = kTile * kTile * kTile;

struct WorldTile {
  const int16_t *tsdf;   // LDS
  const uint8_t *weight;
  const uint32_t *rgb;
  int w0[3];             // world index of local voxel 0: 8 b_k
  float vs[3];
};
__device__ __forceinline__ int vw_index(const WorldTile &, int x, int y, int z) {
  return ((z + 1) * kTile + (y + 1)) * kTile + (x + 1);
}
__device__ __forceinline__ int vw_weight(const WorldTile &v, int i) { return v.weight[i]; }
__device__ __forceinline__ int vw_tsdf(const WorldTile &v, int i) { return v.tsdf[i]; }
__device__ __forceinline__ uint32_t vw_rgb(const WorldTile &v, int i) { return v.rgb[i]; }
// no volume faces: every neighbour an item reads is in the tile, valid iff its weight != 0
__device__ __forceinline__ bool vw_above(const WorldTile &, int, int) { return true; }
__device__ __forceinline__ bool vw_below(const WorldTile &, int, int) { return true; }
__device__ __forceinline__ float vw_coord(const WorldTile &v, int k, int q) { return (float)(v.w0[k] + q); }

struct WorldGeom {
  float vs[3];
};

// Gather: the tile is 121 (z, y) rows of 11 voxels, and a row crosses three
// bricks: 1 voxel of the -x neighbour, 8 of the middle one, 2 of the +x one.
// A lane takes one (row, brick) unit at a time and reads that brick's whole x
// row with 16-byte loads where the record allows it (16 B of tsdf, 8 of weight,
// 32 of colour), as k_brick_restore reads a record, then stores the voxels the
// tile keeps.  Returns whether the tile holds a negative tsdf (wave-uniform).
__device__ __forceinline__ bool world_gather(const uint4 *__restrict__ recs, const int32_t *__restrict__ nb,
                                             int16_t *lt, uint8_t *lw, uint32_t *lc) {
  const int lane = threadIdx.x & 63;
  bool neg = false;
  for (int u = lane; u < kTile * kTile * 3; u += 64) {
    const int row = u / 3, sx = u % 3;
    const int tz = row / kTile, ty = row % kTile;
    const int sz = tz == 0 ? 0 : (tz >= 9 ? 2 : 1), sy = ty == 0 ? 0 : (ty >= 9 ? 2 : 1);
    const int dz = (tz + 7) & 7, dy = (ty + 7) & 7;  // local -1 -> 7, 8 -> 0, 9 -> 1
    const int32_t r = nb[(sz * 3 + sy) * 3 + sx];
    union {
      uint4 q;
      int16_t s[8];
    } T;
    union {
      uint2 q;
      uint8_t b[8];
    } W;
    union {
      uint4 q[2];
      uint32_t c[8];
    } Cc;
    T.q = make_uint4(0u, 0u, 0u, 0u);
    W.q = make_uint2(0u, 0u);
    Cc.q[0] = Cc.q[1] = T.q;
    if (r >= 0) {
      const uint4 *rec = recs + (size_t)r * kBrickPieces;  // (64-bit: n * 225 pieces passes 2^31)
      const int xr = 8 * dz + dy;                          // the x row's number inside the brick
      T.q = rec[1 + xr];
      W.q = reinterpret_cast<const uint2 *>(rec + 65)[xr];
      Cc.q[0] = rec[97 + 2 * xr];
      Cc.q[1] = rec[98 + 2 * xr];
    }
    // voxels [j0, j1) of the row go to tile x = t0 + (j - j0)
    const int j0 = sx == 0 ? 7 : 0, j1 = sx == 2 ? 2 : 8, t0 = sx == 0 ? 0 : (sx == 1 ? 1 : 9);
    const int at = (tz * kTile + ty) * kTile + t0 - j0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j >= j0 && j < j1) {
        lt[at + j] = T.s[j];
        lw[at + j] = W.b[j];
        lc[at + j] = Cc.c[j];
        neg = neg || T.s[j] < 0;
      }
  }
  return __any(neg);
}

// One block = one wave = one brick.  kEmit = false: counts[brick] = its items
// (0 without a read of more than the tile when no tsdf in it is negative:
// every point needs a negative end, every triangle a negative corner);
// true: the items at offsets[brick] + rank (rank < cap only), 7 words per
// vertex.  Order inside the brick: dz, lane = 8 dy + dx, edge axis / triangle.
template <bool kEmit, bool kMesh>
__global__ __launch_bounds__(64) void k_world_sweep(const uint4 *__restrict__ recs, const int32_t *__restrict__ neigh,
                                                    DevPose aff, WorldGeom g, const uint8_t *__restrict__ tab,
                                                    unsigned *counts, const unsigned long long *__restrict__ offsets,
                                                    float *out, unsigned long long cap) {
  __shared__ int16_t lt[kTileVox + 1];
  __shared__ uint32_t lc[kTileVox];
  __shared__ uint8_t lw[kTileVox + 1];
  const size_t brick = blockIdx.x;
  unsigned long long base = 0;
  if (kEmit) {  // (block-uniform)
    if (counts[brick] == 0u) return;
    base = offsets[brick];
    if (base >= cap) return;
  }
  const int lane = threadIdx.x & 63;
  const bool neg = world_gather(recs, neigh + brick * 27, lt, lw, lc);
  if (!kEmit && !neg) {
    if (lane == 0) counts[brick] = 0u;
    return;
  }
  __syncthreads();
  const uint4 h = recs[brick * kBrickPieces];
  WorldTile v;
  v.tsdf = lt, v.weight = lw, v.rgb = lc;
  v.w0[0] = 8 * (int)h.x, v.w0[1] = 8 * (int)h.y, v.w0[2] = 8 * (int)h.z;
  for (int k = 0; k < 3; ++k) v.vs[k] = g.vs[k];
  const int x = lane & 7, y = lane >> 3;
  const unsigned n = kMesh ? mesh_wave<kEmit, true>(v, aff, tab, x, y, 0, 8, base, out, cap)
                           : extract_wave<kEmit, true>(v, aff, x, y, 0, 8, base, out, cap);
  if (!kEmit && lane == 0) counts[brick] = n;
}

// Indexed mesh, one block = one wave = one brick as above.
// pass 0: vcounts[brick] = the used edges its voxels own, tcounts[brick] = its
// triangles (both 0 without more than the gather when the tile holds nothing
// negative: a used edge has a negative end at local 0..8); pass 1: the vertices
// at voff[brick] + rank and their keys; pass 2: 3 indices per triangle at
// toff[brick] + rank.  A corner's owner voxel lies at local 0..8 per axis: in
// this brick or, through the neighbour table, one of its 7 + neighbours.
struct WorldFind {
  const int32_t *__restrict__ nb;  // the brick's 27 table entries
  const unsigned *__restrict__ vcounts;
  const unsigned long long *__restrict__ voff;
  const uint16_t *__restrict__ keys;
  __device__ __forceinline__ uint32_t operator()(int x, int y, int z, int a) const {
    const int32_t r = nb[(((z >> 3) + 1) * 3 + (y >> 3) + 1) * 3 + (x >> 3) + 1];
    if (r < 0) return 0xffffffffu;
    return edge_find(keys, voff[r], vcounts[r], edge_key(x, y, z, a));
  }
};
template <int kPass>
__global__ __launch_bounds__(64) void k_world_isweep(const uint4 *__restrict__ recs, const int32_t *__restrict__ neigh,
                                                     DevPose aff, WorldGeom g, const uint8_t *__restrict__ tab,
                                                     unsigned *vcounts, unsigned *tcounts,
                                                     const unsigned long long *__restrict__ voff,
                                                     const unsigned long long *__restrict__ toff, uint32_t *verts,
                                                     uint16_t *keys, uint32_t *tris) {
  __shared__ int16_t lt[kTileVox + 1];
  __shared__ uint32_t lc[kTileVox];
  __shared__ uint8_t lw[kTileVox + 1];
  const size_t brick = blockIdx.x;
  if (kPass == 1 && vcounts[brick] == 0u) return;  // (block-uniform)
  if (kPass == 2 && tcounts[brick] == 0u) return;
  const int lane = threadIdx.x & 63;
  const bool neg = world_gather(recs, neigh + brick * 27, lt, lw, lc);
  if (kPass == 0 && !neg) {
    if (lane == 0) vcounts[brick] = tcounts[brick] = 0u;
    return;
  }
  __syncthreads();
  const uint4 h = recs[brick * kBrickPieces];
  WorldTile v;
  v.tsdf = lt, v.weight = lw, v.rgb = lc;
  v.w0[0] = 8 * (int)h.x, v.w0[1] = 8 * (int)h.y, v.w0[2] = 8 * (int)h.z;
  for (int k = 0; k < 3; ++k) v.vs[k] = g.vs[k];
  const int x = lane & 7, y = lane >> 3;
  if (kPass == 0) {
    const unsigned nv = edge_wave<false>(v, aff, x, y, 0, 8, 0ull, verts, keys);
    const unsigned nt = mesh_wave<false, true>(v, aff, tab, x, y, 0, 8, 0ull, nullptr, 0ull);
    if (lane == 0) {
      vcounts[brick] = nv;
      tcounts[brick] = nt;
    }
  } else if (kPass == 1) {
    (void)edge_wave<true>(v, aff, x, y, 0, 8, voff[brick], verts, keys);
  } else {
    const WorldFind find = {neigh + brick * 27, vcounts, voff, keys};
    index_wave(v, tab, x, y, 0, 8, toff[brick], tris, find);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// Launchers

void launch_world_neigh(hipStream_t s, const void *recs, size_t n, unsigned long long *keys, int32_t *neigh) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_world_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, static_cast<const uint4 *>(recs),
                     (long long)n, keys);
  hipLaunchKernelGGL(k_world_neigh, dim3((unsigned)((n * 27 + 255) / 256)), dim3(256), 0, s, keys, (long long)n, neigh);
}

void launch_world_sweep(hipStream_t s, const void *recs, size_t n, const int32_t *neigh, DevPose pose0,
                        const float vs[3], const uint8_t *tab, unsigned *counts, const unsigned long long *offsets,
                        float *out, unsigned long long cap) {
  if (n == 0) return;
  WorldGeom g;
  for (int k = 0; k < 3; ++k) g.vs[k] = vs[k];
  const uint4 *r = static_cast<const uint4 *>(recs);
  const dim3 grd((unsigned)n), blk(64);
  if (offsets && tab)
    hipLaunchKernelGGL((k_world_sweep<true, true>), grd, blk, 0, s, r, neigh, pose0, g, tab, counts, offsets, out, cap);
  else if (offsets)
    hipLaunchKernelGGL((k_world_sweep<true, false>), grd, blk, 0, s, r, neigh, pose0, g, tab, counts, offsets, out, cap);
  else if (tab)
    hipLaunchKernelGGL((k_world_sweep<false, true>), grd, blk, 0, s, r, neigh, pose0, g, tab, counts, offsets, out, 0ull);
  else
    hipLaunchKernelGGL((k_world_sweep<false, false>), grd, blk, 0, s, r, neigh, pose0, g, tab, counts, offsets, out, 0ull);
}

void launch_world_indexed(hipStream_t s, const void *recs, size_t n, const int32_t *neigh, DevPose pose0,
                          const float vs[3], const uint8_t *tab, int pass, unsigned *vcounts, unsigned *tcounts,
                          const unsigned long long *voff, const unsigned long long *toff, void *verts, uint16_t *keys,
                          uint32_t *tris) {
  if (n == 0) return;
  WorldGeom g;
  for (int k = 0; k < 3; ++k) g.vs[k] = vs[k];
  const uint4 *r = static_cast<const uint4 *>(recs);
  uint32_t *vw = static_cast<uint32_t *>(verts);
  const dim3 grd((unsigned)n), blk(64);
  if (pass == 0)
    hipLaunchKernelGGL((k_world_isweep<0>), grd, blk, 0, s, r, neigh, pose0, g, tab, vcounts, tcounts, voff, toff, vw, keys, tris);
  else if (pass == 1)
    hipLaunchKernelGGL((k_world_isweep<1>), grd, blk, 0, s, r, neigh, pose0, g, tab, vcounts, tcounts, voff, toff, vw, keys, tris);
  else
    hipLaunchKernelGGL((k_world_isweep<2>), grd, blk, 0, s, r, neigh, pose0, g, tab, vcounts, tcounts, voff, toff, vw, keys, tris);
}

}  // namespace kfx
