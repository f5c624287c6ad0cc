// kfx_shift.hip — the moving volume: the in-place shift of the
// TSDF window by whole bricks, the extraction of the surface points the
// shift would drop (eviction), and the bricks themselves handed out and taken
// back.  Compiled like kfx_extract.hip
// (-ffp-contract=off), whose per-voxel functions the eviction shares
// (kfx_extract_dev.h), so an evicted item has kfx_extract_points_attr's bytes.
#include <algorithm>
#include <climits>
#include <cstdlib>

#include "kfx_extract_dev.h"

namespace kfx {
namespace {

// ---------------------------------------------------------------------------
// A region of bricks (cells: column tile x 8-slice group) that is the union of
// one slab per axis: per axis k the brick indices [a[k], b[k]) (empty: a = b =
// 0).  Its cells are numbered without a list, in the extraction's canonical
// order (z group, tile row, tile): a group inside the z range holds every tile
// (T cells), any other the tile rows of the y range whole and the x range of
// the other rows (P cells).
struct BrickRegion {
  int a[3], b[3];
  int s[3];                // the shift (voxels)
  int nX;                  // b[0] - a[0]
  unsigned long long P, T;
  unsigned long long total;
};

__device__ __forceinline__ void region_cell(const VolView &v, const BrickRegion &rg, unsigned long long un, int *cz,
                                            int *tile) {
  const unsigned long long lo = (unsigned long long)rg.a[2] * rg.P,
                           mid = (unsigned long long)(rg.b[2] - rg.a[2]) * rg.T;
  unsigned long long r;
  if (un < lo) {  // (P > 0 here; likewise nX > 0 wherever it divides below)
    *cz = (int)(un / rg.P);
    r = un % rg.P;
  } else if (un < lo + mid) {
    *cz = rg.a[2] + (int)((un - lo) / rg.T);
    *tile = (int)((un - lo) % rg.T);
    return;
  } else {
    *cz = rg.b[2] + (int)((un - lo - mid) / rg.P);
    r = (un - lo - mid) % rg.P;
  }
  const unsigned long long rlo = (unsigned long long)rg.a[1] * rg.nX,
                           rmid = (unsigned long long)(rg.b[1] - rg.a[1]) * v.tiles_x;
  int tx, ty;
  if (r < rlo) {
    ty = (int)(r / rg.nX);
    tx = rg.a[0] + (int)(r % rg.nX);
  } else if (r < rlo + rmid) {
    ty = rg.a[1] + (int)((r - rlo) / v.tiles_x);
    tx = (int)((r - rlo) % v.tiles_x);
  } else {
    ty = rg.b[1] + (int)((r - rlo - rmid) / rg.nX);
    tx = rg.a[0] + (int)((r - rlo - rmid) % rg.nX);
  }
  *tile = ty * v.tiles_x + tx;
}

// The slab of axis k: the bricks within |s_k| / 8 of the face the shift moves
// away from (s_k > 0: the low face), plus `touch` more layers on a high face.
BrickRegion make_region(const VolView &v, const int s[3], int touch) {
  BrickRegion rg{};
  const int nb[3] = {v.tiles_x, v.tiles_y, (v.Z + 7) / 8};
  for (int k = 0; k < 3; ++k) {
    rg.s[k] = s[k];
    const int d = s[k] / 8;  // bricks
    if (d > 0) {
      rg.a[k] = 0;
      rg.b[k] = std::min(nb[k], d);
    } else if (d < 0) {
      rg.a[k] = std::max(0, nb[k] + d - touch);
      rg.b[k] = nb[k];
    }
  }
  rg.nX = rg.b[0] - rg.a[0];
  const unsigned long long nY = (unsigned long long)(rg.b[1] - rg.a[1]);
  rg.T = (unsigned long long)v.tiles_x * v.tiles_y;
  rg.P = nY * v.tiles_x + ((unsigned long long)v.tiles_y - nY) * rg.nX;
  const unsigned long long nZ = (unsigned long long)(rg.b[2] - rg.a[2]);
  rg.total = nZ * rg.T + ((unsigned long long)nb[2] - nZ) * rg.P;
  return rg;
}

// ---------------------------------------------------------------------------
// Shift.  With every component a multiple of 8, brick c = (tile x, tile y, z
// group) takes the brick c + d, d = s / 8, whole: 1024 B of tsdf, 512 B of
// weight and 2048 B of colour, each contiguous (VolView: tile-column layout),
// = 64 + 32 + 128 lanes of 16 bytes, one per thread of the block (threads
// 224..255 only keep the barriers).  A brick without a source becomes 0.
//
// In place, in one launch: the bricks fall into chains c, c + d, c + 2d, ...,
// and a brick is read only as the source of its predecessor in its own chain.
// One block owns a chain and walks it from its head (the brick whose
// predecessor c - d lies outside the volume: the slab of |d_k| brick layers at
// the face the shift moves away from, per axis — a BrickRegion) in the shift's
// direction, 4 bricks per round: every thread loads its piece of the sources
// c + d .. c + 4d, waits for them, the block synchronises, then it stores the
// bricks c .. c + 3d and goes on at c + 4d.  A round's stores land on bricks
// this or an earlier round loaded (all loads of a round have returned before
// its barrier) and never on a brick still to be loaded (those lie ahead);
// no other block touches the chain.
//
// The first wave holds the tsdf of the brick it stores, so it marks the
// occupancy maps (cleared by the launcher) as k_occ_rebuild would, without
// another read of the volume.
struct ShiftPlan {
  BrickRegion heads;
  int d[3];  // the shift in bricks
};

template <typename I>
__global__ __launch_bounds__(256) void k_shift(VolView v, ShiftPlan pl) {
  int cz = 0, tile = 0;
  region_cell(v, pl.heads, blockIdx.x, &cz, &tile);
  int cx = tile % v.tiles_x, cy = tile / v.tiles_x;
  const int groups = (v.zn + 7) >> 3;
  const int t = (int)threadIdx.x;
  uint4 *base = nullptr;  // the thread's array, as 16-byte pieces
  int ps = 1, u = 0;      // pieces per slice, the thread's piece of a brick
  if (t < 64) {
    base = reinterpret_cast<uint4 *>(v.tsdf), ps = 8, u = t;
  } else if (t < 96) {
    base = reinterpret_cast<uint4 *>(v.weight), ps = 4, u = t - 64;
  } else if (t < 224) {
    base = reinterpret_cast<uint4 *>(v.rgb), ps = 16, u = t - 96;
  }
  const int du = u / ps;  // the piece's slice inside the brick
  auto inside = [&](int x, int y, int z) {
    return x >= 0 && x < v.tiles_x && y >= 0 && y < v.tiles_y && z >= 0 && z < groups;
  };
  auto piece = [&](int x, int y, int z) {  // (a volume's last group may be short: the caller checks the slice)
    return ((I)(y * v.tiles_x + x) * (I)v.zn + (I)(8 * z)) * (I)ps + (I)u;
  };
  while (inside(cx, cy, cz)) {  // (block-uniform)
    uint4 r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r[j] = make_uint4(0u, 0u, 0u, 0u);
      const int x = cx + j * pl.d[0], y = cy + j * pl.d[1], z = cz + j * pl.d[2];
      const int sx = x + pl.d[0], sy = y + pl.d[1], sz = z + pl.d[2];
      if (base && inside(x, y, z) && inside(sx, sy, sz) && 8 * sz + du < v.zn) r[j] = base[piece(sx, sy, sz)];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's loads have returned ...
    __syncthreads();                                   // ... and so have every thread's
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = cx + j * pl.d[0], y = cy + j * pl.d[1], z = cz + j * pl.d[2];
      if (!inside(x, y, z)) break;  // (block-uniform; the chain has left the volume)
      if (base && 8 * z + du < v.zn) base[piece(x, y, z)] = r[j];
      if (t < 64) {  // the brick's tsdf: slices with a negative value
        const bool neg = ((r[j].x | r[j].y | r[j].z | r[j].w) & 0x80008000u) != 0u;
        const int zq = v.zb + 8 * z + du;
        if (__any(neg)) occ_mark_wave(v, y * v.tiles_x + x, neg ? zq : INT_MAX, neg ? zq : -1, t);  // (most bricks: none)
      }
    }
    cx += 4 * pl.d[0], cy += 4 * pl.d[1], cz += 4 * pl.d[2];
  }
}

// ---------------------------------------------------------------------------
// Eviction.  A unit is one brick, as in the extraction sweep.  Only the bricks
// that hold a leaving voxel, or a kept voxel whose +x, +y or +z neighbour
// leaves (the layer below a slab that leaves at a high face), can own an
// evicted item: the shift's head region with one more layer at the high
// faces.  Count, scan and emit run over that region alone.

// voxel (x, y, z) is dropped by the shift: not 0 <= v_k - s_k < dims_k
__device__ __forceinline__ bool leaves(const VolView &v, const BrickRegion &rg, int x, int y, int z) {
  const int qx = x - rg.s[0], qy = y - rg.s[1], qz = z - rg.s[2];
  return qx < 0 || qx >= v.X || qy < 0 || qy >= v.Y || qz < 0 || qz >= v.Z;
}

// extract_wave (kfx_extract.hip) over the items whose edge has a leaving end:
// a subset in the same order.  kEmit = false: counts[unit]; true: the items
// at offsets[unit] + rank (rank < cap only), 7 words each.
template <bool kEmit>
__global__ __launch_bounds__(256) void k_evict(VolView v, DevPose aff, BrickRegion rg, unsigned *counts,
                                               const unsigned long long *offsets, uint32_t *out,
                                               unsigned long long cap) {
  const unsigned long long un = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (un >= rg.total) return;
  const int lane = threadIdx.x & 63;
  int cz = 0, tile = 0;
  region_cell(v, rg, un, &cz, &tile);
  const int x = (tile % v.tiles_x) * 8 + (lane & 7), y = (tile / v.tiles_x) * 8 + (lane >> 3);
  const int z0 = cz * 8, z1 = min(v.Z - 1, z0 + 8);  // FullScan6 reads z + 1
  unsigned long long base = kEmit ? offsets[un] : 0ull;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned total = 0;
  for (int z = z0; z < z1; ++z) {
    f3 pts[3];
    int axes = 0;
    const int n = extract_voxel<true>(v, aff, x, y, z, pts, &axes);
    const bool aout = leaves(v, rg, x, y, z);
    int keep = 0, m = 0;  // bit l: point l is evicted
#pragma unroll
    for (int l = 0; l < 3; ++l)
      if (l < n) {
        const int ax = (axes >> (2 * l)) & 3;
        if (aout || leaves(v, rg, x + (ax == 0), y + (ax == 1), z + (ax == 2))) {
          keep |= 1 << l;
          ++m;
        }
      }
    const unsigned long long b1 = __ballot(m >= 1), b2 = __ballot(m >= 2), b3 = __ballot(m >= 3);
    if (kEmit) {
      unsigned long long r = base + (unsigned long long)(__popcll(b1 & below) + __popcll(b2 & below) +
                                                         __popcll(b3 & below));
#pragma unroll
      for (int l = 0; l < 3; ++l)
        if (l < n && ((keep >> l) & 1)) {
          if (r < cap) {
            uint32_t *dst = out + (size_t)r * kVertexWords;
            st_vertex(dst, pts[l]);
            vertex_attr(v, aff, x, y, z, (axes >> (2 * l)) & 3, dst + 3);
          }
          ++r;
        }
    }
    const unsigned wt = (unsigned)(__popcll(b1) + __popcll(b2) + __popcll(b3));
    base += wt;
    total += wt;
  }
  if (!kEmit && lane == 0) counts[un] = total;
}

// ---------------------------------------------------------------------------
// Bricks out and back in.  A kfx_brick record is 225 pieces of
// 16 bytes: the header {b0, b1, b2, 0}, then the brick's three runs as the
// volume stores them, 64 pieces of tsdf, 32 of weight, 128 of colour (k_shift's
// thread order).  The records lie in hipMalloc'ed buffers, 3600 = 225 * 16
// bytes apart, so every access is a 16-byte vector access.
constexpr int kBrickPieces = 225;

struct BrickOrigin {
  int o[3];  // the window's origin in bricks
};

// The bricks with a voxel the shift drops, one slab per axis.  Where every
// dimension is a multiple of 8 this is make_region(v, s, 0); a short last group
// (8 nb > dim) makes the slab at the high face start one brick earlier: voxel x
// leaves iff x >= dim + s, so the first brick with such a voxel is (dim + s) / 8.
BrickRegion make_drop_region(const VolView &v, const int s[3]) {
  BrickRegion rg = make_region(v, s, 0);
  const int dims[3] = {v.X, v.Y, v.Z};
  for (int k = 0; k < 3; ++k)
    if (s[k] < 0) rg.a[k] = dims[k] + s[k] <= 0 ? 0 : (dims[k] + s[k]) / 8;
  rg.nX = rg.b[0] - rg.a[0];
  const unsigned long long nY = (unsigned long long)(rg.b[1] - rg.a[1]);
  rg.P = nY * v.tiles_x + ((unsigned long long)v.tiles_y - nY) * rg.nX;
  const unsigned long long nZ = (unsigned long long)(rg.b[2] - rg.a[2]);
  rg.total = nZ * rg.T + ((unsigned long long)((v.Z + 7) / 8) - nZ) * rg.P;
  return rg;
}

__device__ __forceinline__ bool nonzero(const uint4 &r) { return (r.x | r.y | r.z | r.w) != 0u; }

// Count: one wave per cell of the region, counts[cell] = 1 iff some stored byte
// of the brick is not 0.  The 512 B of weight first (a brick that was ever
// integrated shows there), the tsdf and the colour only while all is 0.
template <typename I>
__global__ __launch_bounds__(256) void k_brick_count(VolView v, BrickRegion rg, unsigned *counts) {
  const unsigned long long un = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (un >= rg.total) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  int cz = 0, tile = 0;
  region_cell(v, rg, un, &cz, &tile);
  const int nsl = min(8, v.zn - 8 * cz);                // slices the group holds (a last group may be short)
  const I col = (I)tile * (I)v.zn + (I)(8 * cz);        // slices stored in front of the brick
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  uint4 r = zero;
  if (lane < 4 * nsl) r = reinterpret_cast<const uint4 *>(v.weight)[col * (I)4 + (I)lane];
  unsigned long long any = __ballot(nonzero(r));
  if (!any) {
    r = zero;
    if (lane < 8 * nsl) r = reinterpret_cast<const uint4 *>(v.tsdf)[col * (I)8 + (I)lane];
    any = __ballot(nonzero(r));
  }
  if (!any) {
    uint4 q = zero;
    r = zero;
    if (lane < 16 * nsl) r = reinterpret_cast<const uint4 *>(v.rgb)[col * (I)16 + (I)lane];
    if (lane + 64 < 16 * nsl) q = reinterpret_cast<const uint4 *>(v.rgb)[col * (I)16 + (I)(lane + 64)];
    any = __ballot(nonzero(r) || nonzero(q));
  }
  if (lane == 0) counts[un] = any ? 1u : 0u;
}

// the thread's array (as 16-byte pieces), pieces per slice and piece of a
// brick: k_shift's assignment of threads 0..223
__device__ __forceinline__ uint4 *brick_piece(const VolView &v, int t, int *ps, int *u) {
  if (t < 64) {
    *ps = 8, *u = t;
    return reinterpret_cast<uint4 *>(v.tsdf);
  }
  if (t < 96) {
    *ps = 4, *u = t - 64;
    return reinterpret_cast<uint4 *>(v.weight);
  }
  *ps = 16, *u = t - 96;
  return reinterpret_cast<uint4 *>(v.rgb);
}

// Emit: one block per cell; the non-empty brick of rank offsets[cell] < cap is
// written as record `rank`: thread t < 224 its piece (0 for a slice past the
// volume's end), thread 224 the header.
template <typename I>
__global__ __launch_bounds__(256) void k_brick_emit(VolView v, BrickRegion rg, BrickOrigin ob, const unsigned *counts,
                                                    const unsigned long long *offsets, uint4 *out,
                                                    unsigned long long cap) {
  const unsigned long long un = blockIdx.x;
  if (!counts[un]) return;  // (block-uniform, as the next)
  const unsigned long long at = offsets[un];
  if (at >= cap) return;
  int cz = 0, tile = 0;
  region_cell(v, rg, un, &cz, &tile);
  uint4 *rec = out + (size_t)at * kBrickPieces;
  const int t = (int)threadIdx.x;
  if (t < 224) {
    int ps, u;
    const uint4 *base = brick_piece(v, t, &ps, &u);
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (8 * cz + u / ps < v.zn) r = base[((I)tile * (I)v.zn + (I)(8 * cz)) * (I)ps + (I)u];
    rec[1 + t] = r;
  } else if (t == 224) {
    rec[0] = make_uint4((unsigned)(ob.o[0] + tile % v.tiles_x), (unsigned)(ob.o[1] + tile / v.tiles_x),
                        (unsigned)(ob.o[2] + cz), 0u);
  }
}

// Restore: one block per input record.  A brick outside the window is skipped
// (block-uniform); otherwise thread t < 224 stores its piece over the brick at
// c = b - origin / 8 (the host has refused two records for one brick), and the
// first wave, which holds the tsdf, marks the occupancy maps as k_shift does.
template <typename I>
__global__ __launch_bounds__(256) void k_brick_restore(VolView v, BrickOrigin ob, const uint4 *in) {
  const uint4 *rec = in + (size_t)blockIdx.x * kBrickPieces;
  const uint4 h = rec[0];
  // (mod 2^32: |origin / 8| < 2^28, so a coordinate outside the window cannot wrap into it)
  const unsigned cx = h.x - (unsigned)ob.o[0], cy = h.y - (unsigned)ob.o[1], cz = h.z - (unsigned)ob.o[2];
  if (cx >= (unsigned)v.tiles_x || cy >= (unsigned)v.tiles_y || cz >= (unsigned)((v.zn + 7) >> 3)) return;
  const int t = (int)threadIdx.x;
  if (t >= 224) return;  // (no barrier below)
  const int tile = (int)cy * v.tiles_x + (int)cx;
  int ps, u;
  uint4 *base = brick_piece(v, t, &ps, &u);
  const int du = u / ps;
  const bool stored = 8 * (int)cz + du < v.zn;  // a slice past the volume's end is ignored
  const uint4 r = stored ? rec[1 + t] : make_uint4(0u, 0u, 0u, 0u);
  if (stored) base[((I)tile * (I)v.zn + (I)(8 * (int)cz)) * (I)ps + (I)u] = r;
  if (t < 64) {  // the brick's tsdf: slices with a negative value
    const bool neg = ((r.x | r.y | r.z | r.w) & 0x80008000u) != 0u;
    const int zq = v.zb + 8 * (int)cz + du;
    if (__any(neg)) occ_mark_wave(v, tile, neg ? zq : INT_MAX, neg ? zq : -1, t);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// Launchers

void launch_shift(hipStream_t s, const VolView &v, const int shift[3]) {
  if (!shift[0] && !shift[1] && !shift[2]) return;
  // the maps as launch_occ_rebuild leaves them for the new contents: cleared
  // and re-marked (by the shift's first waves), no settled byte, the gate open
  (void)hipMemsetAsync(v.bocc, 0, v.bocc_bytes(), s);
  (void)hipMemsetAsync(v.socc, 0, v.socc_bytes(), s);
  if (v.settled) {
    (void)hipMemsetAsync(v.settled, 0, v.settled_bytes(), s);
    (void)hipMemsetAsync(v.sgate, 0x40, 4, s);
  }
  const int dims[3] = {v.X, v.Y, v.Z};
  bool all = false;  // a component as long as its dimension: nothing stays
  for (int k = 0; k < 3; ++k) all = all || std::abs(shift[k]) >= dims[k];
  if (all) {
    const size_t n = v.local_voxels();
    (void)hipMemsetAsync(v.tsdf, 0, n * sizeof(int16_t), s);
    (void)hipMemsetAsync(v.weight, 0, n * sizeof(uint8_t), s);
    (void)hipMemsetAsync(v.rgb, 0, n * sizeof(uint32_t), s);
    return;
  }
  ShiftPlan pl;
  pl.heads = make_region(v, shift, 0);
  for (int k = 0; k < 3; ++k) pl.d[k] = shift[k] / 8;
  const dim3 grd((unsigned)pl.heads.total);
  if (v.force64 || v.local_voxels() >= ((size_t)1 << 31))
    hipLaunchKernelGGL((k_shift<unsigned long long>), grd, dim3(256), 0, s, v, pl);
  else
    hipLaunchKernelGGL((k_shift<unsigned>), grd, dim3(256), 0, s, v, pl);
}

size_t evict_units(const VolView &v, const int shift[3]) { return (size_t)make_region(v, shift, 1).total; }

void launch_evict(hipStream_t s, const VolView &v, DevPose vpose, const int shift[3], unsigned *counts,
                  const unsigned long long *offsets, float *out, unsigned long long cap) {
  const BrickRegion rg = make_region(v, shift, 1);
  if (rg.total == 0) return;
  const dim3 grd((unsigned)((rg.total + 3) / 4));
  if (offsets)
    hipLaunchKernelGGL(k_evict<true>, grd, dim3(256), 0, s, v, vpose, rg, counts, offsets,
                       reinterpret_cast<uint32_t *>(out), cap);
  else
    hipLaunchKernelGGL(k_evict<false>, grd, dim3(256), 0, s, v, vpose, rg, counts, offsets,
                       reinterpret_cast<uint32_t *>(out), cap);
}

static bool index64(const VolView &v) { return v.force64 || v.local_voxels() >= ((size_t)1 << 31); }
static BrickOrigin brick_origin(const int origin[3]) { return {{origin[0] / 8, origin[1] / 8, origin[2] / 8}}; }

size_t brick_evict_units(const VolView &v, const int shift[3]) { return (size_t)make_drop_region(v, shift).total; }

void launch_brick_count(hipStream_t s, const VolView &v, const int shift[3], unsigned *counts) {
  const BrickRegion rg = make_drop_region(v, shift);
  if (rg.total == 0) return;
  const dim3 grd((unsigned)((rg.total + 3) / 4));
  if (index64(v))
    hipLaunchKernelGGL((k_brick_count<unsigned long long>), grd, dim3(256), 0, s, v, rg, counts);
  else
    hipLaunchKernelGGL((k_brick_count<unsigned>), grd, dim3(256), 0, s, v, rg, counts);
}

void launch_brick_emit(hipStream_t s, const VolView &v, const int shift[3], const int origin[3],
                       const unsigned *counts, const unsigned long long *offsets, void *out,
                       unsigned long long cap) {
  const BrickRegion rg = make_drop_region(v, shift);
  if (rg.total == 0) return;
  const dim3 grd((unsigned)rg.total);
  if (index64(v))
    hipLaunchKernelGGL((k_brick_emit<unsigned long long>), grd, dim3(256), 0, s, v, rg, brick_origin(origin), counts,
                       offsets, static_cast<uint4 *>(out), cap);
  else
    hipLaunchKernelGGL((k_brick_emit<unsigned>), grd, dim3(256), 0, s, v, rg, brick_origin(origin), counts, offsets,
                       static_cast<uint4 *>(out), cap);
}

void launch_brick_restore(hipStream_t s, const VolView &v, const int origin[3], const void *in, size_t n) {
  if (n == 0) return;
  // new contents under whatever byte was set: as the upload and the shift, no
  // settled byte and the gate open; the occupancy maps only gain bits
  if (v.settled) {
    (void)hipMemsetAsync(v.settled, 0, v.settled_bytes(), s);
    (void)hipMemsetAsync(v.sgate, 0x40, 4, s);
  }
  const dim3 grd((unsigned)n);
  if (index64(v))
    hipLaunchKernelGGL((k_brick_restore<unsigned long long>), grd, dim3(256), 0, s, v, brick_origin(origin),
                       static_cast<const uint4 *>(in));
  else
    hipLaunchKernelGGL((k_brick_restore<unsigned>), grd, dim3(256), 0, s, v, brick_origin(origin),
                       static_cast<const uint4 *>(in));
}

}  // namespace kfx
