// kfx_volume_io.hip — the volume in and out of the device: reference records,
// SoA planes, column gathers, the order-free checksum, and the occupancy maps'
// rebuild after an upload.
#include <algorithm>
#include <climits>

#include "kfx_device.h"

namespace kfx {
namespace {

// Reference 8-byte record {int16 tsdf, int16 weight, u8 c0,c1,c2, pad}
// (device_types.hpp:51-56), x-fastest linear order, for slices [z0, z0+nz).
__global__ void k_export_records(VolView v, int z0, int nz, uint64_t *dst) {
  const size_t n = v.slice * (size_t)nz;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % v.X);
    const int y = (int)((i / v.X) % v.Y);
    const int z = z0 + (int)(i / v.slice);
    const size_t s = vox_index(v, x, y, z);
    const uint64_t rec = (uint64_t)(uint16_t)v.tsdf[s] | ((uint64_t)(uint16_t)v.weight[s] << 16) |
                         ((uint64_t)(v.rgb[s] & 0xffffffu) << 32);
    dst[i] = rec;
  }
}

__global__ void k_import_records(VolView v, int z0, int nz, const uint64_t *src, unsigned *bad) {
  const size_t n = v.slice * (size_t)nz;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % v.X);
    const int y = (int)((i / v.X) % v.Y);
    const int z = z0 + (int)(i / v.slice);
    const size_t s = vox_index(v, x, y, z);
    const uint64_t rec = src[i];
    v.tsdf[s] = (int16_t)(rec & 0xffffu);
    const int w = (int16_t)((rec >> 16) & 0xffffu);
    if ((unsigned)w > 255u) *bad = 1u;  // not representable in the u8 weight store
    v.weight[s] = (uint8_t)w;
    v.rgb[s] = (uint32_t)((rec >> 32) & 0xffffffu);
  }
}

// Order-free volume checksum over the owned slices: sum of a 64-bit mix of
// (global x-fastest index, tsdf, weight, colour) per voxel, and the count of
// voxels with weight > 0 — slab sums add up to the single volume's.
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__global__ __launch_bounds__(256) void k_checksum(VolView v, unsigned long long *out) {
  const size_t n = v.local_voxels(), per_tile = v.tile_voxels();
  unsigned long long h = 0, cnt = 0;
  for (size_t li = (size_t)blockIdx.x * 256 + threadIdx.x; li < n; li += (size_t)gridDim.x * 256) {
    const size_t tile = li / per_tile, rem = li % per_tile;
    const int z = v.zb + (int)(rem >> 6), inner = (int)(rem & 63);
    if (z < v.own0 || z >= v.own1) continue;
    const int x = (int)(tile % v.tiles_x) * 8 + (inner & 7), y = (int)(tile / v.tiles_x) * 8 + (inner >> 3);
    const unsigned long long g = (unsigned long long)x + (unsigned long long)v.X * ((unsigned long long)y + (unsigned long long)v.Y * z);
    const unsigned long long rec = ((unsigned long long)(uint16_t)v.tsdf[li] << 48) |
                                   ((unsigned long long)(uint16_t)v.weight[li] << 32) | (v.rgb[li] & 0xffffffu);
    h += mix64(g * 0x9E3779B97F4A7C15ull ^ rec);
    cnt += v.weight[li] > 0;
  }
  for (int off = 32; off > 0; off >>= 1) {
    h += __shfl_xor(h, off);
    cnt += __shfl_xor(cnt, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&out[0], h);
    atomicAdd(&out[1], cnt);
  }
}

// Occupancy maps of the whole stored volume (after an upload; the maps were
// cleared): wave = one brick (column tile x 8 slices), lane = one column.
__global__ __launch_bounds__(256) void k_occ_rebuild(VolView v) {
  const int lane = threadIdx.x & 63;
  const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (size_t)v.tiles_x * v.tiles_y * v.nbz) return;
  const int tile = (int)(w / v.nbz), lb = (int)(w % v.nbz);
  const int z0 = max((v.bz0 + lb) * 8, v.zb), z1 = min((v.bz0 + lb) * 8 + 8, v.zb + v.zn);
  int lo = INT_MAX, hi = -1;
  for (int z = z0; z < z1; ++z)
    if (v.tsdf[(size_t)tile * v.tile_voxels() + (size_t)(z - v.zb) * 64 + lane] < 0) {
      lo = min(lo, z);
      hi = max(hi, z);
    }
  occ_mark_wave(v, tile, lo, hi, lane);
}

__global__ void k_gather_columns(VolView v, const int32_t *cols, int n, int16_t *t, int16_t *w, uint32_t *c) {
  const int nz = v.own1 - v.own0;
  const size_t total = (size_t)n * nz;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / nz), z = v.own0 + (int)(i % nz);
    const size_t s = vox_index(v, cols[2 * k], cols[2 * k + 1], z);
    if (t) t[i] = v.tsdf[s];
    if (w) w[i] = v.weight[s];
    if (c) c[i] = v.rgb[s];
  }
}

__global__ void k_export_soa(VolView v, int z0, int nz, int16_t *t, int16_t *w, uint32_t *c) {
  const size_t n = v.slice * (size_t)nz;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % v.X);
    const int y = (int)((i / v.X) % v.Y);
    const int z = z0 + (int)(i / v.slice);
    const size_t s = vox_index(v, x, y, z);
    if (t) t[i] = v.tsdf[s];
    if (w) w[i] = v.weight[s];
    if (c) c[i] = v.rgb[s];
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// Launchers

static dim3 slab_grid(const VolView &v, int nz) {
  const size_t n = v.slice * (size_t)nz;
  size_t b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  return dim3((unsigned)b);
}

void launch_export_records(hipStream_t s, VolView v, int z0, int nz, uint64_t *dst) {
  hipLaunchKernelGGL(k_export_records, slab_grid(v, nz), dim3(256), 0, s, v, z0, nz, dst);
}
void launch_import_records(hipStream_t s, VolView v, int z0, int nz, const uint64_t *src, unsigned *bad) {
  hipLaunchKernelGGL(k_import_records, slab_grid(v, nz), dim3(256), 0, s, v, z0, nz, src, bad);
}
void launch_checksum(hipStream_t s, VolView v, unsigned long long *out) {
  hipLaunchKernelGGL(k_checksum, dim3(2048), dim3(256), 0, s, v, out);
}

void launch_export_soa(hipStream_t s, VolView v, int z0, int nz, int16_t *t, int16_t *w,
                       uint32_t *c) {
  hipLaunchKernelGGL(k_export_soa, slab_grid(v, nz), dim3(256), 0, s, v, z0, nz, t, w, c);
}

void launch_gather_columns(hipStream_t s, VolView v, const int32_t *cols, int n, int16_t *t, int16_t *w,
                           uint32_t *c) {
  const size_t total = (size_t)n * (v.own1 - v.own0);
  const unsigned b = (unsigned)std::min<size_t>(8192, (total + 255) / 256);
  hipLaunchKernelGGL(k_gather_columns, dim3(std::max(1u, b)), dim3(256), 0, s, v, cols, n, t, w, c);
}

void launch_occ_rebuild(hipStream_t s, VolView v) {
  (void)hipMemsetAsync(v.bocc, 0, v.bocc_bytes(), s);
  (void)hipMemsetAsync(v.socc, 0, v.socc_bytes(), s);
  if (v.settled) {  // new contents: no brick is known settled, any may be (the gate opens)
    (void)hipMemsetAsync(v.settled, 0, v.settled_bytes(), s);
    (void)hipMemsetAsync(v.sgate, 0x40, 4, s);
  }
  const size_t waves = (size_t)v.tiles_x * v.tiles_y * v.nbz;
  hipLaunchKernelGGL(k_occ_rebuild, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, v);
}

}  // namespace kfx
