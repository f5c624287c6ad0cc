/*
 * kfx_ref_shim.h — TEST INFRASTRUCTURE ONLY.
 *
 * Just enough of the CUDA runtime surface for the reference's per-thread
 * kernels (tsdfhelper, raycasthelper, the image kernels, ICP::findCoresp) to
 * compile as host C++ with g++ (oracle/Makefile, target `ref`).  Written from
 * the CUDA API's names; it holds no reference text.
 *
 * A kernel launch k<<<grid, block>>>(args) is rewritten by the Makefile into
 * KFX_REF_LAUNCH(k, grid, block)(args): a loop over grid x block that sets
 * blockIdx / threadIdx and calls the kernel once per thread, one after another.
 * That is exact for kernels whose threads neither share memory nor talk to
 * each other, which is all the parity tests call.
 *
 * Intrinsic mapping ("div/sqrt: IEEE results, no
 * contraction"; the build passes -ffp-contract=off -fno-fast-math):
 *
 *   __fdividef(a, b)      a / b
 *   __fsqrt_rn(a)         sqrtf(a)
 *   __fmaf_rn(a, b, c)    fmaf(a, b, c)
 *   __float2int_rn(a)     nearbyintf(a) (ties to even), saturating, NaN -> 0
 *   __float2int_rd(a)     floorf(a), saturating, NaN -> 0
 *   __int2float_rn(a)     (float)a
 *   __int_as_float(a)     memcpy of the 4 bytes
 *
 * __syncthreads, the warp votes, the atomics and asm() only compile: nothing
 * the tests call reaches them (FullScan6 and the ICP block reduction are out of
 * scope: they are warp- and block-synchronous).
 */
#ifndef KFX_REF_SHIM_H
#define KFX_REF_SHIM_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __inline__ inline
#define __shared__ static
#define asm(...) ret = 0 /* PTX lane-id reads: compile only */

typedef unsigned char uchar;
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct uchar3 { unsigned char x, y, z; };
struct uint3 { unsigned x, y, z; };
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
inline float2 make_float2(float a, float b) { return {a, b}; }
inline float3 make_float3(float a, float b, float c) { return {a, b, c}; }
inline int2 make_int2(int a, int b) { return {a, b}; }
inline int3 make_int3(int a, int b, int c) { return {a, b, c}; }
inline uchar3 make_uchar3(unsigned char a, unsigned char b, unsigned char c) { return {a, b, c}; }

inline uint3 threadIdx, blockIdx;
inline dim3 blockDim, gridDim;

namespace kfx_ref_shim {
template <class F>
struct Launch {
  dim3 g, b;
  F f;
  template <class... A>
  void operator()(A... a) const {
    gridDim = g;
    blockDim = b;
    for (unsigned bz = 0; bz < g.z; ++bz)
      for (unsigned by = 0; by < g.y; ++by)
        for (unsigned bx = 0; bx < g.x; ++bx)
          for (unsigned tz = 0; tz < b.z; ++tz)
            for (unsigned ty = 0; ty < b.y; ++ty)
              for (unsigned tx = 0; tx < b.x; ++tx) {
                blockIdx = {bx, by, bz};
                threadIdx = {tx, ty, tz};
                f(a...);
              }
  }
};
template <class F>
Launch<F> launch(dim3 g, dim3 b, F f) {
  return Launch<F>{g, b, f};
}
inline int sat_int(float r) {
  if (r != r) return 0;
  if (r >= 2147483648.f) return INT_MAX;
  if (r <= -2147483648.f) return INT_MIN;
  return (int)r;
}
}  // namespace kfx_ref_shim
#define KFX_REF_LAUNCH(k, g, b) kfx_ref_shim::launch(dim3(g), dim3(b), [&](auto... a) { k(a...); })

inline float __fdividef(float a, float b) { return a / b; }
inline float __fsqrt_rn(float a) { return sqrtf(a); }
inline float __fmaf_rn(float a, float b, float c) { return fmaf(a, b, c); }
inline int __float2int_rn(float a) { return kfx_ref_shim::sat_int(nearbyintf(a)); }
inline int __float2int_rd(float a) { return kfx_ref_shim::sat_int(floorf(a)); }
inline float __int2float_rn(int a) { return (float)a; }
inline float __int_as_float(int a) {
  float f;
  memcpy(&f, &a, 4);
  return f;
}
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
using std::isnan;

/* compile-only stand-ins */
inline void __syncthreads() {}
inline unsigned __activemask() { return 1; }
inline int __all_sync(unsigned, int p) { return p; }
inline unsigned __ballot_sync(unsigned, int p) { return p ? 1u : 0u; }
inline int __popc(unsigned v) { return __builtin_popcount(v); }
inline int atomicAdd(int *p, int v) {
  int o = *p;
  *p += v;
  return o;
}
inline unsigned atomicInc(unsigned *p, unsigned v) {
  unsigned o = *p;
  *p = o >= v ? 0 : o + 1;
  return o;
}

typedef int cudaError_t;
enum { cudaSuccess = 0, cudaMemcpyDeviceToHost = 2 };
inline cudaError_t cudaGetLastError() { return 0; }
inline cudaError_t cudaDeviceSynchronize() { return 0; }
inline cudaError_t cudaThreadSynchronize() { return 0; }
inline const char *cudaGetErrorString(cudaError_t) { return ""; }
inline cudaError_t cudaMalloc(void **p, size_t n) {
  *p = calloc(1, n);
  return 0;
}
inline cudaError_t cudaMallocPitch(void **p, size_t *pitch, size_t w, size_t h) {
  *pitch = w;
  *p = calloc(h, w);
  return 0;
}
inline cudaError_t cudaFree(void *p) {
  free(p);
  return 0;
}
inline cudaError_t cudaMemcpy(void *d, const void *s, size_t n, int) {
  memcpy(d, s, n);
  return 0;
}
template <class T>
cudaError_t cudaMemcpyFromSymbol(void *d, const T &s, size_t n) {
  memcpy(d, &s, n);
  return 0;
}

#endif
