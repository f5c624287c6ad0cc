/*
 * TEST INFRASTRUCTURE ONLY: the few OpenCV types the reference's headers and
 * per-thread kernels name (cv::cuda::PtrStep / PtrStepSz / PtrSz / GpuMat over
 * caller memory, Vec, Matx, Affine3f), written from OpenCV's public API.
 * Nothing allocates: a GpuMat here is a view the driver fills in.
 */
#pragma once
#include <cstddef>
#include <vector>

#define CV_32FC1 5
#define CV_8UC3 16
#define CV_32FC3 21

namespace cv {
template <class T, int N>
struct Vec {
  T v[N]{};
  T &operator()(int i) { return v[i]; }
  const T &operator()(int i) const { return v[i]; }
};
typedef Vec<float, 3> Vec3f;
typedef Vec<int, 3> Vec3i;
typedef Vec<double, 6> Vec6d;

template <class T, int M, int N>
struct Matx {
  T val[M * N]{};
  T &operator()(int i, int j) { return val[i * N + j]; }
  const T &operator()(int i, int j) const { return val[i * N + j]; }
};
typedef Matx<float, 3, 3> Matx33f;
typedef Matx<double, 6, 6> Matx66d;

struct Affine3f {
  Matx33f R;
  Vec3f t;
  Matx33f rotation() const { return R; }
  Vec3f translation() const { return t; }
};

namespace cuda {
template <class T>
struct PtrSz {
  T *data;
  size_t size;
};
template <class T>
struct PtrStep {
  T *data;
  size_t step; /* bytes per row */
  T &operator()(int y, int x) const { return *(T *)((char *)data + y * step + x * sizeof(T)); }
};
template <class T>
struct PtrStepSz : PtrStep<T> {
  int cols, rows;
};
struct GpuMat {
  int rows = 0, cols = 0;
  size_t step = 0;
  void *data = nullptr;
  template <class T>
  operator PtrStepSz<T>() const {
    PtrStepSz<T> p;
    p.data = (T *)data;
    p.step = step;
    p.cols = cols;
    p.rows = rows;
    return p;
  }
  template <class T>
  operator PtrStep<T>() const {
    return PtrStep<T>{(T *)data, step};
  }
  void setTo(int) {}
  void release() {}
};
inline GpuMat createContinuous(int, int, int) { return GpuMat(); }
}  // namespace cuda
}  // namespace cv
