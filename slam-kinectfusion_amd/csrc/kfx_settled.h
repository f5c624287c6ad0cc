// Free-space certificate of one brick for integrate's settled-brick skip
// (DESIGN.md §15).
//
// A brick is one 8x8 column tile by 8 global slices (z >> 3).  Its settled
// byte says that every voxel holds weight 64 and a tsdf that a ts = 1 update
// reproduces.  Such a brick needs no work in a frame in which every voxel is
// either not updated at all (behind the camera, off the image, on a pixel
// without depth) or updated with ts = 1 outside the colour band: both leave
// the stored values as they are.  brick_certified proves the second half from
// the frame's pose and its 16x16-pixel min-depth grid alone:
//
//   * The brick's 8 corners under the linear model vc0 + z zs all have
//     pz >= pzmin.  The projection u = fx x / z + cx is linear-fractional, so
//     over the convex brick it takes its extremes at the corners; with 2.5
//     pixels of margin (2 for the drift of the accumulated vc, as int_column /
//     int_tile_clip, 0.5 for the rounding) the box covers the pixel of every
//     voxel of the brick that projects into the image.  pzmin = 0.1 voxel *
//     focal length keeps that drift (< 0.1 voxel) below one pixel.
//   * Dmin = the least positive depth of the grid cells under the box bounds
//     the depth d of each such pixel from below (+inf: none has depth).
//   * For an in-image voxel il |vc| <= vc.z (1 + delta) (il = 1 / lambda of
//     its pixel; far_clip_factor below), and vc.z <= pzmax + 2 voxels (the
//     linear model's largest corner plus the drift margin), so
//       sdf = d - il |vc| >= Dmin - (1 + delta) (pzmax + 2 vs).
//     Certified when Dmin >= (pzmax + 2 vs + trunc) * far_k + 0.01 (the far
//     clip's form; far_k >= 1.02 and far_k >= 1.001 (1 + delta)): then
//     sdf >= 1.02 trunc + 0.01, so tq = RN(sdf / trunc) >= 1 and
//     sdf > trunc / 2 with a margin far above the few ulps of the device's
//     sdf arithmetic.  (far_k = +inf, a camera too coarse for any bound,
//     certifies only a brick none of whose pixels has depth.)
// Any NaN makes a comparison false: not certified.  Host and device share
// this text (tests/settled/settled_check.cpp).
#pragma once
#include <cmath>

#include "kfx_ffadd.h"

namespace kfx {

// How far |vc| / lambda can lie from vc.z, and the factor integrate's far
// clips (int_column, int_tile_clip) and the certificate below derive from it.
//
// A voxel at vc (vc.z > 0) is tested against the pixel (u, v) its projection
// rounds to, with lambda = |p|, p = ((u - cx) / fx, (v - cy) / fy, 1), while
// |vc| = vc.z |r| with r = (vc.x / vc.z, vc.y / vc.z, 1) its own ray.  Rounding
// moves the projection by at most half a pixel per axis, so
// |r - p| <= delta = hypot(1 / fx, 1 / fy) / 2, hence ||r| - |p|| <= delta, and
// with |p| >= 1
//     |vc| / lambda = vc.z |r| / |p|  lies in  vc.z [1 - delta, 1 + delta]
// for every voxel whose pixel is in the image (the same at every pixel: the
// bound does not depend on cx, cy or the image size).
//
// A voxel is updated only when d - |vc| / lambda >= -trunc, d its pixel's
// depth: with D >= d that needs vc.z (1 - delta) <= D + trunc.  No voxel with
//     vc.z > (D + trunc) * far_k,   far_k = max(1.02, 1.001 / (1 - delta)),
// is updated (the clips add 0.01 m on top).  1.001 leaves a thousand times the
// rounding of the float evaluation of sdf; 1.02 is the value every camera with
// fx, fy >= 38 px keeps (delta <= 0.0187), among them every benchmark camera.
// Below that the half pixel is worth more than 2 %: at fx = fy = 9.6 px the
// factor is 1.0806.  For delta >= 0.5 (fx, fy of about 1.4 px and less) no
// bound of this kind holds: +inf, which switches the far clips and the
// certificate off.  A launch-time constant of the level-0 intrinsics
// (VolView::far_k), not loop code.
KFX_HD inline float far_clip_delta(float fx, float fy) {
  return 0.5f * std::sqrt(1.f / (fx * fx) + 1.f / (fy * fy));
}
KFX_HD inline float far_clip_factor(float fx, float fy) {
  const float delta = far_clip_delta(fx, fy);
  if (!(delta < 0.5f)) return INFINITY;  // (NaN too)
  const float k = 1.001f / (1.f - delta);
  return k > 1.02f ? k : 1.02f;
}

constexpr int kSettledMaxCells = 36;  // a larger pixel box: not certified

// dmin: the min-depth grid (float bits, +inf bits for a cell without depth),
// nbx cells per row; (x0, y0, z0) the brick's first voxel; far_k =
// far_clip_factor of the level-0 intrinsics
KFX_HD inline bool brick_certified(const float *R, const float *t, float vs0, float vs1, float fx, float fy, float cx,
                                   float cy, int w, int h, int x0, int y0, int z0, float trunc, const unsigned *dmin,
                                   int nbx, float far_k) {
  const float zsx = R[2] * vs0, zsy = R[5] * vs0, zsz = R[8] * vs0;
  const float pzmin = 0.1f * vs0 * (fx > fy ? fx : fy);
  float umin = 0.f, umax = 0.f, vmin = 0.f, vmax = 0.f, pzmax = 0.f;
  bool good = pzmin >= 1e-3f;
  for (int k = 0; k < 8; ++k) {
    const float vx = (float)(x0 + ((k & 1) ? 7 : 0)) * vs0, vy = (float)(y0 + ((k & 2) ? 7 : 0)) * vs1;
    const float z = (float)(z0 + ((k & 4) ? 7 : 0));
    const float px = (R[0] * vx + R[1] * vy + t[0]) + z * zsx;
    const float py = (R[3] * vx + R[4] * vy + t[1]) + z * zsy;
    const float pz = (R[6] * vx + R[7] * vy + t[2]) + z * zsz;
    good = good && pz >= pzmin;
    const float u = fx * (px / pz) + cx, v = fy * (py / pz) + cy;
    if (k == 0) {
      umin = umax = u;
      vmin = vmax = v;
      pzmax = pz;
    } else {
      umin = u < umin ? u : umin;
      umax = u > umax ? u : umax;
      vmin = v < vmin ? v : vmin;
      vmax = v > vmax ? v : vmax;
      pzmax = pz > pzmax ? pz : pzmax;
    }
    good = good && u == u && v == v;  // NaN
  }
  if (!good) return false;
  const float fu0 = umin - 2.5f > 0.f ? umin - 2.5f : 0.f, fu1 = umax + 2.5f < (float)(w - 1) ? umax + 2.5f : (float)(w - 1);
  const float fv0 = vmin - 2.5f > 0.f ? vmin - 2.5f : 0.f, fv1 = vmax + 2.5f < (float)(h - 1) ? vmax + 2.5f : (float)(h - 1);
  if (!(fu0 <= fu1) || !(fv0 <= fv1)) return false;  // off the image (the frustum clip's business)
  const int cx0 = (int)fu0 >> 4, cx1 = (int)fu1 >> 4, cy0 = (int)fv0 >> 4, cy1 = (int)fv1 >> 4;
  if ((cx1 - cx0 + 1) * (cy1 - cy0 + 1) > kSettledMaxCells) return false;
  unsigned dm = 0x7f800000u;  // +inf
  for (int y = cy0; y <= cy1; ++y)
    for (int x = cx0; x <= cx1; ++x) {
      const unsigned c = dmin[y * nbx + x];
      dm = c < dm ? c : dm;  // positive floats order as their bits
    }
  float Dmin;
  std::memcpy(&Dmin, &dm, 4);
  const float need = (pzmax + 2.f * vs0 + trunc) * far_k + 0.01f;
  return Dmin >= need;
}

// The same with far_k derived here from the focal lengths (callers that hold
// no launch constant: host checks).
KFX_HD inline bool brick_certified(const float *R, const float *t, float vs0, float vs1, float fx, float fy, float cx,
                                   float cy, int w, int h, int x0, int y0, int z0, float trunc, const unsigned *dmin,
                                   int nbx) {
  return brick_certified(R, t, vs0, vs1, fx, fy, cx, cy, w, h, x0, y0, z0, trunc, dmin, nbx,
                         far_clip_factor(fx, fy));
}

}  // namespace kfx
