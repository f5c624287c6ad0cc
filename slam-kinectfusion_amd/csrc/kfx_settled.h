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
//
// brick_hidden proves the first half for a whole brick, whatever it stores
// (DESIGN.md §17): no voxel of the brick is updated, so the brick needs
// neither loads nor stores nor occupancy marks, and its settled byte (a
// property of what it stores) stays as it is.  From the pose and the
// 16x16-pixel max-depth grid alone:
//
//   * Corners and pixel box as above (the same pzmin, the same 2.5 px margin,
//     the same cap of kSettledMaxCells cells); a box off the image is not
//     certified, the frustum clip owns it.
//   * Dmax = the largest cell of the max-depth grid under the box (a cell
//     without depth reads 0) bounds from above the depth d of every pixel a
//     voxel of the brick can round to.
//   * A voxel is updated only if d > 0 and d - il |vc| >= -trunc.  For an
//     in-image voxel il |vc| >= vc.z (1 - delta), and vc.z >= pznear - 2 vs
//     (the linear model's nearest corner minus the drift margin).
//   * Certified when pznear - 2 vs > (Dmax + trunc) * hid_k, hid_k = 1.001 /
//     (1 - delta) (hidden_clip_factor): then il |vc| > 1.001 (d + trunc), so
//     sdf < -trunc - 0.001 (d + trunc), a thousand times the rounding of the
//     float evaluation of sdf (as for far_clip_factor).  Dmax = 0: no pixel
//     under the box has depth, nothing can be updated, certified.  hid_k =
//     +inf (delta >= 0.5) certifies nothing.
// Any NaN compares false: not certified (tests/hidden/hidden_check.cpp).
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

// The hidden certificate's factor: 1.001 / (1 - delta), without far_clip_factor's
// 1.02 floor (at 2.3 m the 2 % is more than a brick at 4 mm voxels).  +inf from
// delta >= 0.5 on (NaN too), which switches brick_hidden off.
KFX_HD inline float hidden_clip_factor(float fx, float fy) {
  const float delta = far_clip_delta(fx, fy);
  if (!(delta < 0.5f)) return INFINITY;
  return 1.001f / (1.f - delta);
}

constexpr int kSettledMaxCells = 36;  // a larger pixel box: not certified

// What both certificates need of a brick: the least and largest corner depth
// under the linear model and the cells of the 16x16-pixel grids under its
// pixel box (2.5 px margin).  False: no certificate (a corner nearer than
// pzmin, a NaN, a box off the image or of more than kSettledMaxCells cells).
struct BrickBox {
  float pznear, pzfar;
  int cx0, cx1, cy0, cy1;
};
KFX_HD inline bool brick_box(const float *R, const float *t, float vs0, float vs1, float fx, float fy, float cx,
                             float cy, int w, int h, int x0, int y0, int z0, BrickBox &b) {
  const float zsx = R[2] * vs0, zsy = R[5] * vs0, zsz = R[8] * vs0;
  const float pzmin = 0.1f * vs0 * (fx > fy ? fx : fy);
  float umin = 0.f, umax = 0.f, vmin = 0.f, vmax = 0.f, pzmax = 0.f, pznear = 0.f;
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
      pzmax = pznear = pz;
    } else {
      umin = u < umin ? u : umin;
      umax = u > umax ? u : umax;
      vmin = v < vmin ? v : vmin;
      vmax = v > vmax ? v : vmax;
      pzmax = pz > pzmax ? pz : pzmax;
      pznear = pz < pznear ? pz : pznear;
    }
    good = good && u == u && v == v;  // NaN
  }
  if (!good) return false;
  const float fu0 = umin - 2.5f > 0.f ? umin - 2.5f : 0.f, fu1 = umax + 2.5f < (float)(w - 1) ? umax + 2.5f : (float)(w - 1);
  const float fv0 = vmin - 2.5f > 0.f ? vmin - 2.5f : 0.f, fv1 = vmax + 2.5f < (float)(h - 1) ? vmax + 2.5f : (float)(h - 1);
  if (!(fu0 <= fu1) || !(fv0 <= fv1)) return false;  // off the image (the frustum clip's business)
  b.cx0 = (int)fu0 >> 4, b.cx1 = (int)fu1 >> 4, b.cy0 = (int)fv0 >> 4, b.cy1 = (int)fv1 >> 4;
  if ((b.cx1 - b.cx0 + 1) * (b.cy1 - b.cy0 + 1) > kSettledMaxCells) return false;
  b.pznear = pznear;
  b.pzfar = pzmax;
  return true;
}

constexpr unsigned kBrickFree = 1u, kBrickHidden = 2u;

// Both certificates of the brick at (x0, y0, z0) from one corner loop and one
// pass over the cells: kBrickFree (brick_certified) when dmin is given and
// `settled` says that the brick's byte is set, kBrickHidden (brick_hidden)
// when dmax is given.
// dmin: the min-depth grid (float bits, +inf bits for a cell without depth);
// dmax: the max-depth grid (float bits, 0 for a cell without depth); nbx cells
// per row; far_k = far_clip_factor, hid_k = hidden_clip_factor of the level-0
// intrinsics.
// The usual box of at most 3x3 cells is read without a branch between the
// loads, so that the device has them in flight together (a cell outside the
// box repeats the box's first column / row: the same minimum and maximum); a
// larger box is read in a loop.
KFX_HD inline unsigned brick_certificates(const float *R, const float *t, float vs0, float vs1, float fx, float fy,
                                          float cx, float cy, int w, int h, int x0, int y0, int z0, float trunc,
                                          const unsigned *dmin, const unsigned *dmax, bool settled, int nbx,
                                          float far_k, float hid_k) {
  BrickBox b;
  if (!brick_box(R, t, vs0, vs1, fx, fy, cx, cy, w, h, x0, y0, z0, b)) return 0u;
  unsigned dm = 0x7f800000u, dx = 0u;  // +inf, 0
  const int nx = b.cx1 - b.cx0 + 1, ny = b.cy1 - b.cy0 + 1;
  if (nx <= 3 && ny <= 3) {
    unsigned cn[9], cm[9];
    for (int k = 0; k < 9; ++k) {
      const int i = k % 3, j = k / 3;
      const int at = (b.cy0 + (j < ny ? j : 0)) * nbx + b.cx0 + (i < nx ? i : 0);
      cn[k] = dmin && settled ? dmin[at] : 0x7f800000u;
      cm[k] = dmax ? dmax[at] : 0u;
    }
    for (int k = 0; k < 9; ++k) {  // positive floats order as their bits
      dm = cn[k] < dm ? cn[k] : dm;
      dx = cm[k] > dx ? cm[k] : dx;
    }
  } else {
    for (int y = b.cy0; y <= b.cy1; ++y)
      for (int x = b.cx0; x <= b.cx1; ++x) {
        if (dmin && settled) {
          const unsigned c = dmin[y * nbx + x];
          dm = c < dm ? c : dm;
        }
        if (dmax) {
          const unsigned c = dmax[y * nbx + x];
          dx = c > dx ? c : dx;
        }
      }
  }
  unsigned out = 0u;
  if (dmin && settled) {
    float Dmin;
    std::memcpy(&Dmin, &dm, 4);
    const float need = (b.pzfar + 2.f * vs0 + trunc) * far_k + 0.01f;
    if (Dmin >= need) out |= kBrickFree;
  }
  if (dmax && hid_k < INFINITY) {
    float Dmax;
    std::memcpy(&Dmax, &dx, 4);
    if (dx == 0u || b.pznear - 2.f * vs0 > (Dmax + trunc) * hid_k) out |= kBrickHidden;
  }
  return out;
}

// (dmax = nullptr leaves the hidden half out, so the hid_k passed is never read)
KFX_HD inline bool brick_certified(const float *R, const float *t, float vs0, float vs1, float fx, float fy, float cx,
                                   float cy, int w, int h, int x0, int y0, int z0, float trunc, const unsigned *dmin,
                                   int nbx, float far_k) {
  return brick_certificates(R, t, vs0, vs1, fx, fy, cx, cy, w, h, x0, y0, z0, trunc, dmin, nullptr, true, nbx, far_k, 0.f) != 0u;
}

// No voxel of the brick can be updated (header comment); hid_k =
// hidden_clip_factor of the level-0 intrinsics
// (dmin = nullptr leaves the free-space half out, so the far_k passed is never read)
KFX_HD inline bool brick_hidden(const float *R, const float *t, float vs0, float vs1, float fx, float fy, float cx,
                                float cy, int w, int h, int x0, int y0, int z0, float trunc, const unsigned *dmax,
                                int nbx, float hid_k) {
  return brick_certificates(R, t, vs0, vs1, fx, fy, cx, cy, w, h, x0, y0, z0, trunc, nullptr, dmax, false, nbx, 0.f, hid_k) != 0u;
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
