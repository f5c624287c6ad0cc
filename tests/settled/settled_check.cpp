// Free-space certificate of integrate's settled-brick skip (csrc/kfx_settled.h)
// against the oracle's per-voxel arithmetic (oracle/kfx_oracle.cpp
// kfo_integrate, tsdf_volume.cu:41-99).
//
// Seeded cases: an intrinsics set from the accepted parameter space, a camera
// a little off the volume's front face, a depth image (metres, as integrate
// reads it) with a tilted background, a nearer half plane (a depth step),
// noise and 0.5 % dropouts, its 16x16 min-depth grid, and bricks drawn three
// ways: anywhere in the volume, ending a few centimetres in front of the
// surface their tile looks at, and on tiles that project across the image
// border.  For every brick the header certifies, each of its 512 voxels is
// evaluated the oracle's way (vc accumulated by float adds from slice 0); a
// voxel that is updated (in front of the camera, in the image, depth > 0,
// sdf >= -trunc) with ts < 1, or inside the colour band, is a failure.
//
// Draw modes (third argument; "base" draws what is described above):
//   rot    the volume turned about its centre by up to +-1.2 rad about x and y
//   aniso  voxels of vs[1], vs[2] = 0.4 .. 2.5 x vs[0]
//   small  images of 16x16 .. 64x48 pixels with fx = 0.3 .. 0.6 w
//   wide   such an image, a brick whose pixel box reaches the image border, and
//          a flat wall at the least depth the certificate accepts for it and up
//          to 0.3 % beyond: the certificate's inequality with nothing to spare
//   bound  no bricks: random intrinsics (fx from 1.5 px), pixels and points
//          that round to them; |vc| / lambda must lie in vc.z [1 - delta,
//          1 + delta] (far_clip_delta), far_clip_factor must cover 1 / (1 -
//          delta), be 1.02f exactly from 38 px on and +inf from delta = 0.5 on
//
// usage: settled_check <seed> <cases> [mode]   prints "bad <n> certified <n> of
// <n> near <n> edge <n>"; exit 0 when bad == 0 and bricks of every kind the
// mode aims at were certified ("bound": "bound bad <n> checked <n>").
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "kfx_settled.h"

namespace {

struct V3 {
  float x, y, z;
};
inline V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 rmul(const float *R, V3 v) {
  return {R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z,
          R[6] * v.x + R[7] * v.y + R[8] * v.z};
}
inline int f2i_rn(float v) {
  const float r = std::rint(v);
  return (r > -2.0e9f && r < 2.0e9f) ? (int)r : INT32_MIN;
}

struct Geom {
  int w, h;
  float fx, fy, cx, cy;
};

// what kfo_integrate does with voxel (x, y, z): 0 not updated, 1 updated with
// ts = 1 outside the colour band, 2 anything else (a store could follow)
struct Vox {
  int kind;
  bool in_image;
};
Vox voxel(const float *R, const float *t, const float *vs, const Geom &g, const std::vector<float> &dmap, float trunc,
          int x, int y, int z) {
  const V3 tt = {t[0], t[1], t[2]};
  const V3 zstep = {R[2] * vs[0], R[5] * vs[0], R[8] * vs[0]};
  V3 vc = add(rmul(R, {(float)x * vs[0], (float)y * vs[1], 0.f * vs[2]}), tt);
  for (int k = 1; k <= z; ++k) vc = add(vc, zstep);
  if (z < 1) return {0, false};  // slice 0 is never updated
  if (vc.z <= 0) return {0, false};
  const int u = f2i_rn((vc.x / vc.z) * g.fx + g.cx);
  const int v = f2i_rn((vc.y / vc.z) * g.fy + g.cy);
  if (u < 0 || u >= g.w || v < 0 || v >= g.h) return {0, false};
  const float depth = dmap[(size_t)v * g.w + u];
  if (depth <= 0) return {0, true};
  const V3 xyl = {(1.f * ((float)u - g.cx)) / g.fx, (1.f * ((float)v - g.cy)) / g.fy, 1.f};
  const float lambda = std::sqrt(dot(xyl, xyl));
  const float sdf = -((1.f / lambda) * std::sqrt(dot(vc, vc)) - depth);
  if (!(sdf >= -trunc)) return {0, true};
  const float ts = std::fmin(1.f, sdf / trunc);
  const float thres_color = trunc / 2;
  if (ts < 1.f || (sdf <= thres_color && sdf >= -thres_color)) return {2, true};
  return {1, true};
}

// far_clip_delta / far_clip_factor against brute force
int check_bound(unsigned seed, int cases) {
  std::mt19937 rng(seed);
  auto U = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
  long bad = 0, checked = 0;
  for (int c = 0; c < cases; ++c) {
    const float fx = (float)std::exp(U(std::log(1.5), std::log(700.0))), fy = fx * (float)U(0.8, 1.25);
    const int w = 8 * (int)U(2, 160), h = 8 * (int)U(2, 90);
    const float cx = (float)U(-0.2, 1.2) * w, cy = (float)U(-0.2, 1.2) * h;
    const float delta = kfx::far_clip_delta(fx, fy), k = kfx::far_clip_factor(fx, fy);
    const double dd = 0.5 * std::hypot(1.0 / fx, 1.0 / fy);
    bool ok = std::fabs(delta - dd) <= 1e-6 * dd;
    if (dd >= 0.5 + 1e-6) ok = ok && std::isinf(k) && k > 0;
    if (dd < 0.5 - 1e-6) ok = ok && k >= 1.02f && (double)k >= 1.0005 / (1.0 - dd) && (double)k <= 1.0015 / (1.0 - dd) + 0.02;
    if (fx >= 38.f && fy >= 38.f) ok = ok && k == 1.02f;
    if (!ok && ++bad <= 5) std::printf("case %d: fx %g fy %g delta %g factor %g\n", c, fx, fy, delta, k);
    for (int i = 0; i < 4000; ++i) {
      // a pixel of the image (corners and borders often), a point that rounds to it
      const int u = U(0, 1) < 0.3 ? (U(0, 1) < 0.5 ? 0 : w - 1) : (int)U(0, w - 1e-9);
      const int v = U(0, 1) < 0.3 ? (U(0, 1) < 0.5 ? 0 : h - 1) : (int)U(0, h - 1e-9);
      const double du = U(0, 1) < 0.3 ? (U(0, 1) < 0.5 ? -0.4999 : 0.4999) : U(-0.4999, 0.4999);
      const double dv = U(0, 1) < 0.3 ? (U(0, 1) < 0.5 ? -0.4999 : 0.4999) : U(-0.4999, 0.4999);
      const double z = U(0.05, 12.0);
      const double x = z * (u + du - cx) / fx, y = z * (v + dv - cy) / fy;
      // lambda the oracle's way (float), the rest in double
      const V3 xyl = {(1.f * ((float)u - cx)) / fx, (1.f * ((float)v - cy)) / fy, 1.f};
      const double lambda = std::sqrt(dot(xyl, xyl));
      const double ratio = std::sqrt(x * x + y * y + z * z) / (lambda * z);
      ++checked;
      if (!(ratio >= 1.0 - dd - 1e-5 && ratio <= 1.0 + dd + 1e-5) && ++bad <= 5)
        std::printf("case %d pixel (%d, %d): |vc| / (lambda z) = %.7f outside 1 -+ %.7f\n", c, u, v, ratio, dd);
    }
  }
  std::printf("bound bad %ld checked %ld\n", bad, checked);
  return bad == 0 && checked > 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
  const int cases = argc > 2 ? std::atoi(argv[2]) : 200;
  const std::string mode = argc > 3 ? argv[3] : "base";
  const bool m_rot = mode == "rot", m_aniso = mode == "aniso", m_small = mode == "small", m_wide = mode == "wide";
  if (mode == "bound") return check_bound(seed, cases);
  if (!(mode == "base" || m_rot || m_aniso || m_small || m_wide)) {
    std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 2;
  }
  std::mt19937 rng(seed);
  auto U = [&](double a, double b) { return (float)std::uniform_real_distribution<double>(a, b)(rng); };
  auto I = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
  static const int sizes[][2] = {{640, 480}, {320, 240}, {328, 248}, {1280, 720}, {160, 120}};
  static const int dims[] = {64, 128, 256, 512};
  long bad = 0, cert = 0, total = 0, near = 0, edge = 0;
  for (int c = 0; c < cases; ++c) {
    const int si = I(0, 4), N = dims[I(m_wide ? 2 : 0, 3)];  // (wide: fine voxels, so that the 2-voxel margin is small)
    Geom g;
    g.w = sizes[si][0];
    g.h = sizes[si][1];
    g.fx = g.w * U(0.7, 1.0);
    if (m_small || m_wide) {
      g.w = 8 * I(2, 8);
      g.h = 8 * I(2, 6);
      g.fx = g.w * U(0.3, 0.6);
    }
    g.fy = g.fx * U(0.9, 1.1);
    g.cx = (g.w - 1) / 2.f + U(-12, 12);
    g.cy = (g.h - 1) / 2.f + U(-12, 12);
    const float L = U(1.5, 3.2);
    float vs[3] = {L / N, L / N, L / N};
    if (m_aniso) {
      vs[1] = vs[0] * U(0.4, 2.5);
      vs[2] = vs[0] * U(0.4, 2.5);
    }
    const float trunc = vs[0] * U(1.6, 4.0);
    const float far_k = kfx::far_clip_factor(g.fx, g.fy);
    // vol2cam = camera^-1 * translate(-L/2, -L/2, 0.5): a small rotation and offset
    const float amax = m_rot ? 1.2 : 0.15;
    const float ax = U(-amax, amax), ay = U(-amax, amax), az = U(-0.08, 0.08);
    const float cxr = std::cos(ax), sxr = std::sin(ax), cyr = std::cos(ay), syr = std::sin(ay), czr = std::cos(az),
                szr = std::sin(az);
    const float R[9] = {cyr * czr, -cyr * szr, syr,
                        sxr * syr * czr + cxr * szr, -sxr * syr * szr + cxr * czr, -sxr * cyr,
                        -cxr * syr * czr + sxr * szr, cxr * syr * szr + sxr * czr, cxr * cyr};
    const float o[3] = {-L / 2 + U(-0.15, 0.15), -L / 2 + U(-0.15, 0.15), 0.5f + U(-0.1, 0.3)};
    float t[3];
    for (int i = 0; i < 3; ++i) t[i] = R[3 * i] * o[0] + R[3 * i + 1] * o[1] + R[3 * i + 2] * o[2];
    if (m_rot) {  // about the volume's centre, which stays in front of the camera
      const float cen[3] = {N * vs[0] / 2, N * vs[1] / 2, N * vs[0] / 2};
      const float at[3] = {o[0] + L / 2, o[1] + L / 2, o[2] + L / 2};
      for (int i = 0; i < 3; ++i) t[i] = at[i] - (R[3 * i] * cen[0] + R[3 * i + 1] * cen[1] + R[3 * i + 2] * cen[2]);
    }
    // depth (m): tilted background, a nearer half plane, noise, dropouts
    std::vector<float> dmap((size_t)g.w * g.h);
    const float d0 = U(1.0, 0.5 + L), gx = U(-0.3, 0.3) / g.w, gy = U(-0.3, 0.3) / g.h;
    const float dstep = U(0.3, 0.9), sa = U(-1, 1), sb = U(-1, 1), sc = U(0.2, 0.8);
    std::normal_distribution<float> noise(0.f, 0.002f);
    for (int y = 0; y < g.h; ++y)
      for (int x = 0; x < g.w; ++x) {
        float d = d0 + gx * x + gy * y;
        if (sa * (x - sc * g.w) + sb * (y - sc * g.h) > 0) d -= dstep;
        d += noise(rng);
        if (U(0, 1) < 0.005f) d = 0.f;
        dmap[(size_t)y * g.w + x] = d > 0.05f ? d : 0.f;
      }
    const int nbx = (g.w + 15) >> 4, nby = (g.h + 15) >> 4;
    std::vector<unsigned> dmin((size_t)nbx * nby);
    auto build_dmin = [&]() {
      std::fill(dmin.begin(), dmin.end(), 0x7f800000u);
      for (int y = 0; y < g.h; ++y)
        for (int x = 0; x < g.w; ++x) {
          const float d = dmap[(size_t)y * g.w + x];
          if (d > 0.f) {
            unsigned b;
            std::memcpy(&b, &d, 4);
            unsigned &m = dmin[(size_t)(y >> 4) * nbx + (x >> 4)];
            m = b < m ? b : m;
          }
        }
    };
    build_dmin();
    const int T = N / 8;
    for (int b = 0; b < 48; ++b) {
      int x0 = 8 * I(0, T - 1), y0 = 8 * I(0, T - 1), z0 = 8 * I(0, T - 1);
      const int how = b % 3;
      if (how == 1) {  // the brick that ends a few centimetres in front of the surface under the tile's centre
        const V3 c0 = add(rmul(R, {(x0 + 3.5f) * vs[0], (y0 + 3.5f) * vs[1], 0.f}), {t[0], t[1], t[2]});
        const float szz = R[8] * vs[0];
        if (!(std::fabs(szz) > 0.05f * vs[0])) continue;  // (rot: a column nearly parallel to the image plane)
        // centre pixel at mid depth, then the slice where vc.z = depth - trunc - 0..10 cm
        const float zm = c0.z + szz * (N / 2);
        if (!(zm > 0.05f)) continue;
        const int u = f2i_rn(((c0.x + R[2] * vs[0] * (N / 2)) / zm) * g.fx + g.cx);
        const int v = f2i_rn(((c0.y + R[5] * vs[0] * (N / 2)) / zm) * g.fy + g.cy);
        if (u < 0 || u >= g.w || v < 0 || v >= g.h) continue;
        const float d = dmap[(size_t)v * g.w + u];
        if (!(d > 0)) continue;
        const int zs = (int)((d - trunc - U(0.0, 0.10) - c0.z) / szz);
        z0 = ((zs - 7) / 8) * 8 - 8 * I(0, 1);
        if (z0 < 0 || z0 > N - 8) continue;
      }
      if (m_wide) {
        // among the volume's farthest bricks: the half pixel is worth the most there
        z0 = 8 * (T - 1 - I(0, 3));
        // the brick's pixel box and farthest corner as the certificate forms them
        float umin = 0, umax = 0, vmin = 0, vmax = 0, pzmax = 0, pzmin = 0;
        for (int k = 0; k < 8; ++k) {
          const float vx = (float)(x0 + ((k & 1) ? 7 : 0)) * vs[0], vy = (float)(y0 + ((k & 2) ? 7 : 0)) * vs[1];
          const float z = (float)(z0 + ((k & 4) ? 7 : 0));
          const float px = (R[0] * vx + R[1] * vy + t[0]) + z * (R[2] * vs[0]);
          const float py = (R[3] * vx + R[4] * vy + t[1]) + z * (R[5] * vs[0]);
          const float pz = (R[6] * vx + R[7] * vy + t[2]) + z * (R[8] * vs[0]);
          const float u = g.fx * (px / pz) + g.cx, v = g.fy * (py / pz) + g.cy;
          umin = k ? std::fmin(umin, u) : u;
          umax = k ? std::fmax(umax, u) : u;
          vmin = k ? std::fmin(vmin, v) : v;
          vmax = k ? std::fmax(vmax, v) : v;
          pzmax = k ? std::fmax(pzmax, pz) : pz;
          pzmin = k ? std::fmin(pzmin, pz) : pz;
        }
        if (!(pzmin > 0.05f)) continue;
        const bool on_image = umax >= 0 && umin <= g.w - 1 && vmax >= 0 && vmin <= g.h - 1;
        const bool at_border = umin < 1 || vmin < 1 || umax > g.w - 2 || vmax > g.h - 2;
        if (!on_image || !at_border || !std::isfinite(far_k)) continue;
        const float need = (pzmax + 2.f * vs[0] + trunc) * far_k + 0.01f;
        const float wall = need * (1.f + 0.003f * U(0, 1) * (b & 1)) * 1.0000005f;  // every other one at the bound itself
        for (auto &d : dmap) d = wall + U(0, 0.0005) * (b & 2 ? 1 : 0);
        build_dmin();
      }
      ++total;
      if (!kfx::brick_certified(R, t, vs[0], vs[1], g.fx, g.fy, g.cx, g.cy, g.w, g.h, x0, y0, z0, trunc, dmin.data(),
                                nbx, far_k))
        continue;
      ++cert;
      near += how == 1;
      int in = 0, out = 0;
      for (int i = 0; i < 512; ++i) {
        const Vox q = voxel(R, t, vs, g, dmap, trunc, x0 + (i & 7), y0 + ((i >> 3) & 7), z0 + (i >> 6));
        in += q.in_image;
        out += !q.in_image;
        if (q.kind == 2) {
          if (++bad <= 5)
            std::printf("case %d brick (%d, %d, %d) voxel %d: updated with ts < 1 or coloured\n", c, x0, y0, z0, i);
        }
      }
      edge += in > 0 && out > 0;
    }
  }
  std::printf("bad %ld certified %ld of %ld near %ld edge %ld\n", bad, cert, total, near, edge);
  if (m_wide) return (bad == 0 && cert > 0) ? 0 : 1;  // (every brick there is a directed one, its box on the border)
  return (bad == 0 && cert > 0 && near > 0 && edge > 0) ? 0 : 1;
}
