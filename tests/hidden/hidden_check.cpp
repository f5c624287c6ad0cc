// Hidden-brick certificate of integrate (csrc/kfx_settled.h brick_hidden,
// DESIGN.md §17) against the oracle's per-voxel arithmetic (oracle/kfx_oracle.cpp
// kfo_integrate, tsdf_volume.cu:41-99).
//
// Seeded cases.  Cameras in turn: VGA, QVGA, a coarse one (64x48 .. 160x120
// pixels, 38 <= f < 100 px) and one with delta >= 0.5 (f <= 1.3 px).  Poses
// turned by up to 0.52 rad about x and y, sometimes with the camera inside the
// volume (bricks near pzmin); a third of the cases with non-cubic voxels.
// Depth images (metres): a tilted background, a nearer half plane (a
// discontinuity), noise, 0.5 % .. 20 % dropouts and, in a third of the cases,
// a quadrant without depth.  Every fourth brick of a case is drawn against a
// flat wall whose depth lies within 3 ulps of the certificate's own bound for
// that brick (Dmax straddled).  Bricks are drawn anywhere, a few centimetres
// behind the surface their tile looks at, and on tiles that project across the
// image border.  For every brick the header certifies, each of its 512 voxels
// is evaluated the oracle's way (vc accumulated by float adds from slice 0); a
// voxel that is updated (in front of the camera, in the image, depth > 0,
// sdf >= -trunc) is a failure, and so is any brick certified under the
// delta >= 0.5 camera.
//
// Modes (third argument):
//   base   the draws above
//   bound  hidden_clip_factor against brute force over pixels
//   sign   directed: a coarse camera, fine voxels, a flat wall at the depth
//          where the certificate with hid_k = 1 - 2 delta just accepts the brick
//   drift  directed: a column 8000 slices deep whose z step loses 0.45 ulp in
//          every add while |vc.z| is in [16, 32), the camera inside the volume
//          at its far end, the brick's corner voxel on the optical axis at
//          about pzmin, a flat wall where the certificate without its 2-voxel
//          drift margin just accepts the brick
// Mutations (fourth argument): "sign" evaluates the certificate with hid_k =
// 1 - 2 delta, "nodrift" without the drift margin (trunc - 2 vs / hid_k passed
// as trunc: pznear > (Dmax + trunc) hid_k is the certificate with the margin
// taken out).  Each must make its directed mode fail.
//
// usage: hidden_check <seed> <cases> [mode] [mutation]   prints "bad <n>
// certified <n> of <n> near <n> edge <n> coarse <n>"; exit 0 when bad == 0
// ("bound": "bound bad <n> checked <n>").
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
inline unsigned bits(float f) {
  unsigned b;
  std::memcpy(&b, &f, 4);
  return b;
}
inline float from_bits(unsigned b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

struct Geom {
  int w, h;
  float fx, fy, cx, cy;
};

// the column (x, y) of kfo_integrate up to slice z: its accumulated vc
V3 column_vc(const float *R, const float *t, const float *vs, int x, int y, int z) {
  const V3 tt = {t[0], t[1], t[2]};
  const V3 zstep = {R[2] * vs[0], R[5] * vs[0], R[8] * vs[0]};
  V3 vc = add(rmul(R, {(float)x * vs[0], (float)y * vs[1], 0.f * vs[2]}), tt);
  for (int k = 1; k <= z; ++k) vc = add(vc, zstep);
  return vc;
}

// what kfo_integrate does with a voxel at vc: updated, in the image, its depth
struct Vox {
  bool updated, in_image;
  float depth;
};
Vox voxel(V3 vc, const Geom &g, const std::vector<float> &dmap, float trunc, int z) {
  if (z < 1) return {false, false, 0.f};  // slice 0 is never updated
  if (vc.z <= 0) return {false, false, 0.f};
  const int u = f2i_rn((vc.x / vc.z) * g.fx + g.cx);
  const int v = f2i_rn((vc.y / vc.z) * g.fy + g.cy);
  if (u < 0 || u >= g.w || v < 0 || v >= g.h) return {false, false, 0.f};
  const float depth = dmap[(size_t)v * g.w + u];
  if (depth <= 0) return {false, true, depth};
  const V3 xyl = {(1.f * ((float)u - g.cx)) / g.fx, (1.f * ((float)v - g.cy)) / g.fy, 1.f};
  const float lambda = std::sqrt(dot(xyl, xyl));
  const float sdf = -((1.f / lambda) * std::sqrt(dot(vc, vc)) - depth);
  return {sdf >= -trunc, true, depth};
}

struct Counts {
  long bad = 0, cert = 0, total = 0, near = 0, edge = 0, coarse = 0, blind = 0;
};

std::vector<unsigned> build_dmax(const Geom &g, const std::vector<float> &dmap) {
  const int nbx = (g.w + 15) >> 4, nby = (g.h + 15) >> 4;
  std::vector<unsigned> dmax((size_t)nbx * nby, 0u);
  for (int y = 0; y < g.h; ++y)
    for (int x = 0; x < g.w; ++x) {
      const float d = dmap[(size_t)y * g.w + x];
      if (d > 0.f) {
        unsigned &m = dmax[(size_t)(y >> 4) * nbx + (x >> 4)];
        m = bits(d) > m ? bits(d) : m;
      }
    }
  return dmax;
}

enum Mut { kNone, kSign, kNoDrift };

// the certificate under the mutation
bool hidden(Mut mut, const float *R, const float *t, const float *vs, const Geom &g, int x0, int y0, int z0, float trunc,
            const std::vector<unsigned> &dmax) {
  const int nbx = (g.w + 15) >> 4;
  float k = kfx::hidden_clip_factor(g.fx, g.fy), tr = trunc;
  if (mut == kSign && std::isfinite(k)) k = 1.f - 2.f * kfx::far_clip_delta(g.fx, g.fy);
  if (mut == kNoDrift && std::isfinite(k)) tr = trunc - 2.f * vs[0] / k;
  return kfx::brick_hidden(R, t, vs[0], vs[1], g.fx, g.fy, g.cx, g.cy, g.w, g.h, x0, y0, z0, tr, dmax.data(), nbx, k);
}

// all 512 voxels of a certified brick
void evaluate(Counts &n, const char *what, int c, const float *R, const float *t, const float *vs, const Geom &g,
              const std::vector<float> &dmap, float trunc, int x0, int y0, int z0) {
  int in = 0, out = 0;
  for (int j = 0; j < 64; ++j) {
    const int x = x0 + (j & 7), y = y0 + (j >> 3);
    V3 vc = column_vc(R, t, vs, x, y, z0);
    const V3 zstep = {R[2] * vs[0], R[5] * vs[0], R[8] * vs[0]};
    for (int z = z0; z < z0 + 8; ++z) {
      const Vox q = voxel(vc, g, dmap, trunc, z);
      in += q.in_image;
      out += !q.in_image;
      if (q.updated && ++n.bad <= 5)
        std::printf("%s case %d brick (%d, %d, %d) voxel (%d, %d, %d): updated\n", what, c, x0, y0, z0, x, y, z);
      if (j == 27 && z == z0 + 3 && q.in_image && q.depth > 0 && vc.z - q.depth < 0.10f) ++n.near;  // a centre voxel
      vc = add(vc, zstep);
    }
  }
  n.edge += in > 0 && out > 0;
}

int check_bound(unsigned seed, int cases) {
  std::mt19937 rng(seed);
  auto U = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
  long bad = 0, checked = 0;
  for (int c = 0; c < cases; ++c) {
    const float fx = (float)std::exp(U(std::log(1.0), std::log(700.0))), fy = fx * (float)U(0.8, 1.25);
    const int w = 8 * (int)U(2, 160), h = 8 * (int)U(2, 90);
    const float cx = (float)U(-0.2, 1.2) * w, cy = (float)U(-0.2, 1.2) * h;
    const float k = kfx::hidden_clip_factor(fx, fy);
    const double dd = 0.5 * std::hypot(1.0 / fx, 1.0 / fy);
    bool ok = true;
    if (dd >= 0.5 + 1e-6) ok = std::isinf(k) && k > 0;
    if (dd < 0.5 - 1e-6) ok = (double)k >= 1.0005 / (1.0 - dd) && (double)k <= 1.0015 / (1.0 - dd);
    if (dd < 0.5 - 1e-6) ok = ok && k <= kfx::far_clip_factor(fx, fy);
    if (!ok && ++bad <= 5) std::printf("case %d: fx %g fy %g delta %g factor %g\n", c, fx, fy, dd, k);
    if (!std::isfinite(k)) continue;
    for (int i = 0; i < 4000; ++i) {
      // a pixel of the image (corners and borders often), a point that rounds to
      // it; with D the pixel's depth the point is updated only if
      // |vc| / lambda <= D + trunc, so vc.z > (D + trunc) k must rule that out
      const int u = U(0, 1) < 0.3 ? (U(0, 1) < 0.5 ? 0 : w - 1) : (int)U(0, w - 1e-9);
      const int v = U(0, 1) < 0.3 ? (U(0, 1) < 0.5 ? 0 : h - 1) : (int)U(0, h - 1e-9);
      const double du = U(0, 1) < 0.3 ? (U(0, 1) < 0.5 ? -0.4999 : 0.4999) : U(-0.4999, 0.4999);
      const double dv = U(0, 1) < 0.3 ? (U(0, 1) < 0.5 ? -0.4999 : 0.4999) : U(-0.4999, 0.4999);
      const double z = U(0.05, 12.0);
      const double x = z * (u + du - cx) / fx, y = z * (v + dv - cy) / fy;
      const V3 xyl = {(1.f * ((float)u - cx)) / fx, (1.f * ((float)v - cy)) / fy, 1.f};
      const double lambda = std::sqrt(dot(xyl, xyl));
      const double range = std::sqrt(x * x + y * y + z * z) / lambda;  // |vc| / lambda
      ++checked;
      // the largest D + trunc the factor still calls hidden at this z
      if (!(range > (z / (double)k) * 1.0005) && ++bad <= 5)
        std::printf("case %d pixel (%d, %d): |vc| / lambda = %.7f z against z / k = %.7f z\n", c, u, v, range / z, 1.0 / k);
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
  const std::string mname = argc > 4 ? argv[4] : "none";
  const Mut mut = mname == "sign" ? kSign : mname == "nodrift" ? kNoDrift : kNone;
  if (mode == "bound") return check_bound(seed, cases);
  std::mt19937 rng(seed);
  auto U = [&](double a, double b) { return (float)std::uniform_real_distribution<double>(a, b)(rng); };
  auto I = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
  Counts n;

  if (mode == "drift") {
    for (int c = 0; c < cases; ++c) {
      Geom g = {64, 48, 60.f + (float)I(0, 30), 0.f, 32.f, 24.f};
      g.fy = g.fx;
      // vc.z in [-32, -16) has ulp 2^-19: a step of (2097 + frac) ulps loses frac ulp per add
      const float vs0 = (2097.f + U(0.40, 0.49)) * 0x1p-19f;
      const float vs[3] = {vs0, vs0, vs0};
      const float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      const int xc = 8 * I(1, 6), yc = 8 * I(1, 6), zt = I(7800, 7990);
      const float t[3] = {-((float)xc * vs0), -((float)yc * vs0), -((float)zt * vs0)};
      const float trunc = 2.f * vs0, pzmin = 0.1f * vs0 * g.fx;
      const int z0 = 8 * ((zt + (int)(pzmin / vs0) + 9) / 8);
      kfx::BrickBox b;
      if (!kfx::brick_box(R, t, vs0, vs0, g.fx, g.fy, g.cx, g.cy, g.w, g.h, xc, yc, z0, b)) continue;
      const float k = kfx::hidden_clip_factor(g.fx, g.fy);
      const float wall = b.pznear / k * (1.f - 2e-6f) - trunc;  // pznear > (wall + trunc) k: the margin-less bound, just met
      if (!(wall > 0.f)) continue;
      std::vector<float> dmap((size_t)g.w * g.h, wall);
      const std::vector<unsigned> dmax = build_dmax(g, dmap);
      ++n.total;
      if (c < 3) {
        const V3 vc = column_vc(R, t, vs, xc, yc, z0);
        std::printf("drift case %d: corner voxel vc.z accumulated %.7g, linear %.7g (drift %.3g voxels), wall + trunc %.7g\n", c,
                    vc.z, b.pznear, (b.pznear - vc.z) / vs0, wall + trunc);
      }
      if (!hidden(mut, R, t, vs, g, xc, yc, z0, trunc, dmax)) continue;
      ++n.cert;
      evaluate(n, "drift", c, R, t, vs, g, dmap, trunc, xc, yc, z0);
    }
    std::printf("bad %ld certified %ld of %ld near %ld edge %ld coarse %ld\n", n.bad, n.cert, n.total, n.near, n.edge, n.coarse);
    return n.bad == 0 && n.total > 0 ? 0 : 1;
  }

  const bool m_sign = mode == "sign";
  if (!(mode == "base" || m_sign)) {
    std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 2;
  }
  static const int dims[] = {64, 128, 256, 512};
  for (int c = 0; c < cases; ++c) {
    const int cam = m_sign ? 2 : (c % 8 == 7 ? 3 : c % 3);  // VGA, QVGA, coarse; every eighth: delta >= 0.5
    const int N = dims[m_sign ? I(2, 3) : I(0, 3)];
    Geom g;
    if (cam == 0) g.w = 640, g.h = 480, g.fx = 525.f * U(0.9, 1.1);
    if (cam == 1) g.w = 320, g.h = 240, g.fx = 262.f * U(0.9, 1.1);
    if (cam == 2) g.w = 8 * I(8, 20), g.h = 8 * I(6, 15), g.fx = U(38.0, 99.9);
    if (cam == 3) g.w = 8 * I(1, 3), g.h = 8 * I(1, 3), g.fx = U(0.6, 1.3);
    g.fy = cam == 3 ? g.fx * U(0.9, 1.0) : g.fx * U(0.9, 1.1);
    if (cam == 2 && g.fy < 38.f) g.fy = 38.f;
    if (cam == 2 && g.fy >= 100.f) g.fy = 99.9f;
    g.cx = (g.w - 1) / 2.f + U(-0.1, 0.1) * g.w;
    g.cy = (g.h - 1) / 2.f + U(-0.1, 0.1) * g.h;
    const float L = U(1.5, 3.2);
    float vs[3] = {L / N, L / N, L / N};
    if (c % 3 == 1 && !m_sign) {
      vs[1] = vs[0] * U(0.5, 2.0);
      vs[2] = vs[0] * U(0.5, 2.0);
    }
    const float trunc = vs[0] * U(1.6, 4.0);
    const float amax = m_sign ? 0.1 : 0.52;
    const float ax = U(-amax, amax), ay = U(-amax, amax), az = U(-0.08, 0.08);
    const float cxr = std::cos(ax), sxr = std::sin(ax), cyr = std::cos(ay), syr = std::sin(ay), czr = std::cos(az),
                szr = std::sin(az);
    const float R[9] = {cyr * czr, -cyr * szr, syr,
                        sxr * syr * czr + cxr * szr, -sxr * syr * szr + cxr * czr, -sxr * cyr,
                        -cxr * syr * czr + sxr * szr, cxr * syr * szr + sxr * czr, cxr * cyr};
    // the camera in front of the volume, or (every fourth case) inside it
    const float oz = (c % 4 == 3) ? -L * U(0.1, 0.6) : 0.5f + U(-0.1, 0.3);
    const float o[3] = {-L / 2 + U(-0.15, 0.15), -(N * vs[1]) / 2 + U(-0.15, 0.15), oz};
    float t[3];
    for (int i = 0; i < 3; ++i) t[i] = R[3 * i] * o[0] + R[3 * i + 1] * o[1] + R[3 * i + 2] * o[2];
    // depth (m): tilted background, a nearer half plane, noise, dropouts, a quadrant without depth
    std::vector<float> dmap((size_t)g.w * g.h), scene;
    const float d0 = U(0.8, 0.5 + L), gx = U(-0.3, 0.3) / g.w, gy = U(-0.3, 0.3) / g.h;
    const float dstep = U(0.2, 0.6), sa = U(-1, 1), sb = U(-1, 1), sc = U(0.2, 0.8);
    const float drop = (c % 5 == 0) ? 0.2f : 0.005f;
    const int quad = (c % 3 == 2) ? I(0, 3) : -1;
    std::normal_distribution<float> noise(0.f, 0.002f);
    for (int y = 0; y < g.h; ++y)
      for (int x = 0; x < g.w; ++x) {
        float d = d0 + gx * x + gy * y;
        if (sa * (x - sc * g.w) + sb * (y - sc * g.h) > 0) d -= dstep;
        d += noise(rng);
        if (U(0, 1) < drop) d = 0.f;
        if (quad >= 0 && (x >= g.w / 2) == (quad & 1) && (y >= g.h / 2) == (quad >> 1)) d = 0.f;
        dmap[(size_t)y * g.w + x] = d > 0.05f ? d : 0.f;
      }
    scene = dmap;
    std::vector<unsigned> dmax = build_dmax(g, dmap);
    const int T = N / 8;
    const float hk = kfx::hidden_clip_factor(g.fx, g.fy);
    for (int b = 0; b < 48; ++b) {
      int x0 = 8 * I(0, T - 1), y0 = 8 * I(0, T - 1), z0 = 8 * I(0, T - 1);
      const int how = m_sign ? 3 : b % 4;
      if (how == 1) {  // the brick that starts a few centimetres behind the surface under the tile's centre
        const V3 c0 = add(rmul(R, {(x0 + 3.5f) * vs[0], (y0 + 3.5f) * vs[1], 0.f}), {t[0], t[1], t[2]});
        const float szz = R[8] * vs[0];
        const float zm = c0.z + szz * (N / 2);
        if (!(zm > 0.05f)) continue;
        const int u = f2i_rn(((c0.x + R[2] * vs[0] * (N / 2)) / zm) * g.fx + g.cx);
        const int v = f2i_rn(((c0.y + R[5] * vs[0] * (N / 2)) / zm) * g.fy + g.cy);
        if (u < 0 || u >= g.w || v < 0 || v >= g.h) continue;
        const float d = dmap[(size_t)v * g.w + u];
        if (!(d > 0)) continue;
        const int zs = (int)((d + trunc + U(0.0, 0.08) - c0.z) / szz);
        z0 = ((zs + 7) / 8) * 8 + 8 * I(0, 1);
        if (z0 < 0 || z0 > N - 8) continue;
      }
      if (how == 2) {  // a tile on the rim of the volume: its projection crosses the image border more often
        if (b & 4) x0 = (b & 8) ? 0 : 8 * (T - 1);
        else y0 = (b & 8) ? 0 : 8 * (T - 1);
      }
      const bool flat = how == 3;
      if (flat) {
        // a flat wall within 3 ulps of the bound the (mutated, in sign mode) certificate sets for this brick
        kfx::BrickBox bb;
        if (!std::isfinite(hk) || !kfx::brick_box(R, t, vs[0], vs[1], g.fx, g.fy, g.cx, g.cy, g.w, g.h, x0, y0, z0, bb)) continue;
        const float k = m_sign ? 1.f - 2.f * kfx::far_clip_delta(g.fx, g.fy) : hk;
        float wall = (bb.pznear - 2.f * vs[0]) / k - trunc;
        if (!(wall > 0.05f)) continue;
        wall = m_sign ? wall * (1.f - 1e-5f) : from_bits(bits(wall) + (unsigned)(I(0, 6) - 3));
        std::fill(dmap.begin(), dmap.end(), wall);
        dmax = build_dmax(g, dmap);
      }
      ++n.total;
      const bool cert = hidden(mut, R, t, vs, g, x0, y0, z0, trunc, dmax);
      if (cert) {
        ++n.cert;
        n.coarse += cam == 2;
        n.blind += cam == 3;
        evaluate(n, mode.c_str(), c, R, t, vs, g, dmap, trunc, x0, y0, z0);
      }
      if (flat) {
        dmap = scene;
        dmax = build_dmax(g, dmap);
      }
    }
  }
  if (n.blind) std::printf("%ld bricks certified under a camera with delta >= 0.5\n", n.blind);
  std::printf("bad %ld certified %ld of %ld near %ld edge %ld coarse %ld\n", n.bad, n.cert, n.total, n.near, n.edge, n.coarse);
  return n.bad == 0 && n.blind == 0 && n.total > 0 ? 0 : 1;
}
