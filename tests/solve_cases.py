"""Crafted systems for what follows the ICP's 27 sums: the unpack, the 3+3
block solve, the determinant test, the Rodrigues step, pose = pose * inc and
the coarse-to-fine loop that stops at the first failure; and a reference for
all of it that shares no code with the oracle or the kernels.

The reference starts from the 27 integer sums (icp_cases.accumulate_np):

  solve     A and b as exact rationals (fractions.Fraction); exact rank, exact
            determinant, exact x where det != 0 (exact_solve).
  decision  exact |det| against the exact value of the double 1e-15 (THR).
  step      rv and t are float32(x) (the narrowing is part of the definition);
            theta and the Rodrigues matrix from mpmath at 60 digits (rodrigues_mp);
            the composition with the incoming pose in float32 numpy in
            kfo_pose_mul's order (pose_mul_f32).
  restate_step restates the oracle's Rodrigues step of the theta < 0.5 arm
            operation for operation (fused multiply-adds as one rounding of the
            exact rational value), so that arm is held bit for bit.

A case is the per-level maps (CUR and PREV vertex and normal maps, all current
normals NaN but the correspondences'), the thresholds, the iteration counts and
what it is named for (case_table).  Single-level cases are 32x32, level-loop
cases 128x128 / 64x64 / 32x32.  Vertices sit on exactly projecting pixels
(icp_cases.crafted_intrinsics, dyadic depths); the model normal enters the row
unnormalised, row = [vcur x npre, npre, npre . (vpre - vcur)], so a short npre
passes the sine gate and scales A.

Measured on the oracle over this table (tests/test_solve_cases.py, which
asserts them):

  x       |x_oracle - x_exact|_inf <= c * kappa_2(A) * 2^-53 * |x|_inf with
          c = 8 * the largest ratio measured = 8 * 0.41 = 3.3 (X_BOUND_C; the
          largest is level 1 of iters_110).  The ratio does not grow with
          kappa, it falls: 0.031, 0.0015 and 1.7e-5 on the cone systems at
          kappa 69, 5.1e5 and 8.4e9 (the error stays near 1e-16 relative).
  det     the ladder's exact det / 1e-15: 0.49999966, 1.99999992, 0.99899987
          and 1.00100038 for 0.5, 2 and 1 -+ 1e-3 (all twelve normals scaled by
          one float32), and the closest a search over float32 steps of one
          model normal's length reaches: 1 - 2.5e-7 below and 1 + 3.4e-8 above
          (the 2^-32 rounding of the products makes the det a step function of
          that length, with steps near 4e-7).  All six are decided alike by the
          exact reference and the oracle.
  R       the increment's R differs from the mpmath matrix by at most 0.50
          ulps of 1.0f per entry over the table (bound asserted: 2).

Not built: a system with 0 < theta < 2.2e-16 in exact arithmetic.  b is a
multiple of 2^-32, so it needs a rotation block of P's Schur complement above
2^-32 / 2.2e-16 = 1.05e6, which is some four thousand rows with entries near 30
(a 64x64 image filled at 30 m); this table stops at a few dozen rows.  What it
has instead is pure_translation: small dyadic rows whose products are exact, b
= A (0, t) exactly, so the exact rotation is 0 and the oracle's and the
device's is the block solve's rounding noise, far below 2.2e-16 but not 0; the
identity arm is reached with a non-zero translation and a non-zero theta.
"""
import math
from fractions import Fraction
from types import SimpleNamespace

import mpmath
import numpy as np

import icp_cases as K
from kfx.abi import Pose

f32 = np.float32
THR = Fraction(1e-15)  # the exact value of the double the code compares with
EPS = 2.220446049250313e-16
X_BOUND_C = 3.3
ULP1 = 2.0 ** -23  # one float32 ulp of 1.0f
mpmath.mp.dps = 60


# --------------------------------------------------------------------------
# the exact reference

def unpack(sums):
    """A (6 x 6) and b as Fractions from the 27 integer sums (rigid_icp.cu:156-165)."""
    A = [[Fraction(0)] * 6 for _ in range(6)]
    b = [Fraction(0)] * 6
    s = 0
    for i in range(6):
        for j in range(i, 7):
            v = Fraction(int(sums[s]), 2 ** 32)
            s += 1
            if j == 6:
                b[i] = v
            else:
                A[i][j] = A[j][i] = v
    return A, b


def _eliminate(M):
    """Fraction Gauss-Jordan with full pivoting of a 6 x 7 matrix: (rank, det of the 6 x 6 part, x or None)."""
    M = [row[:] for row in M]
    n = 6
    cols = list(range(n))
    det = Fraction(1)
    rank = 0
    for k in range(n):
        piv = next(((i, j) for i in range(k, n) for j in range(k, n) if M[i][j] != 0), None)
        if piv is None:
            det = Fraction(0)
            break
        i, j = piv
        if i != k:
            M[i], M[k] = M[k], M[i]
            det = -det
        if j != k:
            for r in M:
                r[j], r[k] = r[k], r[j]
            cols[j], cols[k] = cols[k], cols[j]
            det = -det
        det *= M[k][k]
        rank += 1
        for r in range(n):
            if r != k and M[r][k] != 0:
                f = M[r][k] / M[k][k]
                M[r] = [a - f * c for a, c in zip(M[r], M[k])]
    if rank < n:
        return rank, Fraction(0), None
    x = [None] * n
    for k in range(n):
        x[cols[k]] = M[k][6] / M[k][k]
    return rank, det, x


def exact_solve(sums):
    A, b = unpack(sums)
    rank, det, x = _eliminate([A[i] + [b[i]] for i in range(6)])
    P = [r[:3] for r in A[:3]]
    detP = (P[0][0] * (P[1][1] * P[2][2] - P[1][2] * P[2][1]) - P[0][1] * (P[1][0] * P[2][2] - P[1][2] * P[2][0])
            + P[0][2] * (P[1][0] * P[2][1] - P[1][1] * P[2][0]))
    return SimpleNamespace(A=A, b=b, rank=rank, det=det, detP=detP, x=x, fail=abs(det) < THR,
                           ratio=float(abs(det) / THR))


def kappa2(sums):
    A, _ = unpack(sums)
    s = np.linalg.svd(np.array([[float(v) for v in r] for r in A]), compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else float("inf")


def narrow(x):
    """float32 of the exact x (correctly rounded: Fraction -> double -> float32 differs from the direct
    rounding only on a double-rounding tie, which the assert excludes)."""
    out = np.array([f32(float(v)) for v in x], f32)
    for v, o in zip(x, out):
        lo, hi = sorted((Fraction(float(np.nextafter(o, f32(-np.inf)))), Fraction(float(np.nextafter(o, f32(np.inf))))))
        assert abs(Fraction(float(o)) - v) <= min(abs(lo - v), abs(hi - v))
    return out


def theta_mp(rv):
    return mpmath.sqrt(sum(mpmath.mpf(float(v)) ** 2 for v in rv))


def rodrigues_mp(rv):
    """(theta, R as 9 mpf) of the float32 rotation vector; identity below EPS as cv::Rodrigues defines it."""
    th = theta_mp(rv)
    eye = [mpmath.mpf(1 if q % 4 == 0 else 0) for q in range(9)]
    if th < EPS:
        return th, eye
    r = [mpmath.mpf(float(v)) / th for v in rv]
    c, s = mpmath.cos(th), mpmath.sin(th)
    rx = [0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0]
    return th, [c * eye[q] + (1 - c) * r[q // 3] * r[q % 3] + s * rx[q] for q in range(9)]


def r_f32(Rmp):
    return np.array([f32(float(v)) for v in Rmp], f32)


def ulps_of_one(R, Rmp):
    """max |R - Rmp| in float32 ulps of 1.0f."""
    return max(float(abs(mpmath.mpf(float(a)) - b)) for a, b in zip(R, Rmp)) / ULP1


def pose_mul_f32(a, Rb, tb):
    """a * (Rb, tb) in float32, kfo_pose_mul's order: sums from 0.f in ascending k, then + a.t."""
    Ra, ta = np.array(a.R[:], f32), np.array(a.t[:], f32)
    Rb, tb = np.asarray(Rb, f32), np.asarray(tb, f32)
    out = Pose()
    for j in range(3):
        for i in range(3):
            v = f32(0)
            for k in range(3):
                v = f32(v + f32(Ra[3 * j + k] * Rb[3 * k + i]))
            out.R[3 * j + i] = float(v)
        d = f32(0)
        for k in range(3):
            d = f32(d + f32(Ra[3 * j + k] * tb[k]))
        out.t[j] = float(f32(d + ta[j]))
    return out


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding of the exact value


def restate_step(rv):
    """The increment's R as kfo_icp_update computes it from the float32 rv on
    the theta < 0.5 arm (and the identity arm), in Python doubles and numpy
    float32, every operation in the oracle's order.  None at theta >= 0.5
    (libm's sin / cos are not restated)."""
    rv = [float(f32(v)) for v in rv]
    th = math.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2])
    if th < EPS:
        return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], f32)
    if not th < 0.5:
        return None
    x2 = th * th
    ps = -1.0 / 1307674368000.0
    for k in (1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0):
        ps = _fma(ps, x2, k)
    sn = _fma(th, x2 * ps, th)
    pc = -1.0 / 87178291200.0
    for k in (1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -0.5):
        pc = _fma(pc, x2, k)
    c = _fma(x2, pc, 1.0)
    c1, it = 1.0 - c, 1.0 / th
    r = [f32(v * it) for v in rv]
    rrt = [f32(r[q // 3] * r[q % 3]) for q in range(9)]
    z = f32(0)
    rx = [z, -r[2], r[1], r[2], z, -r[0], -r[1], r[0], z]
    out = np.zeros(9, f32)
    for q in range(9):
        e = 1.0 if q % 4 == 0 else 0.0
        out[q] = f32(f32(f32(c * e) + f32(c1 * float(rrt[q]))) + f32(sn * float(rx[q])))
    return out


# --------------------------------------------------------------------------
# maps

def level_intrinsics(w):
    return K.crafted_intrinsics(w, w)


def blank(w):
    I = level_intrinsics(w)
    nan = np.full((w, w, 3), np.nan, f32)
    return SimpleNamespace(I=I, w=w, cur_v=np.zeros((w, w, 3), f32), cur_n=nan, pre_v=np.zeros((w, w, 3), f32),
                           pre_n=np.zeros((w, w, 3), f32), pix=[])


def ray(I, u, v):
    return np.array([(f32(u) - f32(I.cx)) / f32(I.fx), (f32(v) - f32(I.cy)) / f32(I.fy), 1], f32)


def put(L, u, v, z, npre, d, ncur=None):
    """One correspondence on pixel (u, v): the vertex on the pixel's ray at
    depth z (exact), the model vertex d away from it, the model normal npre
    (any length), the current normal ncur (default npre)."""
    vc = (ray(L.I, u, v) * f32(z)).astype(f32)
    assert np.all(vc.astype(np.float64) == ray(L.I, u, v).astype(np.float64) * float(z)), "inexact vertex"
    assert np.isnan(L.cur_n[v, u, 0]), "pixel used twice"
    L.cur_v[v, u] = vc
    L.cur_n[v, u] = np.asarray(npre if ncur is None else ncur, f32)
    L.pre_v[v, u] = (vc + np.asarray(d, f32)).astype(f32)
    L.pre_n[v, u] = np.asarray(npre, f32)
    L.pix.append((u, v))
    return vc


PIX12 = [(2, 3), (29, 4), (5, 27), (27, 28), (15, 2), (3, 16), (28, 15), (16, 29), (10, 10), (21, 11), (11, 21), (22, 22)]
DEPTH12 = [0.75, 4.0, 1.5, 3.0, 2.0, 1.0, 2.5, 3.5, 1.25, 0.875, 2.75, 1.75]
NORMAL12 = [(0, 0, -1), (0.6, 0, -0.8), (0, -0.6, -0.8), (-0.6, 0, -0.8), (0, 0.6, -0.8), (0.8, 0, -0.6),
            (0, 0.8, -0.6), (-0.48, 0.6, -0.64), (0.36, -0.48, -0.8), (-0.8, 0, -0.6), (0, -0.8, -0.6), (0.48, 0.64, -0.6)]
AXIS = np.array([0.3, 1.0, -0.2]) / np.linalg.norm([0.3, 1.0, -0.2])
TDIR = np.array([0.02, -0.01, 0.03])


def twist(theta, axis=AXIS, tdir=TDIR):
    return np.concatenate([theta * np.asarray(axis, float), theta * np.asarray(tdir, float)])


def corr12(w=32, variant=0, depth_scale=1.0):
    """The twelve healthy correspondences at image side w: (u, v, depth, unit normal); variant
    rotates the depths and normals over the pixels, so levels get different systems."""
    m = w // 32
    out = []
    for k, (u, v) in enumerate(PIX12):
        out.append((u * m + variant % m, v * m + (variant // 2) % m, DEPTH12[(k + 5 * variant) % 12] * depth_scale,
                    np.array(NORMAL12[(k + 7 * variant) % 12], float)))
    return out


def system12(w=32, variant=0, x=None, depth_scale=1.0, nscale=1.0, scales=None, corr=None):
    """The healthy system: residuals r_k = row_k . x (unit normals) laid along the
    normals, model normals f32(scale_k) * n_k (scale_k = nscale unless `scales` gives it)."""
    L = blank(w)
    x = np.zeros(6) if x is None else np.asarray(x, float)
    for k, (u, v, z, n) in enumerate(corr12(w, variant, depth_scale) if corr is None else corr):
        vc = ray(L.I, u, v).astype(float) * z
        r = float(np.cross(vc, n) @ x[:3] + n @ x[3:])
        s = f32(nscale if scales is None else scales[k])
        nf = n.astype(f32)
        put(L, u, v, z, (s * nf).astype(f32), (f32(r) * nf).astype(f32), ncur=nf)
    return L


def fit_depth_scale(x, corr_fn, limit=0.9):
    """The largest power of two <= 1 that keeps every residual of twist x within `limit`."""
    s = 1.0
    while True:
        worst = 0.0
        for u, v, z, n in corr_fn(s):
            vc = ray(level_intrinsics(32), u, v).astype(float) * z
            worst = max(worst, abs(float(np.cross(vc, n) @ x[:3] + n @ x[3:])))
        if worst <= limit:
            return s
        s /= 2


def sums_of(L, pose=None, dist=0.015, deg=30.0):
    return K.accumulate_np(L.cur_v, L.cur_n, L.pre_v, L.pre_n, L.I, pose or Pose.identity(), dist, K.sinf_deg(deg))


def _single(name, cls, L, dist=0.015, deg=30.0, **meta):
    return SimpleNamespace(name=name, cls=cls, levels=[L], size=L.w, dist=dist, deg=deg, iters=(1, 0, 0, 0), **meta)


# ---- theta arms

def theta_case(name, theta):
    x = twist(theta)
    s = fit_depth_scale(x, lambda s: corr12(32, 0, s))
    return _single(name, "theta", system12(32, 0, x, depth_scale=s), dist=1.0, theta_about=theta,
                   side=("ge" if theta >= 0.5 else "lt"))


def sym12(depth_scale):
    """Six correspondences and their images under the half turn about the optical
    axis, (u, v) -> (31 - u, 31 - v), n -> (-nx, -ny, nz): products between the
    {c_z, n_z, residual} entries and the {c_x, c_y, n_x, n_y} entries cancel in
    pairs exactly, so with equal residuals in a pair x_0 = x_1 = x_3 = x_4 = 0
    exactly (signed zeros on oracle and device) and theta = |float32(x_2)|."""
    base = [(2, 3, 3.0, (0.6, 0, -0.8)), (5, 27, 2.0, (0, 0.8, -0.6)), (12, 6, 1.0, (-0.48, 0.6, -0.64)),
            (9, 20, 4.0, (0.8, 0, -0.6)), (14, 13, 1.5, (0.36, -0.48, -0.8)), (6, 12, 2.5, (0, -0.6, -0.8))]
    out = []
    for u, v, z, n in base:
        out.append((u, v, z * depth_scale, np.array(n, float)))
        out.append((31 - u, 31 - v, z * depth_scale, np.array([-n[0], -n[1], n[2]], float)))
    return out


def theta_rung_case(name, target):
    """theta exactly the float32 `target`: a rotation about the optical axis on
    sym12.  The residual scale brings the exact x_2 within a few float32 ulps (the
    model vertices' own float32 grid allows no better); then single model
    coordinates of a pair move by one ulp each, mirrored, keeping every move that
    brings x_2 closer, until float32 of the exact x_2 is the target."""
    target = f32(target)
    corr = sym12(0.5)
    guess = float(target)
    for _ in range(3):
        L = system12(32, 0, [0, 0, guess, 0, 0, 0.01], corr=corr)
        got = float(exact_solve(sums_of(L, dist=1.0).sums).x[2])
        guess *= float(target) / got
    L = system12(32, 0, [0, 0, guess, 0, 0, 0.01], corr=corr)
    rng = np.random.default_rng(int(target.view(np.uint32)))
    e = exact_solve(sums_of(L, dist=1.0).sums)
    for _ in range(600):
        if f32(float(e.x[2])) == target:
            assert e.x[0] == 0 and e.x[1] == 0 and e.x[3] == 0 and e.x[4] == 0
            return _single(name, "theta_rung", L, dist=1.0, theta_exact=float(target),
                           side=("ge" if target >= f32(0.5) else "lt"))
        k, comp, up = 2 * int(rng.integers(6)), int(rng.integers(3)), bool(rng.integers(2))
        (u, v), (mu, mv) = L.pix[k], L.pix[k + 1]
        old = L.pre_v[v, u, comp]
        new = np.nextafter(old, f32(np.inf) if up else f32(-np.inf))
        L.pre_v[v, u, comp], L.pre_v[mv, mu, comp] = new, (new if comp == 2 else -new)
        e2 = exact_solve(sums_of(L, dist=1.0).sums)
        if abs(e2.x[2] - Fraction(float(target))) < abs(e.x[2] - Fraction(float(target))):
            e = e2
        else:
            L.pre_v[v, u, comp], L.pre_v[mv, mu, comp] = old, (old if comp == 2 else -old)
    raise AssertionError(("theta rung not reachable", float(target)))


def pure_translation_case():
    """Small dyadic rows whose products are all exact in float32 and in 2^-32
    fixed point, model = current + t: b = A (0, t) exactly, the exact x is (0, t)."""
    L = blank(32)
    t = np.array([2.0 ** -7, -(2.0 ** -8), 2.0 ** -6], f32)
    normals = [(0, 0, -1), (0.5, 0, -1), (0, -0.5, -1), (-0.5, 0.25, -1), (0.25, 0.5, -0.5), (-1, 0, -0.5),
               (0, 1, -0.5), (0.5, -0.5, -1), (-0.25, -0.5, -1), (1, 0.5, -0.5), (0, 0, -0.5), (-0.5, 1, -1)]
    for (u, v), z, n in zip(PIX12, [1, 2, 1, 2, 1, 0.5, 2, 1, 0.5, 1, 2, 0.5], normals):
        put(L, u, v, z, np.array(n, f32), t)
    return _single("pure_translation", "tiny_theta", L, dist=0.03, t=t)


# ---- det ladder

_base_det = {}


def _det_at(scales):
    L = system12(32, 0, twist(0.002), scales=scales)
    return L, exact_solve(sums_of(L).sums)


def det_scale_for(ratio):
    """All twelve model normals scaled by one float32 s with exact det near ratio * 1e-15."""
    if "d0" not in _base_det:
        _base_det["d0"] = float(_det_at([1.0] * 12)[1].det)
    s = (ratio * 1e-15 / _base_det["d0"]) ** (1.0 / 12)
    for _ in range(3):
        e = _det_at([s] * 12)[1]
        s *= (ratio / e.ratio) ** (1.0 / 12)
    # one float32 step of s moves the det by 7e-7 relative, the products' 2^-32 rounding by about as much
    near = [float(K.step(f32(s), j)) for j in range(-6, 7)]
    return min(near, key=lambda v: abs(_det_at([v] * 12)[1].ratio / ratio - 1.0))


def det_case(name, ratio):
    L, e = _det_at([det_scale_for(ratio)] * 12)
    return _single(name, "det", L, want_ratio=ratio, fails=ratio < 1)


def det_closest_cases():
    """On either side of the threshold, the closest exact det a search over
    float32 steps of one model normal's length reaches (the eighth's, all three of
    whose components are non-zero; the other eleven at
    the scale of ratio 1)."""
    if "closest" in _base_det:
        return _base_det["closest"]
    s = f32(det_scale_for(1.0))

    def at(j):
        L, e = _det_at([float(s)] * 7 + [float(K.step(s, j))] + [float(s)] * 4)
        return L, e

    lo, hi = -(2 ** 16), 2 ** 16
    assert at(lo)[1].fail and not at(hi)[1].fail
    while hi - lo > 1:  # the det grows with the length up to the fixed-point noise: a crossing, then a scan round it
        mid = (lo + hi) // 2
        if at(mid)[1].fail:
            lo = mid
        else:
            hi = mid
    best = {True: None, False: None}
    for j in range(lo - 96, lo + 97):
        L, e = at(j)
        d = abs(e.ratio - 1.0)
        if best[e.fail] is None or d < best[e.fail][0]:
            best[e.fail] = (d, j, L, e)
    below = _single("det_closest_below", "det", best[True][2], want_ratio=best[True][3].ratio, fails=True, closest=True)
    above = _single("det_closest_above", "det", best[False][2], want_ratio=best[False][3].ratio, fails=False,
                    closest=True)
    _base_det["closest"] = (below, above)
    return below, above


# ---- exactly singular

def radial_case():
    """npre = ncur = -2 vcur: vcur x npre = 0 exactly, P = Q = 0, 1 / det P = inf, the products NaN."""
    L = blank(32)
    for u, v, z, n in corr12(32, 0):
        vc = ray(L.I, u, v) * f32(z)
        put(L, u, v, z, (f32(-2) * vc).astype(f32), (f32(2.0 ** -9) * vc).astype(f32))
    return _single("radial", "singular", L, rank=3, fails=True)


def zero_case():
    return _single("zero_sums", "singular", blank(32), rank=0, fails=True)


def rank5_case():
    """Eight correspondences at depth 2 m with axis-aligned model normals: A has exact rank 5, P is regular."""
    L = blank(32)
    normals = [(0, 0, -1), (1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (1, 0, 0), (0, 1, 0)]
    for (u, v), n in zip(PIX12[:8], normals):
        put(L, u, v, 2.0, np.array(n, f32), (f32(2.0 ** -9) * np.array(n, f32)).astype(f32))
    return _single("rank5_depth2", "rank5", L, rank=5)


def two_planes_case():
    c = K.gen_degenerate("two_planes", level_intrinsics(32))
    L = SimpleNamespace(I=c.I, w=32, cur_v=c.cur_v, cur_n=c.cur_n, pre_v=c.pre_v, pre_n=c.pre_n, pix=[])
    return _single("two_planes", "rank5", L, rank=5)


# ---- conditioning

CONE = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1), (0.5, 1), (-1, 0.5), (1, -0.5), (-0.5, -1)]


def cone_level(w, eps, scale, x, variant=0, dmax=None):
    """Model normals scale * (eps a, eps b, -1): a cone of half-angle ~eps round
    the optical axis, so the lateral translation and the roll are held by terms
    of order eps^2 only; residuals row . x laid along the normals."""
    L = blank(w)
    for k, (u, v, z, _) in enumerate(corr12(w, variant)):
        a, b = CONE[k]
        n = np.array([eps * a, eps * b, -1.0]) * scale
        nf = n.astype(f32)
        vc = ray(L.I, u, v).astype(float) * z
        r = float(np.cross(vc, nf.astype(float)) @ x[:3] + nf.astype(float) @ x[3:])
        d = (f32(r / float(nf.astype(float) @ nf.astype(float))) * nf).astype(f32)
        assert dmax is None or float(np.linalg.norm(d)) < dmax
        put(L, u, v, z, nf, d)
    return L


def cone_case(name, eps, scale, about):
    x = np.array([0.01, -0.02, 0.015, 0.01, 0.02, -0.005])
    return _single(name, "conditioning", cone_level(32, eps, scale, x), dist=1.0, kappa_about=about)


# ---- the level loop: 128x128 / 64x64 / 32x32, levels[l] is pyramid level l

SIDES = (128, 64, 32)
SMALL = 2.0e-4  # twists that keep every projection on its pixel at all three sizes


def healthy_levels(zero=()):
    return [system12(SIDES[l], l, None if l in zero else twist(SMALL * (l + 1), tdir=TDIR * (1 + l))) for l in range(3)]


def _loop(name, levels, iters, dist=0.015, deg=30.0, **meta):
    return SimpleNamespace(name=name, cls="loop", levels=levels, size=128, dist=dist, deg=deg,
                           iters=tuple(iters) + (0,), **meta)


def lateral_level():
    """Level 0 of fail_second_iteration: a cone of normals whose residuals (all
    within the default 15 mm) ask for half a metre sideways; the step carries every
    correspondence past the distance gate and off its pixel, the next sums are 0."""
    return cone_level(128, 0.02, 1.0, np.array([0, 0, 0, 0.5, 0, 0.0]), dmax=0.015)


def _surface(I):
    """A dense smooth model: depth 2 + 0.3 cos(2.5 ax) + 0.25 sin(3 ay + 0.4) along the ray (ax, ay, 1)."""
    w = I.width
    u, v = np.meshgrid(np.arange(w, dtype=float), np.arange(w, dtype=float))
    ax, ay = (u - I.cx) / I.fx, (v - I.cy) / I.fy
    z = 2 + 0.3 * np.cos(2.5 * ax) + 0.25 * np.sin(3 * ay + 0.4)
    zx, zy = -0.75 * np.sin(2.5 * ax), 0.75 * np.cos(3 * ay + 0.4)
    a = np.stack([ax, ay, np.ones_like(ax)], -1)
    du = zx[..., None] * a + z[..., None] * np.array([1.0, 0, 0])
    dv = zy[..., None] * a + z[..., None] * np.array([0, 1.0, 0])
    n = np.cross(du, dv)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n *= -np.sign(n[..., 2:3])
    return z[..., None] * a, n


def _rot(axis, angle):
    ax = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def chain_level(w, angle):
    """The dense model seen from a camera turned by `angle` about AXIS through
    (0, 0, 2) and shifted a little: 36 model points, each stored (in the current
    camera's frame) on the current pixel it projects to."""
    L = blank(w)
    pv, pn = _surface(L.I)
    L.pre_v[:], L.pre_n[:] = pv.astype(f32), pn.astype(f32)
    R, c, tau = _rot(AXIS, angle), np.array([0, 0, 2.0]), np.array([0.01, -0.02, 0.015]) * angle
    m = w // 32
    for gy in range(6):
        for gx in range(6):
            u, v = (6 + 4 * gx) * m + (gy % m), (6 + 4 * gy) * m + (gx % m)
            p, n = pv[v, u], pn[v, u]
            q = R.T @ (p - c - tau) + c  # p = R (q - c) + c + tau
            uu, vv = int(np.rint(q[0] / q[2] * L.I.fx + L.I.cx)), int(np.rint(q[1] / q[2] * L.I.fy + L.I.cy))
            if not (0 <= uu < w and 0 <= vv < w and np.isnan(L.cur_n[vv, uu, 0])):
                continue  # outside the current image, or the pixel is taken
            L.cur_v[vv, uu], L.cur_n[vv, uu] = q.astype(f32), (R.T @ n).astype(f32)
            L.pix.append((uu, vv))
    assert len(L.pix) >= 24
    return L


def chain_case(name, angles):
    return _loop(name, [chain_level(SIDES[l], angles[l]) for l in range(3)], (1, 1, 1), dist=1.0, deg=60.0, chain=True)


# --------------------------------------------------------------------------
# the table

HALF = f32(0.5)


def case_table():
    """name -> builder.  `stop` of a loop case: (level, iteration) of the failing solve, or None."""
    t = {}
    t["theta_zero"] = lambda: _single("theta_zero", "theta", system12(32, 0), theta_about=0.0, side="zero")
    for nm, th in (("theta_1e-6", 1e-6), ("theta_0.1", 0.1), ("theta_0.4", 0.4), ("theta_0.7", 0.7),
                   ("theta_1.5", 1.5), ("theta_above_pi", 3.3)):
        t[nm] = (lambda nm=nm, th=th: theta_case(nm, th))
    for k in (-3, -2, -1, 0, 1, 2):
        nm = f"theta_half{k:+d}ulp"
        t[nm] = (lambda nm=nm, k=k: theta_rung_case(nm, K.step(HALF, k)))
    t["pure_translation"] = pure_translation_case
    for nm, r in (("det_half", 0.5), ("det_double", 2.0), ("det_1-1e-3", 1 - 1e-3), ("det_1+1e-3", 1 + 1e-3)):
        t[nm] = (lambda nm=nm, r=r: det_case(nm, r))
    t["det_closest_below"] = lambda: det_closest_cases()[0]
    t["det_closest_above"] = lambda: det_closest_cases()[1]
    t["radial"] = radial_case
    t["zero_sums"] = zero_case
    t["rank5_depth2"] = rank5_case
    t["two_planes"] = two_planes_case
    t["cond_1e2"] = lambda: cone_case("cond_1e2", 0.5, 1.0, 1e2)
    t["cond_1e6"] = lambda: cone_case("cond_1e6", 2.0 ** -8, 8.0, 1e6)
    t["cond_1e10"] = lambda: cone_case("cond_1e10", 2.0 ** -15, 64.0, 1e10)
    t["fail_coarsest"] = lambda: _loop("fail_coarsest", healthy_levels()[:2] + [radial_case().levels[0]], (1, 1, 1),
                                       stop=(2, 0))
    t["fail_middle"] = lambda: _loop("fail_middle", [healthy_levels()[0], blank(64), healthy_levels()[2]], (1, 1, 1),
                                     stop=(1, 0))
    t["fail_second_iteration"] = lambda: _loop("fail_second_iteration",
                                               [lateral_level()] + healthy_levels(zero=(1, 2))[1:], (2, 1, 1),
                                               stop=(0, 1))
    for it in ((2, 0, 3), (0, 0, 1), (1, 1, 0), (0, 0, 0)):
        nm = "iters_%d%d%d" % it
        t[nm] = (lambda nm=nm, it=it: _loop(nm, healthy_levels(), it, stop=None))
    t["chain"] = lambda: chain_case("chain", CHAIN_ANGLES)
    t["chain_last_ge_half"] = lambda: chain_case("chain_last_ge_half", CHAIN_ANGLES_BIG)
    return t


CHAIN_ANGLES = (0.36, 0.24, 0.12)      # level 0, 1, 2: each level is asked for about 0.12 rad more
CHAIN_ANGLES_BIG = (1.0, 0.24, 0.12)   # level 0 for about 0.76 rad more: its step is on the libm / ocml arm
SINGLE = [n for n in case_table() if not n.startswith(("fail_", "iters_", "chain"))]
LOOP = [n for n in case_table() if n not in SINGLE]
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = case_table()[name]()
    return _cache[name]


def level_I(c, l):
    return c.levels[l].I


def replay_ref(c):
    """The loop on the reference alone: per iteration the restated sums, the
    exact solve and decision, float32(x), the mpmath step rounded to float32 and
    the float32 composition.  Returns the iterations (level, it, sums, exact,
    theta, pose_in, accumulate_np's result), the stop (level, it) or None, the pose."""
    pose, its = Pose.identity(), []
    for l in reversed(range(len(c.levels))):
        L = c.levels[l]
        for it in range(c.iters[l]):
            r = sums_of(L, pose, c.dist, c.deg)
            e = exact_solve(r.sums)
            rec = SimpleNamespace(level=l, it=it, sums=K.sums_i64(r.sums), exact=e, pose_in=pose, acc=r, theta=None)
            its.append(rec)
            if e.fail:
                return its, (l, it), pose
            xf = narrow(e.x)
            rec.theta, Rmp = rodrigues_mp(xf[:3])
            pose = pose_mul_f32(pose, r_f32(Rmp), xf[3:])
    return its, None, pose


# --------------------------------------------------------------------------
# the oracle's loop, for the tests (nothing above uses the oracle)

def oracle_loop(c):
    """kfo_icp_accumulate / kfo_icp_update as kfo_icp_track chains them, per
    iteration: level, it, sums, status, pose_in, pose_out, x and the increment
    alone (the update applied to the identity).  Returns (iterations, status, pose)."""
    import oracle as O
    pose, its = Pose.identity(), []
    ang = float(K.sinf_deg(c.deg))
    for l in reversed(range(len(c.levels))):
        L = c.levels[l]
        for it in range(c.iters[l]):
            sums = O.icp_accumulate(L.cur_v, L.cur_n, L.pre_v, L.pre_n, L.I, pose, c.dist, ang)
            st, out, x = O.icp_update(sums, pose)
            inc = O.icp_update(sums, Pose.identity())[1]
            its.append(SimpleNamespace(level=l, it=it, sums=sums, status=st, pose_in=pose, pose_out=out, x=x, inc=inc))
            if st:
                return its, 1, pose
            pose = out
    return its, 0, pose
