"""Known-answer tests that pin the CPU oracle (oracle/kfx_oracle.cpp).

The reference ships no tests or golden vectors.  Its per-thread kernels are
compiled for the host and compared with the oracle bit for bit in
test_ref_parity.py (integrate, raycast, vertex / normal / resize / render
kernels, level intrinsics, the ICP correspondence rows).  What that build
cannot reach stays pinned here alone: pyrDown and the bilateral filter
(OpenCV's), the ICP solve and Rodrigues step, FullScan6 (warp-synchronous),
the pipeline glue and the pose text.  The KATs pin all of the oracle by:
  * closed-form answers (planes, identical frames, constants);
  * an independent vectorised numpy restatement of the OpenCV pieces;
  * tracking against the analytic ground truth of the synthetic scene;
  * the reference's only data artifact, doc/poses.txt (output format).
"""
import math

import numpy as np
import pytest

from kfx import synth
from kfx.abi import Intrinsics, Pose, default_params, fptr

f32 = np.float32


def np_reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def np_pyr_down(src):
    """Independent numpy restatement of cv::cuda::pyrDown (float32, same op order)."""
    src = src.astype(np.float32)
    h, w = src.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    k = [f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625)]
    rows = [np_reflect101(2 * np.arange(dh) + j - 2, h) for j in range(5)]
    col = k[0] * src[rows[0], :]
    for j in range(1, 5):
        col = col + k[j] * src[rows[j], :]
    cols = [np_reflect101(2 * np.arange(dw) + j - 2, w) for j in range(5)]
    out = k[0] * col[:, cols[0]]
    for j in range(1, 5):
        out = out + k[j] * col[:, cols[j]]
    return out


def test_expf_accuracy(oracle_lib):
    xs = np.concatenate([np.linspace(-86.0, 0.0, 4001), -np.logspace(-8, 1.9, 500)]).astype(np.float32)
    got = np.array([oracle_lib.expf(float(x)) for x in xs], dtype=np.float64)
    ref = np.exp(xs.astype(np.float64))
    rel = np.abs(got - ref) / ref
    assert rel.max() < 3e-7
    assert oracle_lib.expf(0.0) == 1.0
    assert oracle_lib.expf(-86.5) == 0.0 and oracle_lib.expf(-1e30) == 0.0


def test_pyr_down_matches_numpy_restatement(oracle_lib):
    rng = np.random.default_rng(0)
    for (h, w) in [(48, 64), (31, 45), (120, 160), (5, 7)]:
        src = (rng.random((h, w)) * 4000).astype(np.float32)
        src[rng.random((h, w)) < 0.1] = 0
        a = oracle_lib.pyr_down(src)
        b = np_pyr_down(src)
        assert a.shape == ((h + 1) // 2, (w + 1) // 2)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_pyr_down_constant(oracle_lib):
    src = np.full((60, 80), 1500.0, np.float32)
    assert np.all(oracle_lib.pyr_down(src) == 1500.0)


def test_bilateral_properties(oracle_lib):
    # constant image stays (almost) constant; an isolated step edge is kept
    c = np.full((40, 50), 1234.0, np.float32)
    out = oracle_lib.bilateral(c)
    assert np.allclose(out, 1234.0, rtol=1e-6)
    step = np.full((40, 50), 1000.0, np.float32)
    step[:, 25:] = 2000.0
    out = oracle_lib.bilateral(step)
    assert np.allclose(out[:, :24], 1000.0, rtol=1e-6) and np.allclose(out[:, 26:], 2000.0, rtol=1e-6)
    # zero (invalid) pixels surrounded by valid depth stay zero; valid pixels ignore zeros
    z = np.full((20, 20), 1500.0, np.float32)
    z[10, 10] = 0.0
    out = oracle_lib.bilateral(z)
    assert out[10, 10] == 0.0 and np.allclose(out[10, 11], 1500.0, rtol=1e-6)


def test_bilateral_matches_python_loop(oracle_lib):
    rng = np.random.default_rng(1)
    src = (1000 + rng.random((9, 11)) * 40).astype(np.float32)
    out = oracle_lib.bilateral(src)
    h, w = src.shape
    sh, ch = f32(-0.5) / f32(100.0), f32(-0.5) / f32(100.0)
    for y in range(h):
        for x in range(w):
            c = src[y, x]
            s1 = s2 = f32(0)
            for cy in range(y - 2, y + 3):
                for cx in range(x - 2, x + 3):
                    sp = (x - cx) ** 2 + (y - cy) ** 2
                    if sp > 4:
                        continue
                    v = src[int(np_reflect101(cy, h)), int(np_reflect101(cx, w))]
                    d = abs(v - c)
                    wgt = f32(oracle_lib.expf(float(f32(sp) * sh + (d * d) * ch)))
                    s1 = f32(s1 + wgt * v)
                    s2 = f32(s2 + wgt)
            assert out[y, x] == f32(s1 / s2)


@pytest.mark.parametrize("with_nan", [False, True])
@pytest.mark.parametrize("ksz", [1, 6, 15])
def test_bilateral_window_sizes_match_python_loop(ksz, with_nan, oracle_lib):
    """The loop of test_bilateral_matches_python_loop at the window sizes the
    GPU parity tests rest on (the smallest, an even one, the largest): taps
    [y - r, y - r + ksz) with r = ksz // 2, cut at space2 > r * r, on a 10x9
    image that holds a zero pixel and, in one variant, a NaN pixel (compared by
    position: it poisons every window that reaches it)."""
    rng = np.random.default_rng(3)
    src = (1000 + rng.random((10, 9)) * 40).astype(np.float32)
    src[4, 5] = 0.0
    if with_nan:
        src[7, 2] = np.nan
    out = oracle_lib.bilateral(src, ksz=ksz, sigma_color=40.0, sigma_spatial=3.0)
    h, w = src.shape
    r = ksz // 2
    assert w > r and h > r  # one reflection reaches every tap
    sh, ch = f32(-0.5) / f32(3.0 * 3.0), f32(-0.5) / f32(40.0 * 40.0)
    n_nan = 0
    with np.errstate(invalid="ignore"):
        for y in range(h):
            for x in range(w):
                c = src[y, x]
                s1 = s2 = f32(0)
                for cy in range(y - r, y - r + ksz):
                    for cx in range(x - r, x - r + ksz):
                        sp = (x - cx) ** 2 + (y - cy) ** 2
                        if sp > r * r:
                            continue
                        v = src[int(np_reflect101(cy, h)), int(np_reflect101(cx, w))]
                        d = abs(v - c)
                        wgt = f32(oracle_lib.expf(float(f32(sp) * sh + (d * d) * ch)))
                        s1 = f32(s1 + wgt * v)
                        s2 = f32(s2 + wgt)
                want = f32(s1 / s2)
                if np.isnan(want):
                    n_nan += 1
                    assert np.isnan(out[y, x]), (y, x)
                else:
                    assert out[y, x] == want, (y, x)
    if with_nan:
        # the NaN reaches exactly the pixels whose disc holds it (ksz 1: itself)
        reach = np.zeros((h, w), bool)
        for y in range(h):
            for x in range(w):
                for cy in range(y - r, y - r + ksz):
                    for cx in range(x - r, x - r + ksz):
                        if (x - cx) ** 2 + (y - cy) ** 2 <= r * r and \
                                (int(np_reflect101(cy, h)), int(np_reflect101(cx, w))) == (7, 2):
                            reach[y, x] = True
        assert np.array_equal(np.isnan(out), reach) and n_nan == reach.sum() > 0
    else:
        assert n_nan == 0 and not np.isnan(out).any()
        assert out[4, 5] == 0.0  # a zero pixel keeps only its own tap (the others' weights underflow to 0)


def _feq(a, b):
    """Bit equality of float32 arrays, NaNs compared by position."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(np.where(na, f32(0), a).view(np.uint32), np.where(nb, f32(0), b).view(np.uint32))


@pytest.mark.parametrize("height", [1, 2, 4])
def test_preprocess_levels_follow_pyramid_height(height, oracle_lib):
    """kfo_preprocess returns pyramid_height levels, each equal to the pieces
    called one by one: pyr_down of the raw level below, bilateral, truncation,
    vertex map, normal map (kinectfusion.cpp:48-76)."""
    w, h = 64, 48
    rng = np.random.default_rng(4)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 1500.0 + 300.0 * np.sin(0.2 * x) + 250.0 * np.cos(0.3 * y) + rng.normal(0.0, 5.0, (h, w))
    d[rng.random((h, w)) < 0.03] = 0.0
    d[10:14, 20:30] = 5200.0  # beyond dfilter_dist: cut
    d = d.astype(np.float32)
    intr = Intrinsics(w, h, 52.0, 50.0, 30.25, 24.5)
    p = default_params(dims=64, range_m=2.048)
    p.pyramid_height = height
    p.bfilter_kernel_size = 7
    p.bfilter_spatial_sigma = 3.0
    p.bfilter_color_sigma = 40.0
    ds, vs, ns = oracle_lib.preprocess(d, intr, p)
    assert len(ds) == len(vs) == len(ns) == height
    raw = d
    for l in range(height):
        if l > 0:
            raw = oracle_lib.pyr_down(raw)
        li = intr.level(l)
        assert raw.shape == (li.height, li.width) == (h >> l, w >> l)
        dm = oracle_lib.bilateral(raw, ksz=7, sigma_color=40.0, sigma_spatial=3.0)
        oracle_lib.lib().kfo_depth_truncation(fptr(dm), dm.size, p.dfilter_dist)
        vm = oracle_lib.vertex_map(dm, li)
        nm = oracle_lib.normal_map(vm)
        assert _feq(ds[l], dm), l
        assert _feq(vs[l], vm), l
        assert _feq(ns[l], nm), l
        assert (dm > 0).any() and (np.isfinite(nm).all(-1) & (nm != 0).any(-1)).any()
    assert (ds[0][10:14, 20:30] == 0).all()  # the cut took place


def plane_params(dims=64, L=2.0):
    p = default_params(dims=dims, range_m=L)
    return p


def test_plane_preprocess_closed_form(oracle_lib):
    intr = Intrinsics(160, 120, 131.25, 131.25, 79.5, 59.5)
    depth = np.full((120, 160), 1500.0, np.float32)
    p = plane_params()
    ds, vs, ns = oracle_lib.preprocess(depth, intr, p)
    for l in range(3):
        li = intr.level(l)
        assert np.allclose(ds[l], 1.5, rtol=1e-6)
        u = np.arange(li.width, dtype=np.float32)[None, :]
        v = np.arange(li.height, dtype=np.float32)[:, None]
        z = ds[l]
        assert np.allclose(vs[l][..., 0], z * (u - f32(li.cx)) / f32(li.fx), atol=1e-6)
        assert np.allclose(vs[l][..., 1], z * (v - f32(li.cy)) / f32(li.fy), atol=1e-6)
        n = ns[l]
        assert np.all(n[0] == 0) and np.all(n[-1] == 0) and np.all(n[:, 0] == 0) and np.all(n[:, -1] == 0)
        inner = n[1:-1, 1:-1]
        assert np.allclose(inner[..., 2], -1.0, atol=1e-6) and np.allclose(inner[..., :2], 0.0, atol=1e-6)


def test_normals_nan_on_invalid_neighbour(oracle_lib):
    intr = Intrinsics(32, 32, 30.0, 30.0, 15.5, 15.5)
    d = np.full((32, 32), 1.0, np.float32)
    d[10, 10] = 0.0
    v = oracle_lib.vertex_map(d, intr)
    n = oracle_lib.normal_map(v)
    for (y, x) in [(10, 9), (10, 11), (9, 10), (11, 10)]:
        assert np.all(np.isnan(n[y, x]))  # A8: normalize(0) = NaN
    assert not np.any(np.isnan(n[10, 10]))  # own depth is not checked (image_process.cu:71)


def test_resize_closed_form(oracle_lib):
    rng = np.random.default_rng(2)
    vb = rng.random((8, 10, 3)).astype(np.float32)
    nb = rng.random((8, 10, 3)).astype(np.float32)
    vb[0, 0, 0] = np.nan
    vs, ns = oracle_lib.resize_points_normals(vb, nb)
    assert np.all(vs[0, 0] == 0) and np.all(ns[0, 0] == 0)
    q = vb[2:4, 4:6].reshape(4, 3)
    exp = ((q[0] + q[1]) + q[2] + q[3]) * f32(0.25)
    assert np.array_equal(vs[1, 2], exp)


def test_icp_identical_frames_zero_increment(oracle_lib):
    intr = synth.Intrinsics.qqvga()
    bgr, dep, gt = synth.sequence(1, intr)
    I = Intrinsics.from_any(intr)
    p = default_params(dims=64, range_m=2.048)
    ds, vs, ns = oracle_lib.preprocess(dep[0].astype(np.float32), I, p)
    sums = oracle_lib.icp_accumulate(vs[0], ns[0], vs[0], ns[0], I, Pose.identity())
    # b = sum row_i * n.(d - s) is exactly 0 when s == d
    b_idx = [6, 12, 17, 21, 24, 26]
    assert all(sums[k] == 0 for k in b_idx)
    assert sums[0] > 0
    st, pose, x = oracle_lib.icp_update(sums, Pose.identity())
    assert st == 0 and np.all(x == 0)
    assert np.array_equal(pose.matrix(), np.eye(4, dtype=np.float32))


def test_icp_block_solve_matches_numpy(oracle_lib):
    """The 3+3 block solve (D: instead of cv::solve(DECOMP_SVD)) on random
    normal equations A = JᵀJ, b = Jᵀr given as the 2^-32 fixed-point sums:
    x agrees with numpy's LU solve of the same A, b to 1e-9 relative."""
    rng = np.random.default_rng(11)
    iu = [(i, j) for i in range(6) for j in range(i, 7)]
    for trial in range(20):
        J = rng.normal(size=(400, 6)) * rng.uniform(0.05, 2.0, size=6)
        r = rng.normal(size=400) * 1e-3
        A = J.T @ J
        b = J.T @ r
        Ab = np.concatenate([A, b[:, None]], 1)
        sums = np.array([round(Ab[i, j] * 2.0 ** 32) for i, j in iu], np.int64)
        Aq = np.zeros((6, 7))
        for k, (i, j) in enumerate(iu):
            Aq[i, j] = sums[k] / 2.0 ** 32
            if j < 6:
                Aq[j, i] = Aq[i, j]
        st, _, x = oracle_lib.icp_update(sums, Pose.identity())
        xe = np.linalg.solve(Aq[:, :6], Aq[:, 6])
        assert st == 0
        assert np.abs(x - xe).max() <= 1e-9 * np.abs(xe).max(), trial


def test_icp_det_threshold_matches_lu(oracle_lib):
    """The tracking-failure test |det A| < 1e-15 (icp_registration.cpp:35-37,
    cv::determinant) on the block solve's det P * det S decides as the LU
    determinant of the same fixed-point A does, for positive semidefinite
    systems (A = JᵀJ) whose determinant spans 1e-18 .. 1e-12 and for rank-
    deficient ones; only determinants within 1e-6 of the threshold are not
    compared (the two products round differently there).  For PSD A a singular
    rotation block P implies a singular A, so the block form never divides by
    a zero det P of a trackable system."""
    rng = np.random.default_rng(5)
    iu = [(i, j) for i in range(6) for j in range(i, 7)]
    decided = fails = 0
    for trial in range(400):
        Qm, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        lam = np.exp(rng.normal(size=6) * 1.5)
        if trial % 8 == 0:
            lam[rng.integers(6)] = 0.0  # rank-deficient: det 0
        else:
            lam *= (10.0 ** rng.uniform(-18, -12) / np.prod(lam)) ** (1 / 6)
        A = (Qm * lam) @ Qm.T
        b = rng.normal(size=6) * 1e-3
        Ab = np.concatenate([A, b[:, None]], 1)
        sums = np.array([round(Ab[i, j] * 2.0 ** 32) for i, j in iu], np.int64)
        Aq = np.zeros((6, 6))
        for k, (i, j) in enumerate(iu):
            if j < 6:
                Aq[i, j] = Aq[j, i] = sums[k] / 2.0 ** 32
        d = np.linalg.det(Aq)
        st, _, _ = oracle_lib.icp_update(sums, Pose.identity())
        if abs(abs(d) / 1e-15 - 1) < 1e-6:
            continue
        decided += 1
        fails += st
        assert st == int(abs(d) < 1e-15 or np.isnan(d)), (trial, d)
    assert decided >= 390 and 0 < fails < decided


def test_icp_singular_fails(oracle_lib):
    st, _, _ = oracle_lib.icp_update(np.zeros(27, np.int64), Pose.identity())
    assert st == 1  # det < 1e-15 -> tracking fail (icp_registration.cpp:35-37)


def test_icp_recovers_known_motion(oracle_lib):
    """Two measured frames with known relative motion: the coarse-to-fine ICP
    (icp_registration.cpp:16-46) recovers T_prev^-1 T_cur."""
    intr = synth.Intrinsics.vga()
    bgr, dep, gt = synth.sequence(3, intr)
    I = Intrinsics.from_any(intr)
    p = default_params(dims=64, range_m=2.048)
    maps = [oracle_lib.preprocess(dep[k].astype(np.float32), I, p) for k in (1, 2)]
    import ctypes as C
    L = 3
    PA = C.POINTER(C.c_float) * L
    from kfx.abi import fptr
    cam = Pose()
    st = oracle_lib.lib().kfo_icp_track(PA(*[fptr(a) for a in maps[1][1]]), PA(*[fptr(a) for a in maps[1][2]]),
                                        PA(*[fptr(a) for a in maps[0][1]]), PA(*[fptr(a) for a in maps[0][2]]),
                                        C.byref(I), C.byref(p), C.byref(cam))
    assert st == 0
    rel = np.linalg.inv(gt[1]) @ gt[2]
    est = cam.matrix().astype(np.float64)
    assert np.abs(est[:3, 3] - rel[:3, 3]).max() < 1.5e-3
    assert np.abs(est[:3, :3] - rel[:3, :3]).max() < 2e-3


def test_integrate_plane_closed_form(oracle_lib):
    intr = Intrinsics(160, 120, 131.25, 131.25, 79.5, 59.5)
    L, dims = 2.0, 64
    p = plane_params(dims, L)
    vol = oracle_lib.Volume((dims,) * 3, (L,) * 3)
    D = 1.5
    dmap = np.full((120, 160), D, np.float32)
    bgr = np.full((120, 160, 3), 200, np.uint8)
    vol2cam = p.volu_pose  # camera at identity
    nu, nc = oracle_lib.integrate(vol, p.volu_trun_dist, intr, vol2cam, dmap, bgr)
    assert nu > 0 and 0 < nc < nu
    t = vol.tsdf.reshape(dims, dims, dims)  # [z][y][x]
    w = vol.weight.reshape(dims, dims, dims)
    vs = L / dims
    trunc = p.volu_trun_dist
    x = y = dims // 2
    for z in range(1, dims):
        zc = 0.5 + z * vs
        sdf = D - zc  # on-axis: ||vc|| / lambda == vc.z up to rounding
        if sdf >= -trunc + 1e-4:
            assert w[z, y, x] == 1
            assert abs(t[z, y, x] / 32767.0 - min(1.0, sdf / trunc)) < 2e-3
        elif sdf < -trunc - 1e-4:
            assert w[z, y, x] == 0 and t[z, y, x] == 0
    assert np.all(w[0] == 0)  # z = 0 is never updated (tsdf_volume.cu:53)
    c = vol.rgb.reshape(dims, dims, dims, 4)
    band = np.abs(D - (0.5 + np.arange(dims) * vs)) <= trunc / 2 - 1e-4
    zb = np.nonzero(band)[0]
    assert np.all(c[zb, y, x, :3] == 100)  # (1*0 + 200) / 2 (A10: divisor new_w + 1)


def test_raycast_plane(oracle_lib):
    intr = Intrinsics(160, 120, 131.25, 131.25, 79.5, 59.5)
    L, dims = 2.0, 64
    p = plane_params(dims, L)
    vol = oracle_lib.Volume((dims,) * 3, (L,) * 3)
    D = 1.5
    dmap = np.full((120, 160), D, np.float32)
    bgr = np.zeros((120, 160, 3), np.uint8)
    for _ in range(2):
        oracle_lib.integrate(vol, p.volu_trun_dist, intr, p.volu_pose, dmap, bgr)
    cam2vol = oracle_lib.pose_mul(oracle_lib.pose_inv(p.volu_pose), Pose.identity())
    Rinv = cam2vol.matrix()[:3, :3].T
    vmap, nmap = oracle_lib.raycast(vol, intr, cam2vol, Rinv)
    hit = vmap[..., 2] > 0
    assert hit[30:90, 40:120].all()
    vs = L / dims
    z = vmap[hit][:, 2]
    # A3: the crossing lies at ray_len + f*step but the reference takes
    # ray_len - f*step (up to 2 steps toward the camera), and samples are
    # nearest-voxel values, so vertices scatter within ~2 voxels of the plane
    assert np.all(np.abs(z - D) <= 2.5 * vs)
    n = nmap[30:90, 40:120].reshape(-1, 3)
    assert np.mean(np.abs(n[:, 2] + 1.0) < 1e-2) > 0.98


def test_pipeline_tracks_synthetic_sequence(oracle_lib):
    # >= 320x240 so level 2 keeps a 32-row ICP grid (A2: 160x120 -> 40x30 -> 0 rows)
    intr = synth.Intrinsics.qvga()
    N = 8
    bgr, dep, gt = synth.sequence(N, intr)
    p = default_params(dims=128, range_m=2.048)
    pipe = oracle_lib.Pipeline(Intrinsics.from_any(intr), p)
    for k in range(N):
        assert pipe.process(bgr[k], dep[k].astype(np.float32)) == 0
    assert pipe.frame_count == N + 1
    P = pipe.poses()
    assert P.shape == (N, 4, 4)
    assert np.array_equal(P[0], np.eye(4, dtype=np.float32))
    # the reference's raycast bias A3 (up to 2 voxels = 32 mm here) limits
    # accuracy; with the bias removed the same loop tracks to < 1 mm
    assert np.abs(P[:, :3, 3] - gt[:, :3, 3]).max() < 3 * 0.016


def test_pipeline_a2_small_image_cannot_track(oracle_lib):
    # A2 (R): 160x120 with 3 levels leaves level 2 (40x30) with floor(30/32)=0
    # ICP rows -> A = 0 -> det check fails on the second frame
    intr = synth.Intrinsics.qqvga()
    bgr, dep, gt = synth.sequence(2, intr)
    pipe = oracle_lib.Pipeline(Intrinsics.from_any(intr), default_params(dims=64, range_m=2.048))
    assert pipe.process(bgr[0], dep[0].astype(np.float32)) == 0
    assert pipe.process(bgr[1], dep[1].astype(np.float32)) == 1


def test_pipeline_tracking_failure_resets(oracle_lib):
    intr = synth.Intrinsics.qvga()
    bgr, dep, gt = synth.sequence(3, intr)
    p = default_params(dims=64, range_m=2.048)
    pipe = oracle_lib.Pipeline(Intrinsics.from_any(intr), p)
    assert pipe.process(bgr[0], dep[0].astype(np.float32)) == 0
    assert pipe.process(bgr[1], dep[1].astype(np.float32)) == 0
    blank = np.zeros_like(dep[2], dtype=np.float32)
    assert pipe.process(bgr[2], blank) == 1  # no correspondences -> det 0 -> reset
    assert pipe.frame_count == 1 and pipe.poses().shape[0] == 1
    t, w, c = pipe.volume()
    assert not t.any() and not w.any() and not c.any()


def test_pose_text_format_matches_reference_artifact(oracle_lib, tmp_path):
    """doc/poses.txt (written by main.cpp:95-98) round-trips through the %.8g
    Matx44f writer byte for byte."""
    import os
    ref = open(os.path.join(os.path.dirname(__file__), "golden", "ref_doc_poses.txt")).read()
    blocks = ref.strip().split("]\n")
    assert len(blocks) == 50
    out = []
    for b in blocks:
        nums = [float(s) for s in b.replace("[", "").replace("]", "").replace(";", ",").split(",")]
        m = np.array(nums, dtype=np.float32).reshape(4, 4)
        out.append(oracle_lib.format_pose(Pose.from_matrix(m)))
    assert "".join(out) == ref


def test_extract_points_plane(oracle_lib):
    """FullScan6 (tsdf_volume.cu:307-481) on the integrated plane z = D: the +z
    zero crossings of every observed column lie on the plane (world z = D,
    since the volume pose is translate(-L/2, -L/2, 0.5) and the camera is at
    the origin), within the tsdf quantisation."""
    intr = Intrinsics(160, 120, 131.25, 131.25, 79.5, 59.5)
    L, dims = 2.0, 64
    p = plane_params(dims, L)
    vol = oracle_lib.Volume((dims,) * 3, (L,) * 3)
    D = 1.5
    dmap = np.full((120, 160), D, np.float32)
    bgr = np.zeros((120, 160, 3), np.uint8)
    for _ in range(3):
        oracle_lib.integrate(vol, p.volu_trun_dist, intr, p.volu_pose, dmap, bgr)
    pts, n = oracle_lib.extract_points(vol, p.volu_pose)
    assert n == len(pts) > 500
    # integrate samples voxel z at z*vs, FullScan6 places it at (z + 0.5)*vs
    # (SURVEY.md §8f): the crossings sit half a voxel beyond the plane
    assert np.median(np.abs(pts[:, 2] - (D + 0.5 * L / dims))) < 0.25 * L / dims
    # a capped call returns the prefix of the canonical order
    pts2, n2 = oracle_lib.extract_points(vol, p.volu_pose, cap=100)
    assert n2 == n and np.array_equal(pts2, pts[:100])
    # slabs [0, 32) + [32, 63) concatenate to the full extraction
    a, _ = oracle_lib.extract_points(vol, p.volu_pose, 0, 32)
    b, _ = oracle_lib.extract_points(vol, p.volu_pose, 32, dims - 1)
    assert np.array_equal(np.concatenate([a, b]), pts)


def test_extract_points_needs_weight_and_sign_change(oracle_lib):
    dims, L = 16, 1.0
    vol = oracle_lib.Volume((dims,) * 3, (L,) * 3)
    t = vol.tsdf.reshape(dims, dims, dims)
    w = vol.weight.reshape(dims, dims, dims)
    t[5, 5, 5], t[5, 5, 6] = 16383, -16383   # +x crossing at the midpoint
    w[5, 5, 5] = w[5, 5, 6] = 1
    pose = Pose.identity()
    pts, n = oracle_lib.extract_points(vol, pose)
    assert n == 1
    vs = L / dims
    np.testing.assert_allclose(pts[0], [6 * vs, 5.5 * vs, 5.5 * vs], rtol=0, atol=1e-6)
    w[5, 5, 6] = 0  # unobserved neighbour: no point
    assert oracle_lib.extract_points(vol, pose)[1] == 0


def test_ply_text_format(oracle_lib):
    txt = oracle_lib.ply_text(np.array([[0.1, -2.5, 1234567.0], [1e-7, 0.0, 3.0]], np.float32))
    assert txt == ("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\n"
                   "property float z\nend_header\n0.1 -2.5 1.23457e+06\n1e-07 0 3\n")


def _render_ref(v, n, eye):
    """numpy float32 restatement of renderPhong for one pixel (image_process.cu:159-211)."""
    f = np.float32
    v, n, eye = (np.asarray(a, f) for a in (v, n, eye))

    def norm(a):
        t = np.sqrt(f(f(a[0] * a[0]) + f(a[1] * a[1])) + f(a[2] * a[2]), dtype=f)
        return np.array([a[0] / t, a[1] / t, a[2] / t], f)

    def dot(a, b):
        return f(f(f(a[0] * b[0]) + f(a[1] * b[1])) + f(a[2] * b[2]))
    e = norm(eye - v)
    li = norm(np.array([500, 500, -500], f) - v)
    lc = abs(dot(n, li))
    coef = f(f(0.9) * lc)
    diff = np.array([0.3843, 0.4745, 0.580], f) * coef
    h = norm(li + e)
    hc = abs(dot(n, h))
    h2 = f(hc * hc)
    h4 = f(h2 * h2)
    h8 = f(h4 * h4)
    spec = 0.5 * float(f(f(0.9) * f(h8 * h2)))
    k = [f(min(1.0, float(f(f(0.1) + d)) + spec)) for d in diff]
    return [int(x * f(255)) if x >= 1 / 255 else 0 for x in k]


def test_render_kat(oracle_lib):
    """renderPhong / renderNormals (image_process.cu:137-221): hand-restated
    pixels, the early returns (zero normal or vertex stay 0) and NaN normals."""
    rng = np.random.default_rng(3)
    h, w = 4, 5
    v = rng.uniform(-1, 1, (h, w, 3)).astype(np.float32)
    v[..., 2] += 2
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    n[0, 0] = 0          # zero normal: early return
    v[0, 1] = 0          # zero vertex: early return
    n[1, 1] = np.nan     # NaN normal (frame-1 measured maps)
    eye = np.array([0.1, -0.2, 0.3], np.float32)
    ph = oracle_lib.render(v, n, eye, "phong")
    nm = oracle_lib.render(v, n, eye, "normal")
    assert (ph[0, 0] == 0).all() and (ph[0, 1] == 0).all() and (nm[1, 1] == 0).all()
    for y in range(h):
        for x in range(w):
            if (y, x) in ((0, 0), (0, 1), (1, 1)):
                continue
            assert list(ph[y, x]) == _render_ref(v[y, x], n[y, x], eye), (y, x)
            assert list(nm[y, x]) == [int(np.float32(abs(c)) * np.float32(255)) for c in n[y, x]]


def test_rodrigues_sincos_within_an_ulp_of_libm(oracle_lib):
    """D: the Rodrigues cos/sin are Taylor polynomials for
    theta < 0.5 (kfo_sincos, the kernel's det_sincos): within 1 ulp of libm in
    double, and the float factors the pose update uses (float(c), float(1-c),
    float(s) times unit-range values) round to libm's except at rounding ties."""
    rng = np.random.default_rng(3)
    th = np.concatenate([rng.uniform(0, 0.5, 20000), 10.0 ** rng.uniform(-12, -0.31, 20000), [1e-15, 0.4999999]])
    worst, fdiff = 0.0, 0
    for t in th:
        s, c = oracle_lib.sincos(float(t))
        worst = max(worst, abs(s - math.sin(t)) / math.ulp(math.sin(t)), abs(c - math.cos(t)) / math.ulp(math.cos(t)))
        fdiff += np.float32(s) != np.float32(math.sin(t))
        fdiff += np.float32(1.0 - c) != np.float32(1.0 - math.cos(t))
    assert worst <= 1.0
    assert fdiff <= 2
    assert oracle_lib.sincos(0.7) == (math.sin(0.7), math.cos(0.7))  # libm above the polynomial range


def test_saturated_free_space_fixed_point():
    """k_integrate skips the update of saturated free space (w0 = MAX_WEIGHT =
    64, t0 = T*, sdf >= trunc so ts = 1 exactly): the reference's running
    average (tsdf_volume.cu:72-81, restated by the oracle) leaves such a voxel
    unchanged, and T* = 32766 is where free space settles (32767 after the
    first update, 32766 from the second on)."""
    import oracle as O
    for trunc in (0.0084, 2.1 * 2.048 / 1024, 2.1 * 4.096 / 2048, 2.1 * 3.0 / 512):
        for sdf in (trunc, float(np.nextafter(np.float32(trunc), np.float32(1))), 2 * trunc, 0.5, 7.0):
            assert O.tsdf_update(32766, 64, sdf, float(np.float32(trunc))) == (32766, 64)
            t = 0
            for w in range(64):  # a voxel seen as free space from its first update on
                t, w1 = O.tsdf_update(t, w, sdf, float(np.float32(trunc)))
                assert (t, w1) == ((32767 if w == 0 else 32766), w + 1)
