"""GPU-vs-oracle parity across the parameter space kfx_create accepts.

test_gpu_parity.py pins the library at the default parameters (pyramid_height
3, a 5x5 bilateral window, sigmas 10/10, dfilter_dist 5) on four image sizes
with a centred principal point and integer-millimetre depth.  This module
moves along each axis create_impl lets through: pyramid heights 1, 2 and 4,
tiny images under windows up to 15x15, widths that are no multiple of 16,
off-centre and anisotropic intrinsics, a depth cut inside the scene, float
depth holding NaN / inf / negative / out-of-range values and large holes,
zero ICP iteration counts and a pyramid level whose ICP region is empty.

The bar is the one of test_gpu_parity.py: float maps bit for bit with NaNs
matched by position, volume records / counts / ICP sums exactly equal, pose
differences == 0.  No tolerance is chosen anywhere.  Every "this case is not
vacuous" assertion is evaluated on the oracle's results only, so a GPU bug
cannot satisfy it.
"""
import functools

import numpy as np
import pytest

import oracle as O
from kfx import KFX_FRAME_CUR, KFX_FRAME_PREV, KFX_OK, KFX_TRACKING_LOST, KinectFusion, synth
from kfx.abi import Intrinsics, Pose, default_params

pytestmark = pytest.mark.gpu

L_VOL = 2.048
N_FRAMES = 4


def feq(a, b):
    """Bit equality of float32 arrays with NaNs compared by position (test_gpu_parity.feq)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    z = np.float32(0)
    return np.array_equal(np.where(na, z, a).view(np.uint32), np.where(nb, z, b).view(np.uint32))


def mismatch(a, b):
    a = np.asarray(a, np.float32).ravel()
    b = np.asarray(b, np.float32).ravel()
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    return int(bad.sum())


def params(**kw):
    """default_params on the 64^3 / 2.048 m volume; icp_iter_count takes a list."""
    p = default_params(dims=64, range_m=L_VOL)
    for k, v in kw.items():
        if k == "icp_iter_count":
            for i, n in enumerate(v):
                p.icp_iter_count[i] = n
        else:
            setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def sequence(w, h, fx, fy, cx, cy):
    """(bgr, depth u16, depth f32) of the 4-frame synthetic sequence, rendered once per geometry."""
    bgr, dep, _ = synth.sequence(N_FRAMES, synth.Intrinsics(w, h, fx, fy, cx, cy), noise=True, dropout=0.01)
    depf = dep.astype(np.float32)
    for a in (bgr, dep, depf):
        a.setflags(write=False)
    return bgr, dep, depf


QVGA = (320, 240, 262.5, 262.5, 159.5, 119.5)
QQVGA = (160, 120, 131.25, 131.25, 79.5, 59.5)
ODD = (328, 248, 262.5, 262.5, 163.5, 123.5)       # widths 328 / 164 / 82: none a multiple of 16
ODD_OFF = (328, 248, 250.0, 281.0, 150.25, 131.75)  # fx != fy, principal point off the centre


def assert_maps_equal(got, want, what):
    for name, g, o in zip(("dmap", "vmap", "nmap"), got, want):
        assert feq(g, o), f"{what} {name}: {mismatch(g, o)} of {o.size} values differ"


def assert_preprocess_equal(kf, levels, ds, vs, ns, what=""):
    for l in range(levels):
        assert_maps_equal(kf.frame_maps(KFX_FRAME_CUR, l), (ds[l], vs[l], ns[l]), f"{what} level {l}")


def assert_volume_equal(kf, tsdf, weight, rgb):
    t, w, c = kf.volume_soa()
    assert np.array_equal(t, tsdf), f"tsdf: {(t != tsdf).sum()} voxels differ"
    assert np.array_equal(w, weight), f"weight: {(w != weight).sum()} voxels differ"
    assert np.array_equal(c, rgb), f"rgb: {(c != rgb).sum()} bytes differ"


def good_normals(n):
    """Pixels whose normal is finite and not the zero vector."""
    return int((np.isfinite(n).all(-1) & (n != 0).any(-1)).sum())


def run_both(I, p, bgr, frames):
    """The frames through the library's pipeline and the oracle's; (kf, pipe, statuses, oracle statuses)."""
    kf = KinectFusion(I, p)
    pipe = O.Pipeline(I, p)
    st, ost = [], []
    for k in range(len(frames)):
        st.append(kf.pipeline(bgr[k], frames[k]))
        ost.append(pipe.process(bgr[k], frames[k]))
    return kf, pipe, st, ost


def assert_pipeline_equal(kf, pipe, st, ost, levels, maps=True, volume=True):
    assert st == ost, (st, ost)
    assert kf.frame_count == pipe.frame_count
    gp, op = kf.pose_record, pipe.poses()
    assert gp.shape == op.shape, (gp.shape, op.shape)
    err = float(np.abs(gp - op).max())
    assert err == 0, err
    if maps:
        for l in range(levels):
            _, gv, gn = kf.frame_maps(KFX_FRAME_PREV, l)
            ov, on = pipe.map(1, 1, l), pipe.map(1, 2, l)
            assert feq(gv, ov), f"PREV vmap level {l}: {mismatch(gv, ov)} differ"
            assert feq(gn, on), f"PREV nmap level {l}: {mismatch(gn, on)} differ"
    if volume:
        assert_volume_equal(kf, *pipe.volume())


def assert_oracle_tracked(pipe, ost):
    """Oracle side only: every frame tracked and the camera moved."""
    assert ost == [KFX_OK] * N_FRAMES, ost
    op = pipe.poses()
    assert op.shape == (N_FRAMES, 4, 4)
    assert np.abs(op[-1] - np.eye(4)).max() > 1e-3  # the trajectory moves ~1e-2 over three frames


# ---------------------------------------------------------------------------
# a. preprocess on tiny images with large windows

def tiny_depth(w, h):
    """Float mm: a smooth surface near 1.2 m, sinusoids of a few hundred mm,
    Gaussian noise (sigma 8 mm) and 3 % zero pixels."""
    rng = np.random.default_rng(1000 * w + h)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 1200.0 + 2.0 * x - 1.5 * y + 150.0 * np.sin(0.45 * x + 0.3) + 120.0 * np.cos(0.6 * y)
    d += rng.normal(0.0, 8.0, (h, w))
    d[rng.random((h, w)) < 0.03] = 0.0
    return d.astype(np.float32)


@pytest.mark.parametrize("w,h,height,ksz", [
    (24, 16, 1, 15),  # the image is smaller than one 16x16 tile plus its halo
    (16, 16, 2, 15),  # level 1 is 8x8 under r = 7
    (32, 32, 3, 7),
    (64, 48, 4, 11),  # level 3 is 8x6 under r = 5: the smallest level create lets through
    (40, 24, 3, 5),   # widths 40 / 20 / 10: partial tiles in x at every level
])
def test_preprocess_tiny_images_large_windows(w, h, height, ksz):
    I = Intrinsics(w, h, 0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0)
    p = params(pyramid_height=height, bfilter_kernel_size=ksz, bfilter_spatial_sigma=3.0,
               bfilter_color_sigma=40.0)
    d = tiny_depth(w, h)
    bgr = np.zeros((h, w, 3), np.uint8)
    ds, vs, ns = O.preprocess(d, I, p)
    assert len(ds) == height
    for l in range(height):  # oracle only: the level holds depth and interior normals
        assert (ds[l] > 0).any(), l
        assert good_normals(ns[l]) > 0, l
    with KinectFusion(I, p) as kf:
        kf.stage_preprocess(bgr, d)
        assert_preprocess_equal(kf, height, ds, vs, ns)


# ---------------------------------------------------------------------------
# b. preprocess parameters at QVGA

PREPROCESS = {
    "ksz1": dict(bfilter_kernel_size=1),
    "ksz6": dict(bfilter_kernel_size=6),
    "ksz15": dict(bfilter_kernel_size=15),
    "ksz15_sigmas": dict(bfilter_kernel_size=15, bfilter_spatial_sigma=4.5, bfilter_color_sigma=30.0),
    "dfilter_2.3": dict(dfilter_dist=2.3),
}


@pytest.mark.parametrize("name", list(PREPROCESS))
def test_preprocess_parameters_qvga(name):
    kw = PREPROCESS[name]
    bgr, _, depf = sequence(*QVGA)
    I = Intrinsics(*QVGA)
    p, p_def = params(**kw), params()
    with KinectFusion(I, p) as kf:
        for k in (0, 3):
            ds, vs, ns = O.preprocess(depf[k], I, p)
            ds_def, _, _ = O.preprocess(depf[k], I, p_def)
            assert mismatch(ds[0], ds_def[0]) > 0  # oracle only: the parameter changes the result
            if name == "dfilter_2.3":  # oracle only: the cut removes part of every level and keeps part
                for l in range(3):
                    assert 0 < (ds[l] > 0).sum() < (ds_def[l] > 0).sum(), l
            kf.stage_preprocess(bgr[k], depf[k])
            assert_preprocess_equal(kf, 3, ds, vs, ns, f"frame {k}")
        if name == "dfilter_2.3":  # integrate over a depth map with cut regions (frame 3's)
            vol = O.Volume((64,) * 3, (L_VOL,) * 3)
            ou, oc = O.integrate(vol, p.volu_trun_dist, I, p.volu_pose, ds[0], bgr[3])
            assert ou > 0 and oc > 0
            assert kf.stage_integrate(p.volu_pose) == (ou, oc)
            assert_volume_equal(kf, vol.tsdf, vol.weight, vol.rgb)


# ---------------------------------------------------------------------------
# c. hostile float depth

def hostile(depth_f32, k):
    """Frame k's depth with sub-millimetre fractions, holes larger than any
    window, NaN, +inf, negative and out-of-range values, and zeros / NaNs on
    the image border."""
    d = depth_f32.copy()
    rng = np.random.default_rng(100 + k)
    d += np.where(d != 0, rng.uniform(-0.5, 0.5, d.shape), 0.0).astype(np.float32)
    d[20:52, 30:70] = 0.0        # 4-aligned
    d[101:131, 203:229] = 0.0    # not aligned
    d[60:64, 100:140] = np.nan
    d[150, 10:300:7] = np.nan
    d[180:184, 40:60] = np.inf
    d[200:203, 250:260] = -800.0
    d[210:214, 100:120] = 65535.0
    d[220:224, 100:120] = 5000.4
    d[0, :17] = 0.0
    d[0, 4:11] = np.nan
    d[-1, -9:] = np.nan
    d[-1, -3] = 0.0
    d[:5, -1] = np.nan
    d[1, -1] = 0.0
    return d


@pytest.fixture(scope="module")
def hostile_frames():
    _, _, depf = sequence(*QVGA)
    frames = np.stack([hostile(depf[k], k) for k in range(N_FRAMES)])
    frames.setflags(write=False)
    return frames


def test_hostile_depth_preprocess(hostile_frames):
    bgr, _, _ = sequence(*QVGA)
    I = Intrinsics(*QVGA)
    p = params()
    k = 1
    ds, vs, ns = O.preprocess(hostile_frames[k], I, p)
    for l in range(3):  # oracle only
        assert np.isnan(ds[l]).any(), l
        assert not np.isinf(ds[l]).any(), l
    assert (ds[0] < 0).any() and (ds[1] < 0).any()
    with KinectFusion(I, p) as kf:
        kf.stage_preprocess(bgr[k], hostile_frames[k])
        assert_preprocess_equal(kf, 3, ds, vs, ns)


def test_hostile_depth_integrate(hostile_frames):
    bgr, _, depf = sequence(*QVGA)
    I = Intrinsics(*QVGA)
    p = params()
    k = 1
    ds, _, _ = O.preprocess(hostile_frames[k], I, p)
    vol = O.Volume((64,) * 3, (L_VOL,) * 3)
    ou, oc = O.integrate(vol, p.volu_trun_dist, I, p.volu_pose, ds[0], bgr[k])
    plain = O.Volume((64,) * 3, (L_VOL,) * 3)  # oracle only: the edits change the integrated volume
    O.integrate(plain, p.volu_trun_dist, I, p.volu_pose, O.preprocess(depf[k], I, p)[0][0], bgr[k])
    assert ou > 0 and ((vol.tsdf != plain.tsdf) | (vol.weight != plain.weight)).sum() > 0
    with KinectFusion(I, p) as kf:
        kf.stage_preprocess(bgr[k], hostile_frames[k])
        assert kf.stage_integrate(p.volu_pose) == (ou, oc)
        assert_volume_equal(kf, vol.tsdf, vol.weight, vol.rgb)


def test_hostile_depth_pipeline(hostile_frames):
    bgr, _, _ = sequence(*QVGA)
    I = Intrinsics(*QVGA)
    kf, pipe, st, ost = run_both(I, params(), bgr, hostile_frames)
    assert ost == [KFX_OK] * N_FRAMES and pipe.poses().shape == (N_FRAMES, 4, 4)  # oracle only
    assert_pipeline_equal(kf, pipe, st, ost, 3)
    kf.close()


# ---------------------------------------------------------------------------
# d. pipeline over image geometry and pyramid height

GEOMETRY = {
    "height1": (QVGA, dict(pyramid_height=1, icp_iter_count=[10, 0, 0, 0])),
    "height2": (QVGA, dict(pyramid_height=2, icp_iter_count=[5, 4, 0, 0])),
    # level 3 is 40x32: its ICP region is one 32x32 block
    "height4": ((320, 256, 262.5, 262.5, 159.5, 127.5), dict(pyramid_height=4, icp_iter_count=[3, 3, 3, 2])),
    "328x248": (ODD, {}),
    "328x248_offcentre": (ODD_OFF, {}),
    "200x136": ((200, 136, 164.0, 164.0, 99.5, 67.5), {}),
}


@pytest.mark.parametrize("case", list(GEOMETRY))
def test_pipeline_geometry_and_pyramid_height(case):
    geom, kw = GEOMETRY[case]
    bgr, _, depf = sequence(*geom)
    I = Intrinsics(*geom)
    p = params(**kw)
    levels = p.pyramid_height
    kf, pipe, st, ost = run_both(I, p, bgr, depf)
    assert_oracle_tracked(pipe, ost)
    assert_pipeline_equal(kf, pipe, st, ost, levels)
    kf.close()
    if case == "height4":  # the coarsest of four levels through the stage seam
        prev = O.preprocess(depf[1], I, p)
        cur = O.preprocess(depf[2], I, p)
        with KinectFusion(I, p) as kf:
            kf.stage_preprocess(bgr[2], depf[2])
            for l in range(levels):
                kf.set_frame_maps(KFX_FRAME_PREV, l, prev[1][l], prev[2][l])
            pose = Pose.identity()
            o = O.icp_accumulate(cur[1][3], cur[2][3], prev[1][3], prev[2][3], I.level(3), pose)
            assert o[0] > 0  # oracle only
            g = kf.stage_icp_accumulate(3, pose)
            assert np.array_equal(g, o), g - o


# ---------------------------------------------------------------------------
# e. ICP iteration counts

@pytest.mark.parametrize("iters", [[0, 0, 3, 0], [2, 0, 0, 0], [0, 0, 0, 0]], ids=["0030", "2000", "0000"])
def test_icp_iteration_counts(iters):
    bgr, _, depf = sequence(*QVGA)
    I = Intrinsics(*QVGA)
    kf, pipe, st, ost = run_both(I, params(icp_iter_count=iters), bgr, depf)
    op = pipe.poses()
    assert ost == [KFX_OK] * N_FRAMES and op.shape == (N_FRAMES, 4, 4)  # oracle only
    if any(iters):
        assert np.abs(op[-1] - np.eye(4)).max() > 1e-3  # oracle only: the iterations moved the pose
    else:
        assert np.array_equal(op, np.broadcast_to(np.eye(4, dtype=np.float32), op.shape))
    assert_pipeline_equal(kf, pipe, st, ost, 3, maps=False, volume=False)
    kf.close()


# ---------------------------------------------------------------------------
# f. a pyramid level whose ICP region is empty

def test_empty_icp_level_qqvga():
    """160x120: level 2 is 40x30, so the 32-row floor of its ICP region is
    empty, the level's sums are zero and the solve fails; the reference loses
    every tracked frame there and bootstraps again on the next."""
    bgr, _, depf = sequence(*QQVGA)
    I = Intrinsics(*QQVGA)
    p = params()
    kf, pipe, st, ost = run_both(I, p, bgr, depf)
    assert ost == [KFX_OK, KFX_TRACKING_LOST, KFX_OK, KFX_TRACKING_LOST]  # oracle only
    assert pipe.poses().shape == (1, 4, 4)
    assert_pipeline_equal(kf, pipe, st, ost, 3, maps=False)
    kf.close()
    prev = O.preprocess(depf[1], I, p)
    cur = O.preprocess(depf[2], I, p)
    with KinectFusion(I, p) as kf:
        kf.stage_preprocess(bgr[2], depf[2])
        for l in range(3):
            kf.set_frame_maps(KFX_FRAME_PREV, l, prev[1][l], prev[2][l])
        pose = Pose.identity()
        o = O.icp_accumulate(cur[1][2], cur[2][2], prev[1][2], prev[2][2], I.level(2), pose)
        g = kf.stage_icp_accumulate(2, pose)
        assert not o.any() and not g.any()


# ---------------------------------------------------------------------------
# g. u16 entry

def test_u16_entry_matches_float_entry():
    """kfx_pipeline_u16 on the 328x248 off-centre frames, one of them holding a
    block of 65535, gives the float entry's poses and volume (and the oracle's)."""
    bgr, dep, _ = sequence(*ODD_OFF)
    I = Intrinsics(*ODD_OFF)
    p = params()
    dep = dep.copy()
    dep[2, 100:140, 60:110] = 65535
    depf = dep.astype(np.float32)
    kf, pipe, st, ost = run_both(I, p, bgr, depf)
    assert_oracle_tracked(pipe, ost)
    assert_pipeline_equal(kf, pipe, st, ost, 3)
    with KinectFusion(I, p) as ku:
        assert [ku.pipeline(bgr[k], dep[k]) for k in range(N_FRAMES)] == st
        assert np.array_equal(ku.pose_record, kf.pose_record)
        for a, b in zip(ku.volume_soa(), kf.volume_soa()):
            assert np.array_equal(a, b)
    kf.close()
