"""Integrate's hidden-brick skip against the oracle.

k_integrate steps over a brick when kfx::brick_hidden proves that the brick
lies behind every surface it projects onto.  Every comparison is bitwise
against the oracle: tsdf, weight and rgb of the whole volume, and for the
pipeline cases the poses and the PREV maps of every level.  debug_get_hidden
gives (bricks skipped as hidden, those among them that hang over an end of
their tile's interval) of the last integrate launch.  (Cutting the trailing
hidden bricks from the interval before the chunks are cut was built and
measured slower; the bricks at the interval's end are stepped
over instead, and the second count pins that they are.)

a  spheres in front of a wall (the default scene), 128^3 on QVGA, 6 frames of a
   moving camera: the shadows sweep, so bricks hidden in one frame are updated
   in the next; every frame hides bricks;
b  a wall 10 slices inside the far face, 128^3 on QQVGA, through the stage
   seam from the base pose and from two oblique ones.  (Seen straight on, the
   tile clip already ends each interval less than a brick behind the wall and
   no brick is hidden; a tile seen obliquely sweeps cells whose depth is the
   far side of the wall, and the trailing bricks of its interval are hidden.)
c  20 % dropouts and a quadrant without depth, then a blank frame (the reset
   path), then a frame again;
d  a volume uploaded settled, static frames: settled and hidden bricks are
   skipped by the same launches;
e  16 x 16 x 1030 and 16 x 24 x 1500 voxels: length-capped chunks of 257 to 375
   slices (up to 47 bricks per wave; no chunk here exceeds the 64-brick mask);
f  two Z-slab contexts against the single volume's oracle, and case a's first
   frames through the 64-bit-index kernels;
g  4 frames of case a staged and overlapped in graph modes 0, 1 and 2;
h  tiles whose whole interval is hidden: the volume's front face 4.095 m from
   the camera, the left half of the image a wall at 4.0 m, the right half one
   at 4.25 m.  A left tile's clip ends its interval at slice 4 (the far clips'
   2 % is 8 cm there), and its one brick lies behind the certificate's bound
   (0.64 % at this camera): the waves of those tiles only step over a brick
   that hangs over both ends of the chunk and run no batch.  The columns left
   of the seam keep every uploaded voxel, the right ones are updated.
"""
import numpy as np
import pytest

import integrate_cases as IC
import oracle as O
from kfx import KFX_FRAME_PREV, KFX_OK, KinectFusion, synth
from kfx.abi import Intrinsics, Pose, default_params

pytestmark = pytest.mark.gpu

L_VOL = 2.048


def feq(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    z = np.float32(0)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, z, a).view(np.uint32),
                                                     np.where(nb, z, b).view(np.uint32))


def assert_volume(kf, t, w, c, what, lo=0, hi=None):
    gt, gw, gc = kf.volume_soa()
    s, s4 = slice(lo, hi), slice(4 * lo, None if hi is None else 4 * hi)
    assert np.array_equal(gt[s], t[s]), f"{what}: tsdf, {(gt[s] != t[s]).sum()} voxels differ"
    assert np.array_equal(gw[s], w[s]), f"{what}: weight, {(gw[s] != w[s]).sum()} voxels differ"
    assert np.array_equal(gc[s4], c[s4]), f"{what}: rgb, {(gc[s4] != c[s4]).sum()} bytes differ"


def assert_same(kf, pipe, what):
    gp, op = kf.pose_record, pipe.poses()
    assert gp.shape == op.shape and np.abs(gp - op).max() == 0, f"{what}: poses"
    for l in range(3):
        _, gv, gn = kf.frame_maps(KFX_FRAME_PREV, l)
        assert feq(gv, pipe.map(1, 1, l)) and feq(gn, pipe.map(1, 2, l)), f"{what}: PREV maps level {l}"
    assert_volume(kf, *pipe.volume(), what)


def upload_both(kf, pipe, vol):
    t, w, c = vol
    kf.upload_tsdf(IC.records(t, w, c))
    n = t.size
    np.ctypeslib.as_array(O.lib().kfo_pipe_tsdf(pipe.h), shape=(n,))[:] = t
    np.ctypeslib.as_array(O.lib().kfo_pipe_weight(pipe.h), shape=(n,))[:] = w
    np.ctypeslib.as_array(O.lib().kfo_pipe_rgb(pipe.h), shape=(4 * n,))[:] = c


@pytest.fixture(scope="module")
def qvga():
    return synth.Intrinsics.qvga()


@pytest.fixture(scope="module")
def moving(qvga):
    """6 frames of the default scene from a moving camera (the spheres' shadows sweep over the wall)."""
    bgr, dep, _ = synth.sequence(6, qvga, noise=True, dropout=0.005, traj_seed=7, amp_t=0.16, period=60.0)
    return bgr, dep.astype(np.float32)


def run_moving(qvga, moving, n, N=128, force64=False):
    bgr, dep = moving
    I, p = Intrinsics.from_any(qvga), default_params(dims=N, range_m=L_VOL)
    pipe = O.Pipeline(I, p)
    with KinectFusion(I, p) as kf:
        if force64:
            kf.debug_force_index64(True)
        kf.debug_count_settled(True)
        for k in range(n):
            assert kf.pipeline(bgr[k], dep[k]) == pipe.process(bgr[k], dep[k]) == KFX_OK
            hid, end = kf.debug_get_hidden()
            print(f"frame {k}: {hid} bricks skipped as hidden ({end} at an interval's end), "
                  f"{kf.debug_get_settled()[1]} as settled")
            assert hid > 0 and 0 < end <= hid, (k, hid, end)
            assert kf.debug_get_settled()[1] == 0  # nothing is settled in the first frames
            assert_same(kf, pipe, f"frame {k}")


def test_a_sphere_shadows_sweep(qvga, moving):
    run_moving(qvga, moving, 6)


def test_b_wall_inside_the_far_face():
    N, I = 128, IC.QQVGA
    vs = L_VOL / N
    case = type("Case", (), {})()
    case.dims, case.range, case.intr = (N, N, N), (L_VOL, L_VOL, L_VOL), I
    case.params = IC._params(case.dims, case.range, None)
    rng = np.random.default_rng(11)
    depth = ((0.5 + (N - 10) * vs) * 1000.0 + rng.uniform(-2.0, 2.0, (I.height, I.width))).astype(np.float32)
    y, x = np.mgrid[0:I.height, 0:I.width]
    bgr = np.stack([40 + x, 30 + 2 * y, 200 - x - y // 2], -1).astype(np.uint8)
    d0 = O.preprocess(depth, I, case.params)[0][0]
    C0, O0 = IC.T(0, 0, 0.5 + L_VOL / 2), IC.T(-L_VOL / 2, -L_VOL / 2, -L_VOL / 2)
    poses = [IC.BASE, C0 @ IC.rot_y(0.45) @ O0, C0 @ IC.rot_y(-0.3) @ IC.rot_x(0.35) @ O0]
    vol = IC.new_volume(case)
    at_end = []
    with KinectFusion(I, case.params) as kf:
        kf.debug_count_settled(True)
        kf.stage_preprocess(bgr, depth)
        for k, m in enumerate(poses):
            pose = Pose.from_matrix(m)
            counts = O.integrate(vol, case.params.volu_trun_dist, I, pose, d0, bgr)
            assert counts[0] >= 10000  # oracle only
            got = kf.stage_integrate(pose)
            hid, end = kf.debug_get_hidden()
            print(f"pose {k}: {hid} bricks skipped as hidden ({end} at an interval's end), {counts[0]} voxels updated")
            assert end <= hid
            at_end.append(end)
            assert got == counts, (k, got, counts)
            assert_volume(kf, vol.tsdf, vol.weight, vol.rgb, f"pose {k}")
    assert sum(at_end) > 0, at_end


def test_c_dropouts_depthless_quadrant_and_reset(qvga):
    N = 64
    scene = synth.Scene.default(L_VOL)
    fr = []
    for k in range(4):
        b, d = synth.render(scene, qvga, np.eye(4), noise_seed=300 + k, dropout=0.2)
        d = d.astype(np.float32)
        d[: qvga.height // 2, qvga.width // 2:] = 0.0
        fr.append((b, d))
    fr[2] = (fr[2][0], np.zeros_like(fr[2][1]))  # blank: the reset path
    I, p = Intrinsics.from_any(qvga), default_params(dims=N, range_m=L_VOL)
    pipe = O.Pipeline(I, p)
    hidden = 0
    with KinectFusion(I, p) as kf:
        kf.debug_count_settled(True)
        for k, (b, d) in enumerate(fr):
            assert kf.pipeline(b, d) == pipe.process(b, d), f"frame {k}: status"
            hid, end = kf.debug_get_hidden()
            print(f"frame {k}: {hid} bricks skipped as hidden ({end} at an interval's end)")
            hidden += hid
            assert_same(kf, pipe, f"frame {k}")
    assert hidden > 0


def settled_volume(intr, depth_mm, N):
    """test_gpu_settled.settled_volume at N^3: free space at weight 64 and T*, the rest zero."""
    vs = L_VOL / N
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    px, py, pz = x * vs - L_VOL / 2, y * vs - L_VOL / 2, z * vs + 0.5
    u = np.rint(px / pz * intr.fx + intr.cx).astype(np.int64)
    v = np.rint(py / pz * intr.fy + intr.cy).astype(np.int64)
    inside = (u >= 0) & (u < intr.width) & (v >= 0) & (v < intr.height)
    d = np.where(inside, depth_mm[np.clip(v, 0, intr.height - 1), np.clip(u, 0, intr.width - 1)] * 0.001, 0.0)
    free = (inside & (d > 0) & (d - np.sqrt(px * px + py * py + pz * pz) >= 0.25)).ravel()
    return (np.where(free, IC.tsat(), 0).astype(np.int16), np.where(free, 64, 0).astype(np.int16),
            np.zeros(4 * N ** 3, np.uint8))


def test_d_settled_and_hidden_in_the_same_waves(qvga):
    N = 128
    scene = synth.Scene.default(L_VOL)
    fr = [synth.render(scene, qvga, np.eye(4), noise_seed=100 + k, dropout=0.002) for k in range(3)]
    fr = [(b, d.astype(np.float32)) for b, d in fr]
    I, p = Intrinsics.from_any(qvga), default_params(dims=N, range_m=L_VOL)
    pipe = O.Pipeline(I, p)
    with KinectFusion(I, p) as kf:
        kf.debug_count_settled(True)
        upload_both(kf, pipe, settled_volume(qvga, fr[0][1], N))
        for k, (b, d) in enumerate(fr):
            assert kf.pipeline(b, d) == pipe.process(b, d) == KFX_OK
            (nset, nskip), (hid, end) = kf.debug_get_settled(), kf.debug_get_hidden()
            print(f"frame {k}: {nset} bricks set, {nskip} skipped as settled, {hid} as hidden ({end} at an interval's end)")
            assert (nskip > 0) == (k >= 1) and hid > 0, (k, nskip, hid)
            assert_same(kf, pipe, f"frame {k}")


@pytest.mark.parametrize("name", ["deep1030", "deep1500"])
def test_e_deep_intervals_take_the_per_chunk_masks(name):
    case = IC.CASES[name]
    bgr, depth = IC.frame(case.frame)
    steps, _ = IC.oracle_zeroed(name)
    with KinectFusion(case.intr, case.params) as kf:
        kf.debug_count_settled(True)
        kf.stage_preprocess(bgr, depth)
        for k, (pose, (counts, t, w, c)) in enumerate(zip(case.poses, steps)):
            got = kf.stage_integrate(pose)
            hid, end = kf.debug_get_hidden()
            print(f"{name} launch {k}: {hid} bricks skipped as hidden ({end} at an interval's end)")
            assert hid > 0 and got == counts, (k, got, counts)
            assert_volume(kf, t, w, c, f"{name} launch {k}")


def test_f_two_slabs_against_the_single_volume():
    name, world = "slab300", 2
    case = IC.CASES[name]
    X, Y, Z = case.dims
    bgr, depth = IC.frame(case.frame)
    steps, _ = IC.oracle_zeroed(name)
    hidden = 0
    for r in range(world):
        with KinectFusion(case.intr, case.params, slab=(r, world)) as kf:
            _, _, o0, o1 = kf.slab_info()
            kf.debug_count_settled(True)
            kf.stage_preprocess(bgr, depth)
            for k, (pose, (_, t, w, c)) in enumerate(zip(case.poses, steps)):
                kf.stage_integrate(pose, counts=False)
                hid, end = kf.debug_get_hidden()
                hidden += hid
                print(f"rank {r} launch {k}: {hid} bricks skipped as hidden ({end} at an interval's end)")
                assert_volume(kf, t, w, c, f"rank {r} launch {k}", o0 * X * Y, o1 * X * Y)
    assert hidden > 0  # slab contexts keep no settled bytes and skip hidden bricks all the same


def test_f_index64(qvga, moving):
    run_moving(qvga, moving, 2, force64=True)


@pytest.fixture(scope="module")
def four_frames(qvga, moving):
    bgr, dep = moving
    I, p = Intrinsics.from_any(qvga), default_params(dims=128, range_m=L_VOL)
    pipe = O.Pipeline(I, p)
    assert [pipe.process(bgr[k], dep[k]) for k in range(4)] == [KFX_OK] * 4
    return pipe


@pytest.mark.parametrize("gmode", [0, 1, 2])
def test_g_staged_overlapped_frames(qvga, moving, four_frames, gmode):
    bgr, dep = moving
    with KinectFusion(Intrinsics.from_any(qvga), default_params(dims=128, range_m=L_VOL)) as kf:
        kf.debug_count_settled(True)
        kf.set_graph_mode(gmode)
        kf.set_frame_overlap(True)
        kf.stage_frames(bgr[:4], dep[:4])
        for k in range(4):
            kf.pipeline_staged(k)
        assert kf.synchronize() == KFX_OK
        assert kf.debug_get_hidden()[0] > 0
        assert_same(kf, four_frames, f"staged frames, graph mode {gmode}")


def test_h_tiles_whose_whole_interval_is_hidden():
    N, I = 128, IC.QQVGA
    vs = L_VOL / N
    case = type("Case", (), {})()
    case.dims, case.range, case.intr = (N, N, N), (L_VOL, L_VOL, L_VOL), I
    case.params = IC._params(case.dims, case.range, None)
    rng = np.random.default_rng(12)
    depth = np.where(np.arange(I.width)[None, :] < 80, 4000.0, 4250.0) + rng.uniform(-0.5, 0.5, (I.height, I.width))
    depth = depth.astype(np.float32)
    y, x = np.mgrid[0:I.height, 0:I.width]
    bgr = np.stack([40 + x, 30 + 2 * y, 200 - x - y // 2], -1).astype(np.uint8)
    d0 = O.preprocess(depth, I, case.params)[0][0]
    init = IC.random_volume(case.dims)
    vol = IC.new_volume(case, init)
    pose = Pose.from_matrix(IC.T(-L_VOL / 2, -L_VOL / 2, 4.095))
    counts = O.integrate(vol, case.params.volu_trun_dist, I, pose, d0, bgr)
    # oracle only: columns more than 0.25 m left of the optical axis (8 pixels from the seam) keep every voxel
    left = (np.arange(N) * vs - L_VOL / 2 < -0.25)
    w0 = init[1].reshape(N, N, N)
    t0 = init[0].reshape(N, N, N)
    assert left.sum() >= 40
    assert np.array_equal(vol.weight.reshape(N, N, N)[:, :, left], w0[:, :, left])
    assert np.array_equal(vol.tsdf.reshape(N, N, N)[:, :, left], t0[:, :, left])
    assert counts[0] >= 10000 and (vol.weight.reshape(N, N, N)[:, :, ~left] != w0[:, :, ~left]).sum() >= 10000
    with KinectFusion(I, case.params) as kf:
        kf.debug_count_settled(True)
        kf.upload_tsdf(IC.records(*init))
        kf.stage_preprocess(bgr, depth)
        got = kf.stage_integrate(pose)
        hid, end = kf.debug_get_hidden()
        print(f"{hid} bricks skipped as hidden ({end} at an interval's end), {counts[0]} voxels updated")
        assert got == counts, (got, counts)
        # the volume (2.048 m wide, 4.1 m away) lies wholly inside the image, so each of the 16 tile rows holds
        # the left.sum() // 8 = 6 tile columns that lie wholly left of -0.25 m: at least 96 tiles hide their one
        # brick (256 skipped bricks measured)
        assert left.sum() // 8 == 6 and hid >= 16 * 6 and end == hid, (hid, end)
        assert_volume(kf, vol.tsdf, vol.weight, vol.rgb, "whole-interval tiles")
