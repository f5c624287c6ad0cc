"""Integrate's settled-brick skip against the oracle.

k_integrate steps over a brick whose settled byte is set and which the
frame's free-space certificate covers.  Every case runs a 64^3 volume on QVGA
frames (the smallest image at which the default three-level ICP tracks:
at 160x120 the coarsest level's region is empty and every tracked frame is
lost) and compares poses, all PREV map levels and the whole volume with
oracle.Pipeline, bit for bit:

a  a volume uploaded settled (weight 64 at the ts = 1 fixed point), a static
   scene with dropouts for 3 frames: bricks are skipped from frame 2 on;
b  then a frame whose depth puts a surface into settled free space;
c  10 frames of a moving trajectory (chunk boundaries move across bricks);
d  a tracking loss (volume reset), then an upload of unsettled values over
   bricks whose byte was set: the bytes are gone, the next frame matches;
e  case a through the 64-bit-index kernels;
f  case c through staged overlapped frames in graph modes 1 and 2.
"""
import numpy as np
import pytest

import oracle as O
from kfx import KFX_FRAME_PREV, KFX_OK, KFX_TRACKING_LOST, KinectFusion, synth
from kfx.abi import Intrinsics, default_params

pytestmark = pytest.mark.gpu

L_VOL = 2.048
N = 64


def feq(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    z = np.float32(0)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, z, a).view(np.uint32),
                                                     np.where(nb, z, b).view(np.uint32))


def tsat():
    """The tsdf fixed point of a weight-64, ts = 1 update (test_gpu_regimes.tsat)."""
    t = 32767
    for _ in range(64):
        pre = np.float32(t) * np.float32(0.0000305185)
        new = (pre * np.float32(64) + np.float32(1)) / np.float32(65)
        q = max(-32767, min(32767, int(np.float32(new) * np.float32(32767))))
        if q == t:
            return t
        t = q
    raise AssertionError("no fixed point")


def records(t, w, c):
    rec = np.zeros(t.size, dtype=np.dtype([("tsdf", "<i2"), ("weight", "<i2"), ("rgb", "u1", 3), ("pad", "u1")]))
    rec["tsdf"], rec["weight"] = t, w
    rec["rgb"] = c.reshape(-1, 4)[:, :3]
    return rec


def settled_volume(intr, depth_mm):
    """Free space settled, the rest untouched: weight 64 at the fixed point
    where the voxel lies at least 0.25 m in front of the depth its pixel shows
    (camera at the origin, volume pose translate(-L/2, -L/2, 0.5)), zero
    elsewhere, so the frames still build their surfaces from weight 0."""
    vs = L_VOL / N
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    px, py, pz = x * vs - L_VOL / 2, y * vs - L_VOL / 2, z * vs + 0.5
    u = np.rint(px / pz * intr.fx + intr.cx).astype(np.int64)
    v = np.rint(py / pz * intr.fy + intr.cy).astype(np.int64)
    inside = (u >= 0) & (u < intr.width) & (v >= 0) & (v < intr.height)
    d = np.where(inside, depth_mm[np.clip(v, 0, intr.height - 1), np.clip(u, 0, intr.width - 1)] * 0.001, 0.0)
    free = (inside & (d > 0) & (d - np.sqrt(px * px + py * py + pz * pz) >= 0.25)).ravel()
    n = N ** 3
    t = np.where(free, tsat(), 0).astype(np.int16)
    w = np.where(free, 64, 0).astype(np.int16)
    return t, w, np.zeros(4 * n, np.uint8)


def unsettled_volume(seed):
    rng = np.random.default_rng(seed)
    n = N ** 3
    w = rng.choice(np.array([0, 1, 30, 63, 64], np.int16), n)
    t = rng.integers(-32767, 32768, n).astype(np.int16)
    t[w == 0] = 0
    c = rng.integers(0, 256, 4 * n, dtype=np.uint8)
    c.reshape(-1, 4)[:, 3] = 0
    c.reshape(-1, 4)[w == 0] = 0
    return t, w, c


def upload_both(kf, pipe, vol):
    t, w, c = vol
    kf.upload_tsdf(records(t, w, c))
    n = N ** 3
    np.ctypeslib.as_array(O.lib().kfo_pipe_tsdf(pipe.h), shape=(n,))[:] = t
    np.ctypeslib.as_array(O.lib().kfo_pipe_weight(pipe.h), shape=(n,))[:] = w
    np.ctypeslib.as_array(O.lib().kfo_pipe_rgb(pipe.h), shape=(4 * n,))[:] = c


def assert_same(kf, pipe, what):
    gp, op = kf.pose_record, pipe.poses()
    assert gp.shape == op.shape and np.abs(gp - op).max() == 0, f"{what}: poses"
    for l in range(3):
        _, gv, gn = kf.frame_maps(KFX_FRAME_PREV, l)
        assert feq(gv, pipe.map(1, 1, l)) and feq(gn, pipe.map(1, 2, l)), f"{what}: PREV maps level {l}"
    t, w, c = kf.volume_soa()
    ot, ow, oc = pipe.volume()
    assert np.array_equal(t, ot), f"{what}: tsdf, {(t != ot).sum()} voxels differ"
    assert np.array_equal(w, ow), f"{what}: weight, {(w != ow).sum()} voxels differ"
    assert np.array_equal(c, oc), f"{what}: rgb, {(c != oc).sum()} bytes differ"


@pytest.fixture(scope="module")
def intr():
    return synth.Intrinsics.qvga()


@pytest.fixture(scope="module")
def static_frames(intr):
    """4 frames of the default scene from one pose (noise and 0.2 % dropouts
    differ per frame) and a fifth with a sphere put into the free space."""
    scene = synth.Scene.default(L_VOL)
    pose = np.eye(4)
    fr = [synth.render(scene, intr, pose, noise_seed=100 + k, dropout=0.002) for k in range(4)]
    scene.spheres.append((np.array([-0.05 * L_VOL, -0.12 * L_VOL, 0.5 + 0.42 * L_VOL]), 0.07 * L_VOL))
    fr.append(synth.render(scene, intr, pose, noise_seed=104, dropout=0.002))
    return [(b, d.astype(np.float32)) for b, d in fr]


@pytest.fixture(scope="module")
def moving(intr):
    """10 frames of a moving trajectory and the oracle's result from the settled volume."""
    bgr, dep, _ = synth.sequence(10, intr, noise=True, dropout=0.005, traj_seed=7, amp_t=0.16, period=60.0)
    dep = dep.astype(np.float32)
    p = default_params(dims=N, range_m=L_VOL)
    pipe = O.Pipeline(Intrinsics.from_any(intr), p)
    t, w, c = settled_volume(intr, dep[0])
    n = N ** 3
    np.ctypeslib.as_array(O.lib().kfo_pipe_tsdf(pipe.h), shape=(n,))[:] = t
    np.ctypeslib.as_array(O.lib().kfo_pipe_weight(pipe.h), shape=(n,))[:] = w
    np.ctypeslib.as_array(O.lib().kfo_pipe_rgb(pipe.h), shape=(4 * n,))[:] = c
    ost = [pipe.process(bgr[k], dep[k]) for k in range(10)]
    assert ost == [KFX_OK] * 10
    return bgr, dep, pipe


def run_static(intr, static_frames, force64=False):
    """Case a: returns the open context and oracle after 3 static frames."""
    p = default_params(dims=N, range_m=L_VOL)
    I = Intrinsics.from_any(intr)
    kf = KinectFusion(I, p)
    if force64:
        kf.debug_force_index64(True)
    kf.debug_count_settled(True)
    pipe = O.Pipeline(I, p)
    upload_both(kf, pipe, settled_volume(intr, static_frames[0][1]))
    assert kf.debug_get_settled()[0] == 0  # an upload leaves no byte set
    for k in range(3):
        b, d = static_frames[k]
        assert kf.pipeline(b, d) == pipe.process(b, d) == KFX_OK
        nset, nskip = kf.debug_get_settled()
        print(f"frame {k + 1}: {nset} bricks set, {nskip} skipped")
        assert nset > 0
        assert (nskip > 0) == (k >= 1), (k, nskip)
        assert_same(kf, pipe, f"static frame {k + 1}")
    return kf, pipe


def test_a_static_scene_skips_from_frame_two(intr, static_frames):
    kf, _ = run_static(intr, static_frames)
    kf.close()


def test_b_surface_enters_settled_space(intr, static_frames):
    kf, pipe = run_static(intr, static_frames)
    before = kf.debug_get_settled()[0]
    b, d = static_frames[4]
    assert kf.pipeline(b, d) == pipe.process(b, d) == KFX_OK
    after = kf.debug_get_settled()[0]
    print(f"bricks set {before} -> {after}")
    assert after < before  # the sphere's bricks were stored into
    assert_same(kf, pipe, "frame with the new surface")
    b, d = static_frames[3]
    assert kf.pipeline(b, d) == pipe.process(b, d)
    assert_same(kf, pipe, "frame after it")
    kf.close()


def test_c_moving_trajectory(intr, moving):
    bgr, dep, pipe = moving
    kf = KinectFusion(Intrinsics.from_any(intr), default_params(dims=N, range_m=L_VOL))
    kf.debug_count_settled(True)
    kf.upload_tsdf(records(*settled_volume(intr, dep[0])))
    skipped = 0
    for k in range(10):
        assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        skipped += kf.debug_get_settled()[1]
    print(f"{skipped} bricks skipped over 10 frames, {kf.debug_get_settled()[0]} set at the end")
    assert skipped > 0
    assert_same(kf, pipe, "10 moving frames")
    kf.close()


def test_d_reset_then_unsettled_upload(intr, static_frames):
    kf, pipe = run_static(intr, static_frames)
    b = static_frames[0][0]
    blank = np.zeros_like(static_frames[0][1])
    assert kf.pipeline(b, blank) == pipe.process(b, blank) == KFX_TRACKING_LOST  # reset
    assert kf.debug_get_settled()[0] == 0
    assert_same(kf, pipe, "after the reset")
    upload_both(kf, pipe, settled_volume(intr, static_frames[0][1]))
    for k in (0, 1):
        b, d = static_frames[k]
        assert kf.pipeline(b, d) == pipe.process(b, d)
    assert kf.debug_get_settled()[0] > 0
    upload_both(kf, pipe, unsettled_volume(5))
    assert kf.debug_get_settled()[0] == 0
    for k in (2, 3):
        b, d = static_frames[k]
        assert kf.pipeline(b, d) == pipe.process(b, d)
        assert_same(kf, pipe, f"frame {k - 1} after the unsettled upload")
    kf.close()


def test_e_static_scene_index64(intr, static_frames):
    kf, _ = run_static(intr, static_frames, force64=True)
    kf.close()


@pytest.mark.parametrize("gmode", [1, 2])
def test_f_staged_overlapped_frames(intr, moving, gmode):
    bgr, dep, pipe = moving
    kf = KinectFusion(Intrinsics.from_any(intr), default_params(dims=N, range_m=L_VOL))
    kf.debug_count_settled(True)
    kf.upload_tsdf(records(*settled_volume(intr, dep[0])))
    kf.set_graph_mode(gmode)
    kf.set_frame_overlap(True)
    kf.stage_frames(bgr, dep)
    for k in range(10):
        kf.pipeline_staged(k)
    assert kf.synchronize() == KFX_OK
    assert kf.debug_get_settled()[0] > 0
    assert_same(kf, pipe, f"staged frames, graph mode {gmode}")  # = the single-stream frames of case c
    kf.close()
