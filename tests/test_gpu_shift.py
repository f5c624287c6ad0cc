"""The moving volume on the GPU: kfx_shift_volume, kfx_evict_points and the
follow mode of examples/kfx_run against the references of shift_cases.py (numpy roll-and-clear,
the float32 pose restatement, StagePipeline and the oracle's extraction), bit for bit.
Volumes are 64^3 and the non-cubic 128 x 64 x 32 (other tile and brick counts per axis);
frames are QVGA, the smallest image the default three-level ICP tracks."""
import os
import re
import subprocess

import numpy as np
import pytest

import integrate_cases as IC
import oracle as O
import pngw
import shift_cases as SC
import kfx
from kfx import KFX_FRAME_PREV, KFX_OK, KinectFusion, KfxError, synth
from kfx.abi import Intrinsics, default_params

pytestmark = pytest.mark.gpu
RUNNER = os.path.join(os.path.dirname(kfx.LIB_PATH), "kfx_run")


def code_of(err) -> int:
    return int(re.search(r"failed \((-?\d+)\)", str(err.value)).group(1))


def assert_volume(kf, want, what):
    for a, b, name in zip(kf.volume_soa(), want, ("tsdf", "weight", "rgb")):
        assert np.array_equal(a, b), f"{what}: {name}, {(a != np.asarray(b)).sum()} entries differ"


def assert_same(kf, sp, what):
    gp, op = kf.pose_record, sp.pose_matrices()
    assert gp.shape == op.shape and np.array_equal(gp.view(np.uint32), op.view(np.uint32)), f"{what}: poses"
    for l in range(sp.L):
        _, gv, gn = kf.frame_maps(KFX_FRAME_PREV, l)
        assert SC.feq(gv, sp.pv[l]) and SC.feq(gn, sp.pn[l]), f"{what}: PREV maps level {l}"
    assert_volume(kf, sp.volume(), what)
    assert kf.volume_origin == tuple(sp.origin), f"{what}: origin"
    assert np.array_equal(kf.volume_pose.view(np.uint32), sp.vpose.matrix().view(np.uint32)), f"{what}: volume pose"


def new_kf(dims=(64, 64, 64)):
    return KinectFusion(Intrinsics.from_any(SC.qvga()), SC.params(dims))


# ---- 1. contents ---------------------------------------------------------------

def shift_table(dims):
    X, Y, Z = dims
    one = [tuple(sg * m if k == a else 0 for k in range(3)) for a in range(3) for m in (8, 16) for sg in (1, -1)]
    # a depth that is no multiple of 8: along z, shifts that leave part of a brick group (the +-8 above too)
    part = [(0, 0, 40), (0, 0, -40), (8, 0, -40)] if Z % 8 else []
    return one + part + [(8, -16, 24), (-8, -8, -8), (X, 0, 0), (0, -Y, 0), (0, 0, (Z + 7) // 8 * 8 + 8), (-X - 16, 8, 0), (0, 0, 0)]


@pytest.mark.parametrize("force64", [False, True])
@pytest.mark.parametrize("dims", [(64, 64, 64), (128, 64, 32), (64, 40, 44)])
def test_contents(dims, force64):
    p = SC.params(dims)
    t, w, c = IC.random_volume(dims)
    rec = IC.records(t, w, c)
    origin = np.zeros(3, np.int64)
    with new_kf(dims) as kf:
        if force64:
            kf.debug_force_index64(True)
        for s in shift_table(dims):
            kf.upload_tsdf(rec)
            kf.shift_volume(s)
            origin += s
            assert_volume(kf, SC.shift_soa(t, w, c, dims, s), f"shift {s}")
            assert kf.volume_origin == tuple(int(x) for x in origin), s
            assert np.array_equal(kf.volume_pose.view(np.uint32),
                                  SC.volume_pose(p, origin).matrix().view(np.uint32)), f"pose after {s}"
        # two shifts in a row = their sum where nothing left the box in between (same sign per axis)
        kf.upload_tsdf(rec)
        kf.shift_volume((8, 0, 0))
        kf.shift_volume((8, -8, 16))
        assert_volume(kf, SC.shift_soa(t, w, c, dims, (16, -8, 16)), "two shifts")
        print(f"{dims} force64={force64}: last shift {kf.shift_ms()['shift']:.3f} ms")


# ---- 2. arguments ---------------------------------------------------------------

def test_arguments():
    dims = (64, 64, 64)
    t, w, c = IC.random_volume(dims)
    with new_kf(dims) as kf:
        kf.upload_tsdf(IC.records(t, w, c))
        kf.shift_volume((0, 8, 0))
        before = (kf.volume_soa(), kf.volume_origin, kf.volume_pose)
        for bad in ((4, 0, 0), (0, -12, 0), (8, 8, 1), None):
            with pytest.raises(KfxError) as e:
                kf.shift_volume(bad)
            assert code_of(e) == -1, bad
            with pytest.raises(KfxError) as e:
                kf.evict_points(bad)
            assert code_of(e) == -1, bad
        assert_volume(kf, before[0], "after refused shifts")
        assert kf.volume_origin == before[1] == (0, 8, 0) and np.array_equal(kf.volume_pose, before[2])
        assert kf.evict_count((0, 0, 0)) == 0 and len(kf.evict_points((0, 0, 0))) == 0
    with KinectFusion(Intrinsics.from_any(SC.qvga()), SC.params(dims), slab=(0, 2)) as sl:
        for call in (sl.shift_volume, sl.evict_points):
            with pytest.raises(KfxError) as e:
                call((8, 0, 0))
            assert code_of(e) == -4
        assert sl.volume_origin == (0, 0, 0)


# ---- 3. stages after a shift ----------------------------------------------------

def test_stages_after_a_shift():
    bgr, dep, _ = SC.frames(12)
    sp = SC.StagePipeline(SC.qvga(), SC.params(64))
    with new_kf() as kf:
        for k in range(4):
            assert kf.pipeline(bgr[k], dep[k]) == sp.process(bgr[k], dep[k]) == KFX_OK
        s = (8, 0, -8)
        kf.shift_volume(s)
        sp.shift(s)
        assert_same(kf, sp, "after the shift")
        ds, _, _ = O.preprocess(dep[4], sp.intr, sp.p)
        v2c = sp.vol2cam()
        O.integrate(sp.vol, float(sp.p.volu_trun_dist), sp.intr, v2c, ds[0], bgr[4])
        kf.stage_preprocess(bgr[4], dep[4])
        kf.stage_integrate(v2c)
        assert_volume(kf, sp.volume(), "stage_integrate on the shifted volume")
        c2v, Rinv = sp.cam2vol()
        maps = [O.raycast(sp.vol, sp.intr, c2v, Rinv)]
        for _ in range(1, sp.L):
            maps.append(O.resize_points_normals(*maps[-1]))
        kf.stage_raycast(c2v, Rinv)
        for l in range(sp.L):  # the skip maps are adequate for the new contents
            _, gv, gn = kf.frame_maps(KFX_FRAME_PREV, l)
            assert SC.feq(gv, maps[l][0]) and SC.feq(gn, maps[l][1]), f"stage_raycast level {l}"
        assert np.isfinite(maps[0][0]).any() and (maps[0][1] != 0).any()


# ---- 4. settled bytes -----------------------------------------------------------

def test_settled_bytes_follow_the_shift():
    """The shift rebuilds the skip maps and clears the settled bytes.

    Seen to fail on a build whose shift left the settled bytes where they were: the frames after
    the shift then differ from StagePipeline in the weights of bricks skipped on a stale byte.

    The volume is integrate_cases.settled_volume's values over the scene's free space only
    (shift_cases.settled_free_volume, the construction of test_gpu_settled.py): with every voxel
    at weight 64 no frame's surface reaches a zero crossing, the raycast finds nothing and the
    reference loses tracking on the third frame."""
    intr = SC.qvga()
    scene = synth.Scene.default(SC.L_VOL)
    fr = [synth.render(scene, intr, np.eye(4), noise_seed=100 + k, dropout=0.002) for k in range(4)]
    fr = [(b, d.astype(np.float32)) for b, d in fr]
    p = SC.params(64)
    sp = SC.StagePipeline(intr, p)
    vol = SC.settled_free_volume((64, 64, 64), intr, fr[0][1], p)
    sp.set_volume(*vol)
    with new_kf() as kf:
        kf.debug_count_settled(True)
        kf.upload_tsdf(IC.records(*vol))
        assert kf.pipeline(*fr[0]) == sp.process(*fr[0]) == KFX_OK
        nset = kf.debug_get_settled()[0]
        assert nset > 0
        # contents move one brick towards the camera: bricks whose byte was set now hold the
        # voxels of the brick behind them, nearer the surfaces, which the next frames change
        s = (0, 0, 8)
        kf.shift_volume(s)
        sp.shift(s)
        assert_same(kf, sp, "after the shift")
        for k in range(1, 4):
            assert kf.pipeline(*fr[k]) == sp.process(*fr[k]) == KFX_OK
            n1, nskip = kf.debug_get_settled()
            print(f"frame {k} after the shift: {n1} bricks set, {nskip} skipped (before the shift {nset} set)")
            assert_same(kf, sp, f"frame {k} after the shift")
        assert nskip > 0  # the skip is not simply dead


# ---- 5. pipeline across shifts --------------------------------------------------

@pytest.mark.parametrize("mode", ["graph0", "graph1", "staged", "staged_overlap"])
def test_pipeline_across_shifts(mode):
    sp, _ = SC.pipeline_reference()
    bgr, dep, _ = SC.frames(12)
    with new_kf() as kf:
        kf.set_graph_mode(0 if mode == "graph0" else 1)
        if mode.startswith("staged"):
            kf.set_frame_overlap(mode == "staged_overlap")
            kf.stage_frames(bgr, dep)
        for k in range(12):
            if k in (4, 8):
                kf.shift_volume(SC.PIPE_SHIFTS[k // 4 - 1])  # (staged: no synchronize in between)
            if mode.startswith("staged"):
                kf.pipeline_staged(k)
            else:
                assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        assert kf.synchronize() == KFX_OK
        assert_same(kf, sp, mode)
        assert kf.frame_count == sp.frame_count


# ---- 6. eviction ----------------------------------------------------------------

def test_eviction():
    vol, vpose, p = SC.fused_volume()
    bgr, dep, _ = SC.frames(12)
    with new_kf() as kf, new_kf() as kf2:
        for k in range(4):
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        assert_volume(kf, (vol.tsdf, vol.weight, vol.rgb), "the fused volume")
        state = (kf.pose_record, [kf.frame_maps(KFX_FRAME_PREV, l) for l in range(3)], kf.volume_soa())
        full = kf.extract_points_attr()
        ofull, n = O.extract_points(vol, vpose)
        assert len(full) == n and np.array_equal(full["xyz"].view(np.uint32), ofull.view(np.uint32))
        rec = IC.records(vol.tsdf, vol.weight, vol.rgb)
        for s in SC.EVICT_SHIFTS + ((0, 0, 64),):
            mask = SC.evicted_mask(vol, vpose, s)
            ev = kf.evict_points(s)
            print(f"shift {s}: {len(ev)} of {len(full)} items evicted, {kf.shift_ms()['evict']:.3f} ms")
            assert len(ev) == mask.sum() and ev.tobytes() == full[mask].tobytes(), s
            assert 0 < len(ev) and (len(ev) < len(full) or s == (0, 0, 64))
            assert kf.evict_count(s) == len(ev)  # cap = 0 counts only
            half = kf.evict_points(s, cap=len(ev) // 2)
            assert half.tobytes() == ev[:len(ev) // 2].tobytes()  # a cap below the total: the prefix
            kf2.upload_tsdf(rec)
            kf2.shift_volume(s)
            assert len(full) == len(ev) + kf2.extract_count(attr=True), s
        # the calls left poses, maps and volume alone
        assert np.array_equal(kf.pose_record, state[0]) and kf.volume_origin == (0, 0, 0)
        for l in range(3):
            for a, b in zip(kf.frame_maps(KFX_FRAME_PREV, l), state[1][l]):
                assert SC.feq(a, b)
        assert_volume(kf, state[2], "after the evictions")
        sp = SC.StagePipeline(SC.qvga(), p)  # and tracking goes on as if they had not happened
        for k in range(5):
            assert sp.process(bgr[k], dep[k]) == KFX_OK
        assert kf.pipeline(bgr[4], dep[4]) == KFX_OK
        assert_same(kf, sp, "the frame after the evictions")


def test_eviction_short_last_group():
    """Z = 44: the last brick group holds 4 slices.  A shift towards the top drops part of it and
    the group below; one away from the bottom leaves it alone."""
    import extract_cases as EC
    dims = (32, 24, 44)
    p = SC.params(dims)
    t, w, rgb = EC.dense(dims)
    vol = O.Volume(dims, [float(r) for r in p.volu_range])
    vol.tsdf[:], vol.weight[:] = t, w
    vol.rgb.reshape(-1, 4)[:, :3] = rgb
    vpose = SC.volume_pose(p, (0, 0, 0))
    with new_kf(dims) as kf:
        kf.upload_tsdf(EC.records(t, w, rgb))
        full = kf.extract_points_attr()
        ofull, n = O.extract_points(vol, vpose)
        assert len(full) == n and np.array_equal(full["xyz"].view(np.uint32), ofull.view(np.uint32))
        for s in ((0, 0, -8), (0, 0, 16)):
            mask = SC.evicted_mask(vol, vpose, s)
            ev = kf.evict_points(s)
            assert len(ev) == mask.sum() and ev.tobytes() == full[mask].tobytes(), s
            assert 0 < len(ev) < len(full)
            assert kf.evict_count(s) == len(ev)
            half = kf.evict_points(s, cap=len(ev) // 2)
            assert half.tobytes() == ev[:len(ev) // 2].tobytes()


# ---- 7. reset -------------------------------------------------------------------

def test_reset_returns_the_origin():
    bgr, dep, _ = SC.frames(12)
    p = SC.params(64)
    I = Intrinsics.from_any(SC.qvga())
    with new_kf() as kf:
        for k in range(2):
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        kf.shift_volume((8, -8, 16))
        assert kf.volume_origin == (8, -8, 16)
        kf.reset()
        assert kf.volume_origin == (0, 0, 0)
        assert np.array_equal(kf.volume_pose.view(np.uint32), p.volu_pose.matrix().view(np.uint32))
        pipe = O.Pipeline(I, p)
        for k in range(4):
            assert kf.pipeline(bgr[k], dep[k]) == pipe.process(bgr[k], dep[k]) == KFX_OK
        assert np.array_equal(kf.pose_record.view(np.uint32), pipe.poses().view(np.uint32))
        for l in range(3):
            _, gv, gn = kf.frame_maps(KFX_FRAME_PREV, l)
            assert SC.feq(gv, pipe.map(1, 1, l)) and SC.feq(gn, pipe.map(1, 2, l))
        assert_volume(kf, pipe.volume(), "4 frames after the reset")


# ---- 8. runner ------------------------------------------------------------------

def test_runner_follows_the_camera(tmp_path):
    """kfx_run's seventh argument against the binding's own follow loop at the runner's
    parameters (the reference defaults, 512^3 over 3 m).  A shift needs the point 2 m ahead of
    the camera to move 4 voxels = 23 mm; the trajectory's amplitude is raised to 0.16 m over a
    60-frame period (about 17 mm a frame, which test_gpu_settled.py's frames show the ICP
    tracks), so 5 frames bring several shifts, which the binding's loop confirms below."""
    intr = SC.qvga()
    bgr, dep, _ = synth.sequence(5, intr, noise=True, dropout=0.01, amp_t=0.16, period=60.0)
    root = str(tmp_path / "ds")
    os.makedirs(os.path.join(root, "color"))
    os.makedirs(os.path.join(root, "depth"))
    for k in range(len(dep)):
        pngw.write_png(os.path.join(root, "color", f"{k:06d}.png"), bgr[k][:, :, ::-1], 8, 2, idat_parts=1)
        pngw.write_png(os.path.join(root, "depth", f"{k:06d}.png"), dep[k], 16, 0, idat_parts=1)
    with open(os.path.join(root, "intr.txt"), "w") as f:
        f.write(f"{intr.fx} 0 {intr.cx}\n0 {intr.fy} {intr.cy}\n0 0 1\n")

    p = default_params()
    ahead = float(np.float32(0.5) + np.float32(p.volu_range[2]) / np.float32(2))
    evicted, shifts = [], 0
    with KinectFusion(Intrinsics.from_any(intr), p) as kf:
        for k in range(len(dep)):
            assert kf.pipeline(bgr[k], dep[k].astype(np.float32)) == KFX_OK
            s = kfx.shift_for_pose(p, kf.volume_pose, kf.getCurCameraPose(), ahead)
            assert s == SC.shift_for_pose(p, kf.volume_pose, kf.getCurCameraPose(), ahead)
            if any(s):
                evicted.append(kf.evict_points(s))
                kf.shift_volume(s)
                shifts += 1
        cloud = np.concatenate(evicted + [kf.extract_points_attr()])
        kfx.write_ply_attr(str(tmp_path / "want.ply"), cloud)
        kf.write_poses_txt(str(tmp_path / "want.txt"))
    assert shifts >= 1

    out = tmp_path / "followed.ply"
    skip = [""] * 4  # no plain cloud, coloured cloud, mesh or view
    r = subprocess.run([RUNNER, root, str(tmp_path / "poses.txt")] + skip + [str(out)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"followed: (\d+) shifts, (\d+) evicted points", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == shifts >= 1 and int(m.group(2)) == sum(len(e) for e in evicted)
    assert open(tmp_path / "poses.txt").read() == open(tmp_path / "want.txt").read()
    got, want = open(out).read(), open(tmp_path / "want.ply").read()
    assert got.startswith(f"ply\nformat ascii 1.0\nelement vertex {len(cloud)}\n")
    assert got == want
