"""Free-viewpoint render on the GPU (kfx_render_view): maps equal
to the oracle's raycast at the view, Phong / normal images equal to the
oracle's shader on them, the colour image equal to the integer restatement
(view_cases.py), all bit for bit; and the call leaves tracking untouched."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import kfx
import view_cases as VC
from kfx import KFX_FRAME_PREV, KFX_OK, KFX_TRACKING_LOST, KinectFusion, synth
from kfx.abi import Intrinsics, Pose, default_params

pytestmark = pytest.mark.gpu
KINDS = ("phong", "normal", "color")


def fused_ctx(dims):
    intr, bgr, dep = VC.scene()
    kf = KinectFusion(Intrinsics.from_any(intr), VC.params(dims))
    for k in range(VC.N_FRAMES):
        assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
    return kf


@functools.lru_cache(maxsize=None)
def refs(dims):
    last = VC.fused(dims)[3][-1]
    return [(name, intr, pose, VC.reference(dims, intr, pose)) for name, intr, pose in VC.views(last)]


def check_views(kf, dims):
    t, _, c = kf.volume_soa()
    ot, _, oc, poses = VC.fused(dims)
    assert np.array_equal(t, ot) and np.array_equal(c.reshape(-1, 4), oc)  # the references' volume
    assert np.array_equal(kf.pose_record, poses)
    for name, intr, pose, ref in refs(dims):
        for kind in KINDS:
            img, v, n, ts = kf.render_view(intr, pose, kind, maps=True)
            assert np.array_equal(v.view(np.uint32), ref["vmap"].view(np.uint32)), (name, kind)
            assert np.array_equal(n.view(np.uint32), ref["nmap"].view(np.uint32)), (name, kind)
            assert np.array_equal(ts.view(np.uint32), ref["ts"].view(np.uint32)), (name, kind)
            assert np.array_equal(img, ref[kind]), (name, kind)
            assert np.array_equal(kf.render_view(intr, pose, kind), img), (name, kind)  # without the maps
            if name == "miss":
                assert not img.any() and not ts.any()
    assert kf.view_ms() > 0.0


@pytest.mark.parametrize("dims", VC.DIMS)
def test_view_parity(dims):
    kf = fused_ctx(dims)
    check_views(kf, dims)
    kf.close()


def test_view_index64_same_bytes():
    kf = fused_ctx(64)
    kf.debug_force_index64(True)
    check_views(kf, 64)
    kf.close()


def test_view_from_tracker_camera_matches_frame_maps():
    kf = fused_ctx(64)
    _, pv, pn = kf.frame_maps(KFX_FRAME_PREV, 0)
    img, v, n, ts = kf.render_view(kf.intr, kf.pose_record[-1], "phong", maps=True)
    assert pn.any()
    assert np.array_equal(v.view(np.uint32), pv.view(np.uint32))
    assert np.array_equal(n.view(np.uint32), pn.view(np.uint32))
    assert np.array_equal(img, kf.render("phong"))
    assert np.array_equal(kf.render_view(kf.intr, kf.pose_record[-1], "normal"), kf.render("normal"))
    kf.close()


def _state(kf):
    maps = [kf.frame_maps(KFX_FRAME_PREV, l)[1:] for l in range(kf.params.pyramid_height)]
    return kf.pose_record, maps, kf.volume_soa()


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("graph", [0, 1])
def test_view_does_not_disturb_tracking(graph, overlap, staged):
    intr = synth.Intrinsics.qvga()
    bgr, dep, _ = synth.sequence(6, intr, noise=True, dropout=0.01)
    dep = dep.astype(np.float32)
    big_i, big_p = VC.make_view(VC.VIEW_BIG, np.eye(4, dtype=np.float32))
    states = []
    for with_views in (True, False):
        kf = KinectFusion(Intrinsics.from_any(intr), VC.params(64))
        kf.set_graph_mode(graph)
        kf.set_frame_overlap(overlap)
        if staged:
            kf.stage_frames(bgr, dep)
            assert kf.synchronize() == KFX_OK
        for k in range(len(dep)):
            if staged:
                kf.pipeline_staged(k)  # no explicit sync before the views
            else:
                assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
            if with_views:
                for kind in KINDS:
                    img = kf.render_view(big_i, big_p, kind, maps=(kind == "color"))
                assert k == 0 or img[0].any()
        assert kf.synchronize() == KFX_OK
        states.append(_state(kf))
        kf.close()
    (pa, ma, va), (pb, mb, vb) = states
    assert len(pa) == len(dep) and np.array_equal(pa, pb)
    for (v0, n0), (v1, n1) in zip(ma, mb):
        assert np.array_equal(v0.view(np.uint32), v1.view(np.uint32))
        assert np.array_equal(n0.view(np.uint32), n1.view(np.uint32))
    for a, b in zip(va, vb):
        assert np.array_equal(a, b)


def test_view_leaves_pending_tracking_status():
    intr, bgr, dep = VC.scene()
    kf = KinectFusion(Intrinsics.from_any(intr), VC.params(64))
    kf.pipeline_async(bgr[0], dep[0])
    kf.pipeline_async(bgr[1], dep[1])
    kf.pipeline_async(bgr[2], np.zeros_like(dep[2]))  # no depth: ICP det check fails, reset, frame dropped
    img = kf.render_view(kf.intr, np.eye(4, dtype=np.float32), "phong")
    assert not img.any()  # the volume was reset
    assert kf.synchronize() == KFX_TRACKING_LOST
    assert kf.synchronize() == KFX_OK
    kf.close()


def test_view_buffers_grow():
    kf = fused_ctx(64)
    last = kf.pose_record[-1]
    small, big = VC.make_view(VC.VIEW_ODD, last), VC.make_view(VC.VIEW_BIG, last)
    first = kf.render_view(*small, "color", maps=True)
    mid = kf.render_view(*big, "color", maps=True)
    again = kf.render_view(*small, "color", maps=True)
    assert mid[0].shape == (300, 400, 3) and mid[0].any()
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    kf.close()


def test_view_argument_table():
    kf = fused_ctx(64)
    L = kfx.lib()
    good_i = Intrinsics(64, 48, 60.0, 60.0, 31.5, 23.5)
    good_p = Pose.from_matrix(kf.pose_record[-1])
    out = np.zeros(1 << 16, np.uint8)
    op = out.ctypes.data_as(C.POINTER(C.c_uint8))

    def call(i=good_i, p=good_p, kind=0, o=op):
        return L.kfx_render_view(kf._h, C.byref(i) if i is not None else None, C.byref(p) if p is not None else None,
                                 kind, o, None, None, None)

    def intr(**kw):
        d = dict(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5)
        d.update(kw)
        return Intrinsics(d["width"], d["height"], d["fx"], d["fy"], d["cx"], d["cy"])

    def pose(idx, val):
        m = Pose.from_matrix(kf.pose_record[-1])
        if idx < 9:
            m.R[idx] = val
        else:
            m.t[idx - 9] = val
        return m

    assert call() == KFX_OK
    assert call(i=None) == -1 and call(p=None) == -1 and call(o=None) == -1
    assert call(kind=-1) == -1 and call(kind=3) == -1
    for bad in (intr(width=0), intr(height=0), intr(width=-5), intr(width=1 << 14, height=(1 << 12) + 1),
                intr(fx=0.0), intr(fy=0.0), intr(fx=float("nan")), intr(fy=float("inf")), intr(cx=float("nan")),
                intr(cy=float("-inf"))):
        assert call(i=bad) == -1, (bad.width, bad.height, bad.fx, bad.fy, bad.cx, bad.cy)
    for idx in (0, 4, 8, 9, 11):
        assert call(p=pose(idx, float("nan"))) == -1 and call(p=pose(idx, float("inf"))) == -1
    assert call() == KFX_OK  # the context is still usable
    kf.close()
    sl = KinectFusion(Intrinsics.from_any(synth.Intrinsics.qvga()), VC.params(64), slab=(0, 2))
    assert L.kfx_render_view(sl._h, C.byref(good_i), C.byref(good_p), 0, op, None, None, None) == -4
    sl.close()


def test_runner_writes_colour_view(tmp_path):
    from test_gpu_dataset import RUNNER, _write
    intr = synth.Intrinsics.qvga()
    bgr, dep, _ = synth.sequence(4, intr, noise=True, dropout=0.01)
    root = str(tmp_path / "ds")
    _write(root, bgr, dep, intr)
    ds = kfx.Dataset(root)
    kf = KinectFusion(ds.intrinsics, default_params())  # the runner's parameters
    for k in range(len(ds)):
        c, d = ds.read(k)
        kf.pipeline(c, d)
    want = tmp_path / "want.ppm"
    kfx.write_ppm(str(want), kf.render_view(ds.intrinsics, kf.getCurCameraPose(), "color"))
    kf.close()
    ds.close()
    got = tmp_path / "view.ppm"
    r = subprocess.run([RUNNER, root, str(tmp_path / "poses.txt"), str(tmp_path / "a.ply"), str(tmp_path / "b.ply"),
                        str(tmp_path / "c.ply"), str(got)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    data = open(got, "rb").read()
    assert data.startswith(b"P6\n320 240\n255\n") and any(data[15:])
    assert data == open(want, "rb").read()
