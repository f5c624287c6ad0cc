"""libkfx against the digests recorded from the reference's own kernels
(tests/golden/ref_digests.json, written by tools/ref_digests.py): the device
library's outputs hash to what the reference gave, with no oracle in between.

Expected values come from the fixture only; neither the reference nor
oracle/_ref/ is read.  The oracle is used for two things that are not expected
values: its float pose helpers (pose_inv, pose_mul) form the input poses
exactly as the fixture's cases formed them, and on a mismatch the failure
message counts the elements that differ from the oracle's arrays, to locate
it.  Case ids, output names and hashing are ref_cases.py's.

The smallest shapes of each stage, a fraction of a second each: 64^3-class
volumes under 160x120 frames, 32x32 ICP maps.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import icp_cases as K
import integrate_cases as IC
import oracle as O
import ref_cases as R
import test_gpu_param_space as PS
import test_gpu_ray_chain as RC
from kfx import KFX_FRAME_CUR, KFX_FRAME_PREV, KinectFusion
from kfx.abi import Intrinsics, Pose, default_params

pytestmark = pytest.mark.gpu
f32 = np.float32


def assert_recorded(cid, outputs, fn=None):
    """The outputs (masked as the case masks them) hash to the recorded digest, or equal the recorded sums."""
    outputs, masked = R.masked_outputs(cid, fn, outputs)
    g = R.golden()
    assert masked == g["masked_elements"].get(cid, 0), (cid, masked)
    got, want = R.recorded(cid, outputs), g["cases"][cid]
    if got != want:  # locate it: the oracle is imported for this message only
        run = R.CASES[cid]
        ref, _ = R.masked_outputs(cid, run, run(R.ORACLE))
        where = [f"{n}: {R.differing(a, b)[0]} of {a.size} differ from the oracle" for (n, a), (_, b) in zip(outputs, ref)]
        pytest.fail(f"{cid}: recorded {want!r:.80}, got {got!r:.80}; " + "; ".join(where))


def prev_maps(kf, levels, prefix=""):
    out = []
    for l in range(levels):
        _, v, n = kf.frame_maps(KFX_FRAME_PREV, l)
        out += [(f"{prefix}vmap{l}", v), (f"{prefix}nmap{l}", n)]
    return out


@pytest.mark.parametrize("name,index64", [("base", False), ("oblique", False), ("aniso_oblique", False), ("odd", False),
                                          ("oblique", True)])
def test_integrate_digests(name, index64):
    """stage_integrate after every pose, then the raycast from the last pose's camera."""
    case = IC.CASES[name]
    bgr, depth = IC.frame(case.frame)
    out = []
    with KinectFusion(case.intr, case.params) as kf:
        if index64:
            kf.debug_force_index64(True)
        kf.stage_preprocess(bgr, depth)
        for k, pose in enumerate(case.poses):
            kf.stage_integrate(pose, counts=False)
            t, w, c = kf.volume_soa()
            out += [(f"tsdf@{k}", t), (f"weight@{k}", w), (f"rgb@{k}", c.reshape(-1, 4)[:, :3].copy())]
        cam2vol = O.pose_inv(case.poses[-1])
        kf.stage_raycast(cam2vol, cam2vol.matrix()[:3, :3].T.copy())
        out += prev_maps(kf, case.params.pyramid_height, "ray_")
    assert_recorded(f"int/{name}", out)


def fused_context(name, index64=False):
    """A context of the ray-chain case with the three frames fused on the device as test_gpu_ray_chain.fuse fuses them."""
    intr, bgr, dep, gt = R.qqvga_seq()
    fz, cam2vol, Rinv = R.chain_view(name)
    vp = Pose.from_matrix(RC.FUSED[fz][0])
    kf = KinectFusion(Intrinsics.from_any(intr), RC.case_params(name))
    if index64:
        kf.debug_force_index64(True)
    for k in range(3):
        kf.stage_preprocess(bgr[k], dep[k].astype(f32))
        kf.stage_integrate(O.pose_mul(O.pose_inv(Pose.from_matrix(gt[k])), vp), counts=False)
    kf.stage_raycast(cam2vol, Rinv)
    return kf


@pytest.mark.parametrize("name,index64", [(n, False) for n in RC.CASES] + [("leaving", True)])
def test_raycast_digests(name, index64):
    """stage_raycast's maps at levels 0..2."""
    with fused_context(name, index64) as kf:
        out = prev_maps(kf, 3)
    assert_recorded(f"ray/{name}", out)


def test_render_digests():
    """kfx_render, both types, on the `inside` case's maps (a staged context lights from the
    identity pose it logs at creation: eye = 0, as the fixture's case)."""
    with fused_context("inside") as kf:
        assert np.array_equal(kf.pose_record[-1], np.eye(4, dtype=f32))
        _, v, n = kf.frame_maps(KFX_FRAME_PREV, 0)
        out = [("phong", kf.render("phong")), ("normal", kf.render("normal"))]
    assert_recorded("render/ray/inside", out, SimpleNamespace(render_inputs=(v, n, np.zeros(3, f32))))


@pytest.mark.parametrize("name", K.DEFAULT_THRESHOLD_CASES)
def test_icp_sums_recorded(name):
    """stage_icp_accumulate at the smallest crafted size, identity and moved pose, against the recorded sums."""
    w, h = 32, 32
    case, dist, deg = K.crafted(name, w, h)
    p = default_params(dims=64, range_m=2.048)
    p.pyramid_height = 1
    p.icp_dist_threshold, p.icp_angle_threshold = dist, deg
    for k, n in enumerate((1, 0, 0, 0)):  # test_gpu_icp_crafted.ctx's one-level context
        p.icp_iter_count[k] = n
    with KinectFusion(case.I, p) as kf:
        kf.set_frame_maps(KFX_FRAME_CUR, 0, case.cur_v, case.cur_n)
        kf.set_frame_maps(KFX_FRAME_PREV, 0, case.pre_v, case.pre_n)
        out = [(label, kf.stage_icp_accumulate(0, mk())) for label, mk in R.ICP_POSES]
    assert_recorded(f"icp/crafted/{name}/{w}x{h}", out)


def test_vertex_and_normal_map_digests():
    """The 160x120 frame's vertex and normal maps at three levels."""
    bgr, _, depf = PS.sequence(*PS.QQVGA)
    with KinectFusion(Intrinsics(*PS.QQVGA), PS.params()) as kf:
        kf.stage_preprocess(bgr[0], depf[0])
        out = []
        for l in range(3):
            _, v, n = kf.frame_maps(KFX_FRAME_CUR, l)
            out += [(f"vmap{l}", v), (f"nmap{l}", n)]
    assert_recorded("img/seq_qqvga", out)
