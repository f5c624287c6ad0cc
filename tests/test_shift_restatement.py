"""The moving volume's references on the CPU: shift_cases.StagePipeline against
oracle.Pipeline (the harness is pinned before anything is judged by it), the counting identity
of eviction on the oracle alone, and the host rule kfx_shift_for_pose."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import shift_cases as SC
from kfx import synth
from kfx.abi import Intrinsics, Params, Pose, default_params


def test_stage_pipeline_equals_oracle_pipeline():
    intr = synth.Intrinsics.qvga()
    bgr, dep, _ = synth.sequence(6, intr)
    p = default_params(dims=64, range_m=SC.L_VOL)
    I = Intrinsics.from_any(intr)
    pipe, sp = O.Pipeline(I, p), SC.StagePipeline(I, p)
    for k in range(6):
        d = dep[k].astype(np.float32)
        a, b = pipe.process(bgr[k], d), sp.process(bgr[k], d)
        assert a == b, f"frame {k}: status {a} vs {b}"
        assert np.array_equal(pipe.poses().view(np.uint32), sp.pose_matrices().view(np.uint32)), f"frame {k}: poses"
        for l in range(p.pyramid_height):
            assert SC.feq(pipe.map(1, 1, l), sp.pv[l]) and SC.feq(pipe.map(1, 2, l), sp.pn[l]), \
                f"frame {k}: previous maps, level {l}"
        for x, y, what in zip(pipe.volume(), sp.volume(), ("tsdf", "weight", "rgb")):
            assert np.array_equal(x, y), f"frame {k}: {what}"
    assert pipe.frame_count == sp.frame_count == 7


def test_shift_soa_and_pose_restatement():
    dims = (16, 8, 24)
    n = int(np.prod(dims))
    t = np.arange(1, n + 1, dtype=np.int32)
    c = np.repeat(t.astype(np.uint8), 4)
    s = (8, 0, -16)
    st, sw, sc = SC.shift_soa(t, t, c, dims, s)
    g = t.reshape(dims[2], dims[1], dims[0])
    want = np.zeros_like(g)
    want[16:, :, :8] = g[:8, :, 8:]
    assert np.array_equal(st.reshape(want.shape), want) and np.array_equal(sw, st)
    assert np.array_equal(sc.reshape(-1, 4)[:, 0], st.astype(np.uint8))
    p = default_params(dims=64, range_m=SC.L_VOL)
    q = SC.volume_pose(p, (8, -16, 24)).matrix()
    vs = np.float32(SC.L_VOL) / np.float32(64)
    assert np.array_equal(q[:3, 3], np.float32(p.volu_pose.t[:]) + np.float32([8, -16, 24]) * vs)
    assert np.array_equal(SC.volume_pose(p, (0, 0, 0)).matrix(), p.volu_pose.matrix())


@pytest.mark.parametrize("s", SC.EVICT_SHIFTS + ((64, 0, 0), (0, 0, 72), (0, 0, 0)))
def test_counting_identity_on_the_oracle(s):
    vol, vpose, p = SC.fused_volume()
    full, n = O.extract_points(vol, vpose)
    mask = SC.evicted_mask(vol, vpose, s)
    t, w, c = SC.shift_soa(vol.tsdf, vol.weight, vol.rgb, SC.fused_volume()[0].dims, s)
    origin = s
    _, nkept = O.extract_points(vol, SC.volume_pose(p, origin), tsdf=t, weight=w)
    print(f"shift {s}: {n} items, {int(mask.sum())} evicted, {nkept} in the shifted volume")
    assert n > 0 and n == int(mask.sum()) + nkept
    if s in SC.EVICT_SHIFTS:  # partial: something leaves, something stays
        assert mask.sum() > 0 and nkept > 0
    elif any(s):
        assert nkept == 0 and mask.all()
    else:
        assert not mask.any()


def test_shifted_extraction_keeps_the_world_points():
    """The kept items come out of the shifted volume at the shifted pose in the same order and
    at the same place: the new pose undoes the move (to the rounding of the float32 pose)."""
    vol, vpose, p = SC.fused_volume()
    s = SC.EVICT_SHIFTS[0]
    full, _ = O.extract_points(vol, vpose)
    mask = SC.evicted_mask(vol, vpose, s)
    t, w, _ = SC.shift_soa(vol.tsdf, vol.weight, vol.rgb, vol.dims, s)
    kept, _ = O.extract_points(vol, SC.volume_pose(p, s), tsdf=t, weight=w)
    assert np.abs(kept - full[~mask]).max() < 1e-5


# ---- kfx_shift_for_pose ------------------------------------------------------

def _cam(t=(0, 0, 0), R=None):
    m = np.eye(4)
    if R is not None:
        m[:3, :3] = R
    m[:3, 3] = t
    return m


def test_shift_for_pose_zero_at_the_default_start(kfx_lib):
    p = default_params()
    ahead = 0.5 + p.volu_range[2] / 2
    assert kfx_lib.shift_for_pose(p, p.volu_pose, _cam(), ahead) == (0, 0, 0)
    q = SC.params((128, 64, 32))
    assert kfx_lib.shift_for_pose(q, q.volu_pose, _cam(), 0.5 + q.volu_range[2] / 2) == (0, 0, 0)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1, -1])
def test_shift_for_pose_one_brick_per_axis(kfx_lib, axis, sign):
    p = default_params()
    vs = 3.0 / 512
    ahead = 0.5 + p.volu_range[2] / 2
    for frac, want in ((1.0, 8), (0.25, 0), (0.75, 8), (1.4, 8), (1.6, 16)):  # bricks; ties lie at .5
        t = [0.0, 0.0, 0.0]
        t[axis] = sign * frac * 8 * vs
        got = kfx_lib.shift_for_pose(p, p.volu_pose, _cam(t), ahead)
        exp = [0, 0, 0]
        exp[axis] = sign * want
        assert got == tuple(exp) == SC.shift_for_pose(p, p.volu_pose.matrix(), _cam(t), ahead), (frac, got)


def test_shift_for_pose_follows_rotation_and_the_volume_pose(kfx_lib):
    p = default_params()
    vs = 3.0 / 512
    ahead = 0.5 + p.volu_range[2] / 2  # 2 m
    Ry = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])  # the camera's +z is the world's +x
    cam = _cam((-ahead + 8 * vs, 0.0, ahead), Ry)       # looks at (8 vs, 0, 2): one brick along x
    assert kfx_lib.shift_for_pose(p, p.volu_pose, cam, ahead) == (8, 0, 0)
    assert SC.shift_for_pose(p, p.volu_pose.matrix(), cam, ahead) == (8, 0, 0)
    # a volume already shifted by that brick has nothing left to do
    assert kfx_lib.shift_for_pose(p, SC.volume_pose(p, (8, 0, 0)), cam, ahead) == (0, 0, 0)
    # a rotated volume pose: the offset is expressed along the volume's own axes
    vp = np.eye(4)
    vp[:3, :3] = Ry
    vp[:3, 3] = Ry @ np.array([-1.5, -1.5, 0.5])
    camr = _cam(Ry @ np.array([0.0, 16 * vs, 0.0]))
    camr[:3, :3] = Ry
    assert kfx_lib.shift_for_pose(p, vp, camr, ahead) == (0, 16, 0)


def test_shift_for_pose_argument_errors(kfx_lib):
    L = kfx_lib.lib()
    p = default_params()
    V, K = p.volu_pose, Pose.identity()
    s = (C.c_int * 3)()
    ok = lambda *a: L.kfx_shift_for_pose(*a)
    assert ok(C.byref(p), C.byref(V), C.byref(K), 2.0, s) == 0
    assert ok(None, C.byref(V), C.byref(K), 2.0, s) == -1
    assert ok(C.byref(p), None, C.byref(K), 2.0, s) == -1
    assert ok(C.byref(p), C.byref(V), None, 2.0, s) == -1
    assert ok(C.byref(p), C.byref(V), C.byref(K), 2.0, None) == -1
    for bad in (float("nan"), float("inf"), -0.5):
        assert ok(C.byref(p), C.byref(V), C.byref(K), bad, s) == -1
    for field, idx in (("R", 4), ("t", 1)):
        for which in (0, 1):
            B = Pose.identity() if which else Pose.from_matrix(p.volu_pose.matrix())
            getattr(B, field)[idx] = float("nan")
            args = (C.byref(p), C.byref(V), C.byref(B)) if which else (C.byref(p), C.byref(B), C.byref(K))
            assert ok(*args, 2.0, s) == -1
