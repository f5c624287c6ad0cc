"""The ICP residual map and quality record on the GPU, every
comparison exact: labels as bytes, residuals as bits, every record field, against
quality_cases.quality_np on crafted maps, on the oracle pipeline's maps after
each frame, and on the oracle's raycast at a world pose; the batch against the
single call; and no call disturbs tracking."""
import ctypes as C
import functools

import numpy as np
import pytest

import icp_cases as K
import kfx
import oracle as O
import quality_cases as Q
import view_cases as VC
from kfx import KFX_FRAME_CUR, KFX_FRAME_PREV, KFX_OK, KFX_TRACKING_LOST, KinectFusion, synth
from kfx.abi import IcpQuality, Intrinsics, Pose, default_params

pytestmark = pytest.mark.gpu

ALL = list(K.case_table())
CRAFTED = [(n, s) for s in Q.SIZES_1PX + [(320, 240)] for n in ALL] + [("a_invalid", (640, 480)),
                                                                       ("b_projection", (640, 480))]
_ctx = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for kf in list(_ctx.values()) + list(_fused.values()):
        kf.close()
    _ctx.clear()
    _fused.clear()


def ctx(I, dist, deg):
    key = (I.width, I.height, float(dist), deg)
    if key not in _ctx:
        p = default_params(dims=64, range_m=2.048)
        p.pyramid_height, p.icp_dist_threshold, p.icp_angle_threshold = 1, dist, deg
        for k in range(4):
            p.icp_iter_count[k] = (1, 0, 0, 0)[k]
        _ctx[key] = KinectFusion(I, p)
    return _ctx[key]


def load(kf, c, level=0):
    kf.set_frame_maps(KFX_FRAME_CUR, level, c.cur_v, c.cur_n)
    kf.set_frame_maps(KFX_FRAME_PREV, level, c.pre_v, c.pre_n)


def same(got, ref, what=""):
    """(record, residual, label) of a call against a quality_np result."""
    q, res, lab = got
    assert np.array_equal(lab, ref.label), (what, int((lab != ref.label).sum()))
    assert np.array_equal(res.view(np.uint32), ref.residual.view(np.uint32)), what
    assert q.fields() == ref.record, (what, q.fields(), ref.record)


@pytest.mark.parametrize("name,size", CRAFTED, ids=[f"{n}-{Q.sid(s)}" for n, s in CRAFTED])
def test_crafted_parity(name, size):
    case, dist, deg = K.crafted(name, *size)
    kf = ctx(case.I, dist, deg)
    load(kf, case)
    kf.stage_icp_accumulate(0, Pose.identity())
    sums = kf.debug_get_icp_sums()
    for moved in (False, True):
        ref = Q.crafted_ref(name, *size, moved)
        pose = K.moved_pose() if moved else Pose.identity()
        same(kf.stage_icp_residuals(0, pose), ref, moved)                      # the instantiation with stores
        assert kf.stage_icp_residuals(0, pose, maps=False).fields() == ref.record  # stats only
        assert kfx.quality_figures(kf.score_poses(0, [pose])[0]) == Q.figures_np(ref.n, ref.sum_r2)
    assert np.array_equal(kf.debug_get_icp_sums(), sums)  # DevState untouched
    assert kf.quality_ms()["residuals"] > 0.0 and kf.quality_ms()["view"] == 0.0


@pytest.mark.parametrize("n", [1, 3, 130])
@pytest.mark.parametrize("size", [(80, 48), (320, 240)], ids=Q.sid)
def test_batch(size, n):
    case, dist, deg = K.crafted("b_projection", *size)
    kf = ctx(case.I, dist, deg)
    load(kf, case)
    poses = Q.pose_family(n)
    chunk = kfx.quality_chunk(*size, n)
    assert chunk == Q.chunk_np(*size, n)
    if n == 130:  # several chunks; at 320x240 (16 to a block) the last is short, at 80x48 the rule gives 1
        assert -(-n // chunk) >= 9 and chunk == {(80, 48): 1, (320, 240): 16}[size]
        assert size == (80, 48) or n % chunk == 2
    out = kf.score_poses(0, poses)
    single = [kf.stage_icp_residuals(0, p, maps=False) for p in poses]
    assert [q.fields() for q in out] == [q.fields() for q in single]
    assert out[0].fields() == Q.crafted_ref("b_projection", *size, False).record
    if n >= 2:
        assert out[1].fields() == Q.crafted_ref("b_projection", *size, True).record
    if n == 130:  # the family repeats with period 40 from its third pose on
        assert len({q.fields() for q in out}) > 20
        for k in range(2, n - 40):
            assert out[k].fields() == out[k + 40].fields()


def test_batch_edges():
    case, dist, deg = K.crafted("b_projection", 80, 48)
    kf = ctx(case.I, dist, deg)
    load(kf, case)
    L = kfx.lib()
    poses = (Pose * 4)(*[Pose.from_matrix(m) for m in Q.pose_family(4)])
    out = (IcpQuality * 4)()
    C.memset(out, 0xAB, C.sizeof(out))
    before = bytes(out)
    assert L.kfx_score_poses(kf._h, 0, poses, 0, out) == KFX_OK and bytes(out) == before  # n = 0: a no-op
    assert L.kfx_score_poses(kf._h, 0, None, 0, None) == KFX_OK
    assert L.kfx_score_poses(kf._h, 0, poses, (1 << 16) + 1, out) == -1 and bytes(out) == before
    assert L.kfx_score_poses(kf._h, 0, poses, -1, out) == -1
    for idx, val in ((0, float("nan")), (4, float("inf")), (11, float("nan"))):
        bad = (Pose * 4)(*[Pose.from_matrix(m) for m in Q.pose_family(4)])
        if idx < 9:
            bad[3].R[idx] = val
        else:
            bad[3].t[idx - 9] = val
        assert L.kfx_score_poses(kf._h, 0, bad, 4, out) == -1 and bytes(out) == before
    assert L.kfx_score_poses(kf._h, 0, poses, 4, out) == KFX_OK and bytes(out) != before


# ---- the frame's own maps ---------------------------------------------------

def thresholds(p):
    return p.icp_dist_threshold, K.sinf_deg(p.icp_angle_threshold)


@functools.lru_cache(maxsize=None)
def frame_refs():
    """Per frame and level: quality_np of the oracle pipeline's CUR against PREV maps under the identity."""
    intr, bgr, dep = VC.scene()
    I, p = Intrinsics.from_any(intr), VC.params(64)
    pipe = O.Pipeline(I, p)
    out = []
    for k in range(VC.N_FRAMES):
        assert pipe.process(bgr[k], dep[k]) == 0
        out.append([Q.quality_np(pipe.map(0, 1, l), pipe.map(0, 2, l), pipe.map(1, 1, l), pipe.map(1, 2, l), I.level(l),
                                 Pose.identity(), *thresholds(p), level=l) for l in range(p.pyramid_height)])
    return out


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("graph", [0, 1])
def test_frame_quality(graph, overlap, staged):
    intr, bgr, dep = VC.scene()
    refs = frame_refs()
    assert refs[-1][0].n[0] > 10000 and refs[-1][0].sum_r2 > 0 and refs[0][0].sum_r2 == 0  # bootstrap: PREV = CUR
    kf = KinectFusion(Intrinsics.from_any(intr), VC.params(64))
    kf.set_graph_mode(graph)
    kf.set_frame_overlap(overlap)
    if staged:
        kf.stage_frames(bgr, dep)
        for k in range(VC.N_FRAMES):
            kf.pipeline_staged(k)
        assert kf.synchronize() == KFX_OK
        frames = [VC.N_FRAMES - 1]
    else:
        frames = range(VC.N_FRAMES)
    for k in frames:
        if not staged:
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        for l in range(kf.params.pyramid_height):
            same(kf.frame_quality(l, maps=True), refs[k][l], (k, l))
            assert kf.frame_quality(l).fields() == refs[k][l].record
    kf.close()


# ---- at a world pose --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def world(dims):
    """The oracle pipeline over the scene: tsdf, poses and the last frame's CUR maps per level."""
    intr, bgr, dep = VC.scene()
    I, p = Intrinsics.from_any(intr), VC.params(dims)
    pipe = O.Pipeline(I, p)
    for k in range(VC.N_FRAMES):
        assert pipe.process(bgr[k], dep[k]) == 0
    cur = [(pipe.map(0, 1, l), pipe.map(0, 2, l)) for l in range(p.pyramid_height)]
    return pipe.volume()[0], pipe.poses(), cur, I, p


def world_pose(dims, which):
    last = world(dims)[1][-1]
    if which == "tracked":
        return last.astype(np.float32)
    if which == "1cm":
        m = last.astype(np.float32).copy()
        m[0, 3] += np.float32(0.01)
        return m
    return dict((n, pose) for n, _, pose in VC.views(last))["miss"]  # view_cases' turned-away camera


@functools.lru_cache(maxsize=None)
def view_ref(dims, which, level):
    tsdf, _, cur, I, p = world(dims)
    vol = O.Volume((dims,) * 3, (VC.RANGE_M,) * 3)
    c2v, Rinv = VC.cam2vol(p, world_pose(dims, which))
    li = I.level(level)
    _, v, n, _ = O.raycast_slab(tsdf, vol, li, c2v, Rinv, 0, dims, 0, dims)
    return Q.quality_np(cur[level][0], cur[level][1], v, n, li, Pose.identity(), *thresholds(p), level=level)


_fused = {}


def get_fused(dims, slab=False):
    """A context that ran the scene (shared, read-only use: the calls under test change no state)."""
    if (dims, slab) not in _fused:
        intr, bgr, dep = VC.scene()
        kf = KinectFusion(Intrinsics.from_any(intr), VC.params(dims), **(dict(slab=(0, 1)) if slab else {}))
        for k in range(VC.N_FRAMES):
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        assert np.array_equal(kf.pose_record, world(dims)[1])
        _fused[(dims, slab)] = kf
    return _fused[(dims, slab)]


@pytest.mark.parametrize("which", ["tracked", "1cm", "away"])
@pytest.mark.parametrize("dims", VC.DIMS)
def test_score_view(dims, which):
    kf = get_fused(dims)
    for l in range(3):
        ref = view_ref(dims, which, l)
        same(kf.score_view(l, world_pose(dims, which), maps=True), ref, (which, l))
        assert kf.score_view(l, world_pose(dims, which)).fields() == ref.record
        ms = kf.quality_ms()
        assert ms["residuals"] > 0.0 and ms["view"] > 0.0
    ref = view_ref(dims, which, 0)  # conditions on the reference alone
    if which == "tracked":
        assert ref.n[0] >= 10000 and all(ref.n[k] > 0 for k in range(5)), ref.n
        print(dims, ref.n, Q.figures_np(ref.n, ref.sum_r2))
    if which == "away":
        assert ref.n[0] == 0


@pytest.mark.parametrize("dims", VC.DIMS)
def test_score_view_uses_render_view_maps(dims):
    kf = get_fused(dims)
    pose = world_pose(dims, "tracked")
    _, v, n, _ = kf.render_view(kf.intr, pose, "normal", maps=True)
    _, cv, cn = kf.frame_maps(KFX_FRAME_CUR, 0)
    assert n.any()
    ref = Q.quality_np(cv, cn, v, n, kf.intr, Pose.identity(), *thresholds(kf.params))
    same(kf.score_view(0, pose, maps=True), ref)
    assert ref.record == view_ref(dims, "tracked", 0).record


# ---- tracking is left alone -------------------------------------------------

def _state(kf):
    maps = [kf.frame_maps(KFX_FRAME_PREV, l)[1:] for l in range(kf.params.pyramid_height)]
    return kf.pose_record, maps, kf.volume_soa()


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("graph", [0, 1])
def test_no_interference(graph, overlap, staged):
    intr, bgr, dep = VC.scene()
    states = []
    for with_calls in (True, False):
        kf = KinectFusion(Intrinsics.from_any(intr), VC.params(64))
        kf.set_graph_mode(graph)
        kf.set_frame_overlap(overlap)
        if staged:
            kf.stage_frames(bgr, dep)
            assert kf.synchronize() == KFX_OK
        for k in range(len(dep)):
            if staged:
                kf.pipeline_staged(k)  # no explicit sync before the calls
            else:
                assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
            if with_calls:
                q = kf.stage_icp_residuals(k % 3, K.moved_pose())[0]
                assert sum(q.n) == (320 >> k % 3) * (240 >> k % 3)
                assert len(kf.score_poses(2, Q.pose_family(20))) == 20
                assert kf.frame_quality(0, maps=True)[0].n[0] > 4000  # (the oracle's frames accept 4331 .. 67951)
                kf.score_view(1, np.eye(4, dtype=np.float32), maps=True)
                assert kf.quality_ms()["view"] > 0.0
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


def test_pending_tracking_status_is_left():
    intr, bgr, dep = VC.scene()
    kf = KinectFusion(Intrinsics.from_any(intr), VC.params(64))
    kf.pipeline_async(bgr[0], dep[0])
    kf.pipeline_async(bgr[1], dep[1])
    kf.pipeline_async(bgr[2], np.zeros_like(dep[2]))  # no depth: the ICP's determinant check fails, the frame is dropped
    q = kf.frame_quality(0)
    assert q.n[0] == 0 and sum(q.n) == 320 * 240  # the dropped frame's maps hold no surface
    assert kf.score_view(0, np.eye(4, dtype=np.float32)).n[0] == 0
    assert kf.synchronize() == KFX_TRACKING_LOST
    assert kf.synchronize() == KFX_OK
    kf.close()


# ---- arguments and state ----------------------------------------------------

def test_argument_and_state_errors():
    kf = get_fused(64)
    L = kfx.lib()
    h, w = 240, 320
    res, lab, q = np.zeros((h, w), np.float32), np.zeros((h, w), np.uint8), IcpQuality()
    rp, lp, qp = res.ctypes.data_as(C.POINTER(C.c_float)), lab.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(q)
    good = Pose.from_matrix(kf.pose_record[-1])
    ident = Pose.identity()
    for level in (-1, 3, 4):
        assert L.kfx_stage_icp_residuals(kf._h, level, C.byref(ident), rp, lp, qp) == -1
        assert L.kfx_frame_quality(kf._h, level, rp, lp, qp) == -1
        assert L.kfx_score_view(kf._h, level, C.byref(good), rp, lp, qp) == -1
        assert L.kfx_score_poses(kf._h, level, C.byref(ident), 1, qp) == -1
    assert L.kfx_stage_icp_residuals(kf._h, 0, None, rp, lp, qp) == -1
    assert L.kfx_score_view(kf._h, 0, None, rp, lp, qp) == -1
    assert L.kfx_score_poses(kf._h, 0, None, 1, qp) == -1 and L.kfx_score_poses(kf._h, 0, C.byref(ident), 1, None) == -1
    assert L.kfx_stage_icp_residuals(kf._h, 0, C.byref(ident), None, None, None) == -1
    assert L.kfx_frame_quality(kf._h, 0, None, None, None) == -1
    assert L.kfx_score_view(kf._h, 0, C.byref(good), None, None, None) == -1
    assert L.kfx_get_quality_ms(kf._h, None) == -1
    for idx in (0, 4, 8, 9, 11):
        for val in (float("nan"), float("inf")):
            bad = Pose.from_matrix(kf.pose_record[-1])
            if idx < 9:
                bad.R[idx] = val
            else:
                bad.t[idx - 9] = val
            assert L.kfx_score_view(kf._h, 0, C.byref(bad), rp, lp, qp) == -1
    # each output alone
    ref = view_ref(64, "tracked", 0)
    assert L.kfx_score_view(kf._h, 0, C.byref(good), rp, None, None) == KFX_OK
    assert L.kfx_score_view(kf._h, 0, C.byref(good), None, lp, None) == KFX_OK
    assert L.kfx_score_view(kf._h, 0, C.byref(good), None, None, qp) == KFX_OK
    same((q, res, lab), ref)
    # one slab of several: the maps are replicated, the volume is not
    sl = KinectFusion(kf.intr, VC.params(64), slab=(0, 2))
    assert L.kfx_frame_quality(sl._h, 0, rp, lp, qp) == KFX_OK
    assert L.kfx_stage_icp_residuals(sl._h, 1, C.byref(ident), None, None, qp) == KFX_OK
    assert L.kfx_score_poses(sl._h, 2, C.byref(ident), 1, qp) == KFX_OK and sum(q.n) == 80 * 60
    assert L.kfx_score_view(sl._h, 0, C.byref(good), rp, lp, qp) == -4
    sl.close()


def test_slab_of_world_one():
    kf, one = get_fused(64), get_fused(64, slab=True)
    pose = world_pose(64, "tracked")
    for l in range(3):
        same(one.frame_quality(l, maps=True), frame_refs()[-1][l], l)
        same(one.score_view(l, pose, maps=True), view_ref(64, "tracked", l), l)
        assert one.stage_icp_residuals(l, K.moved_pose(), maps=False).fields() == \
            kf.stage_icp_residuals(l, K.moved_pose(), maps=False).fields()


def test_runner_writes_quality_log(tmp_path):
    import subprocess
    from test_gpu_dataset import RUNNER, _write
    intr = synth.Intrinsics.qvga()
    bgr, dep, _ = synth.sequence(4, intr, noise=True, dropout=0.01)
    root = str(tmp_path / "ds")
    _write(root, bgr, dep, intr)
    ds = kfx.Dataset(root)
    kf = KinectFusion(ds.intrinsics, default_params())  # the runner's parameters
    want = []
    for k in range(len(ds)):
        c, d = ds.read(k)
        st = kf.pipeline(c, d)
        q = kf.frame_quality(0)
        want.append("%d %d %d %d %d %d %d %d %.9g %.9g" % ((k, st) + tuple(q.n[:]) + kfx.quality_figures(q)))
    kf.close()
    ds.close()
    log = tmp_path / "quality.txt"
    args = [RUNNER, root, str(tmp_path / "poses.txt")] + [""] * 10 + [str(log)]  # the thirteenth argument
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = open(log).read().splitlines()
    assert got == want and len(got) == 4 and int(got[-1].split()[2]) > 10000
    r = subprocess.run(args[:3], capture_output=True, text=True, timeout=120)  # without it: as before
    assert r.returncode == 0 and "end!" in r.stdout
