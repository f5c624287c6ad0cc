"""Multi-start ICP, tracking against a view and resuming at a pose on the GPU
(DESIGN.md §27).  Every comparison is exact: poses and x as bits, status, stop
point and solves as integers, quality records field by field.  The reference is
multi_cases.loop_from (the oracle's accumulate and update chained from a start
pose); tests/test_multi_cases.py holds it to the oracle's own loop and asserts
what the start family has to contain."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import kfx
import multi_cases as M
import oracle as O
import solve_cases as S
import view_cases as VC
from kfx import KFX_FRAME_CUR, KFX_FRAME_PREV, KFX_OK, KFX_TRACKING_LOST, KinectFusion, synth
from kfx.abi import IcpQuality, IcpResult, Intrinsics, Pose, default_params

pytestmark = pytest.mark.gpu
f32 = np.float32
LOOPS = ["iters_203", "iters_000", "chain", "fail_middle", "fail_second_iteration"]
_ctx = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for kf in _ctx.values():
        kf.close()
    _ctx.clear()


def fields(results):
    return [r.fields() for r in results]


def load(kf, levels):
    for l, L in enumerate(levels):
        kf.set_frame_maps(KFX_FRAME_CUR, l, L.cur_v, L.cur_n)
        kf.set_frame_maps(KFX_FRAME_PREV, l, L.pre_v, L.pre_n)


def params_for(levels, iters, dist, deg):
    p = default_params(dims=64, range_m=2.048)
    p.pyramid_height, p.icp_dist_threshold, p.icp_angle_threshold = len(levels), dist, deg
    for k in range(4):
        p.icp_iter_count[k] = iters[k] if k < len(iters) else 0
    return p


# ---- 1. crafted loops ---------------------------------------------------------

@pytest.mark.parametrize("name", LOOPS)
def test_crafted_loops(name):
    """solve_cases' loop cases in a 128 x 128 context with the case's iteration counts (iters_203 has a level
    with none, iters_000 no iteration at all): one start equals kfx_stage_icp and loop_from, five equal loop_from."""
    c = S.case(name)
    kf = KinectFusion(c.levels[0].I, params_for(c.levels, c.iters, c.dist, c.deg))
    try:
        load(kf, c.levels)
        rc, gpose = kf.stage_icp()
        step = kf.debug_get_icp_step()
        ref = [M.loop_from(c.levels, c.iters, s, c.dist, c.deg) for s in M.starts(5)]
        assert max(r.theta_max for r in ref) < 0.5  # (a condition on the inputs: one sincos on both sides)
        one = kf.icp_multi([Pose.identity()])
        assert len(one) == 1 and one[0].fields() == ref[0].fields()
        assert one[0].status == rc and bytes(one[0].pose) == bytes(gpose)
        if one[0].solves and rc == KFX_OK:
            assert np.array_equal(np.array(one[0].x[:]).view(np.uint64), step.view(np.uint64))
        if c.__dict__.get("stop"):
            assert rc == KFX_TRACKING_LOST and (one[0].stop_level, one[0].stop_iter) == c.stop
        assert fields(kf.icp_multi(M.starts(5))) == fields(ref)
        assert np.array_equal(kf.debug_get_icp_step().view(np.uint64), step.view(np.uint64))
        ms = kf.icp_multi_ms()
        assert ms["view"] == 0.0 and ms["score"] == 0.0 and (ms["loop"] > 0.0 or sum(c.iters) == 0)
    finally:
        kf.close()


# ---- 2. batch shapes ----------------------------------------------------------

def qvga_ctx():
    if "qvga" not in _ctx:
        p = M.qvga_pairs()[2]
        kf = KinectFusion(M.qvga_levels()[0].I, p)
        load(kf, M.qvga_levels())
        _ctx["qvga"] = kf
    return _ctx["qvga"]


def small_ctx():
    if "small" not in _ctx:
        p = M.qvga_pairs()[2]
        L = M.small_levels()
        kf = KinectFusion(L[0].I, params_for(L, (4,), p.icp_dist_threshold, p.icp_angle_threshold))
        load(kf, L)
        _ctx["small"] = kf
    return _ctx["small"]


SHAPES = {"80x48": (small_ctx, M.small_refs, (80, 48)), "320x240": (qvga_ctx, M.qvga_refs, (320, 240))}


@pytest.mark.parametrize("n", [1, 3, 21, 130])
@pytest.mark.parametrize("size", list(SHAPES))
def test_batch(size, n):
    make, refs, wh = SHAPES[size]
    kf, ref = make(), refs(n)
    chunk = kfx.icp_multi_chunk(*wh, n)
    assert chunk == M.chunk_np(*wh, n)
    if n == 21:  # at QVGA two poses to a block, the last block's chunk short; at 80 x 48 the rule gives 1
        assert chunk == {"80x48": 1, "320x240": 2}[size] and (size == "80x48" or n % chunk == 1)
    if n == 130:
        assert chunk == {"80x48": 1, "320x240": 16}[size] and (size == "80x48" or n % chunk == 2)
    if n > M.FAR + 1:  # a lost pose between two that converge, in one chunk with the first of them where chunk > 1
        assert [ref[M.FAR + d].status for d in (-1, 0, 1)] == [0, 1, 0]
        assert size == "80x48" or (M.FAR - 1) // chunk == M.FAR // chunk
    st = M.starts(n)
    got = kf.icp_multi(st)
    assert fields(got) == fields(ref)
    assert fields(kf.icp_multi(st[::-1])) == fields(ref)[::-1]  # the batch order does not matter
    if n > 10:  # repeated starts
        assert got[0].fields() == got[8].fields() == got[10].fields() and got[1].fields() == got[6].fields()
    if n == 130:
        assert {r.status for r in got} == {0, 1} and len({(r.stop_level, r.stop_iter) for r in got}) >= 4


# ---- 3. edges -------------------------------------------------------------------

def test_edges_and_scoring():
    kf = qvga_ctx()
    L = kfx.lib()
    n = 21
    poses = (Pose * n)(*[Pose.from_matrix(m) for m in M.starts(n)])
    out = (IcpResult * n)()
    q = (IcpQuality * n)()
    C.memset(out, 0xAB, C.sizeof(out))
    C.memset(q, 0xCD, C.sizeof(q))
    before, qbefore = bytes(out), bytes(q)
    assert L.kfx_icp_multi(kf._h, poses, 0, out, q) == KFX_OK and bytes(out) == before and bytes(q) == qbefore
    assert L.kfx_icp_multi(kf._h, None, 0, None, None) == KFX_OK
    assert L.kfx_icp_multi(kf._h, poses, (1 << 16) + 1, out, q) == -1 and bytes(out) == before
    assert L.kfx_icp_multi(kf._h, poses, -1, out, q) == -1
    assert L.kfx_icp_multi(kf._h, None, n, out, q) == -1 and L.kfx_icp_multi(kf._h, poses, n, None, q) == -1
    view = Pose.identity()
    assert L.kfx_track_view(kf._h, None, poses, n, out, None, None) == -1
    assert L.kfx_track_view(kf._h, C.byref(view), None, n, out, None, None) == -1
    assert L.kfx_track_view(kf._h, C.byref(view), poses, n, None, None, None) == -1
    assert L.kfx_track_view(kf._h, C.byref(view), poses, (1 << 16) + 1, out, None, None) == -1
    assert L.kfx_track_view(kf._h, C.byref(view), poses, 0, out, None, None) == KFX_OK and bytes(out) == before
    assert L.kfx_resume_at(kf._h, None) == -1 and L.kfx_get_icp_multi_ms(kf._h, None) == -1
    for idx, val in ((0, float("nan")), (4, float("inf")), (11, float("nan"))):
        bad = (Pose * n)(*[Pose.from_matrix(m) for m in M.starts(n)])
        bv = Pose.identity()
        if idx < 9:
            bad[n - 1].R[idx] = val
            bv.R[idx] = val
        else:
            bad[n - 1].t[idx - 9] = val
            bv.t[idx - 9] = val
        assert L.kfx_icp_multi(kf._h, bad, n, out, q) == -1 and bytes(out) == before and bytes(q) == qbefore
        assert L.kfx_track_view(kf._h, C.byref(view), bad, n, out, None, q) == -1 and bytes(out) == before
        assert L.kfx_track_view(kf._h, C.byref(bv), poses, n, out, None, q) == -1 and bytes(out) == before
        assert L.kfx_resume_at(kf._h, C.byref(bv)) == -1
    assert bytes(q) == qbefore
    # with q: kfx_score_poses' level-0 records of the poses reached (a lost pose where it stopped)
    qms = kf.quality_ms()
    res, rec = kf.icp_multi(M.starts(n), quality=True)
    assert fields(res) == fields(M.qvga_refs(n)) and {r.status for r in res} == {0, 1}
    assert kf.quality_ms() == qms and kf.icp_multi_ms()["score"] > 0.0
    want = kf.score_poses(0, [r.pose for r in res])
    assert [a.fields() for a in rec] == [b.fields() for b in want]
    assert rec[0].n[0] > 10000 and rec[M.FAR].n[0] == 0 and all(sum(a.n) == 320 * 240 and a.level == 0 for a in rec)


# ---- 4. state -------------------------------------------------------------------

def _prev(kf):
    return [kf.frame_maps(KFX_FRAME_PREV, l)[1:] for l in range(kf.params.pyramid_height)]


def _same_maps(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for la, lb in zip(a, b) for x, y in zip(la, lb))


def test_calls_leave_state():
    intr, bgr, dep = VC.scene()
    kf = KinectFusion(Intrinsics.from_any(intr), VC.params(64))
    try:
        for k in range(VC.N_FRAMES):
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        kf.stage_icp()  # leaves its sums and step in DevState
        state = lambda: (kf.debug_get_icp_sums().tobytes(), kf.debug_get_icp_step().tobytes(), kf.pose_record.tobytes(),
                         kf.volume_checksum(), kf.frame_count)
        s0, m0 = state(), _prev(kf)
        res = kf.icp_multi(M.starts(21), quality=True)[0]
        assert {r.status for r in res} == {0, 1}
        res, world = kf.track_view(kf.pose_record[1], M.starts(12))
        assert res[0].status == 0 and res[M.FAR].status == 1
        assert state() == s0 and _same_maps(_prev(kf), m0)
    finally:
        kf.close()


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
                assert len(kf.icp_multi(M.starts(12))) == 12
                res, world = kf.track_view(np.eye(4, dtype=f32), M.starts(3))
                assert len(res) == 3 and kf.icp_multi_ms()["view"] > 0.0
        assert kf.synchronize() == KFX_OK
        states.append((kf.pose_record, _prev(kf), kf.volume_soa()))
        kf.close()
    (pa, ma, va), (pb, mb, vb) = states
    assert len(pa) == len(dep) and np.array_equal(pa, pb) and _same_maps(ma, mb)
    for a, b in zip(va, vb):
        assert np.array_equal(a, b)


def test_pending_tracking_status_is_left():
    intr, bgr, dep = VC.scene()
    kf = KinectFusion(Intrinsics.from_any(intr), VC.params(64))
    kf.pipeline_async(bgr[0], dep[0])
    kf.pipeline_async(bgr[1], dep[1])
    kf.pipeline_async(bgr[2], np.zeros_like(dep[2]))  # no depth: the determinant check fails, the frame is dropped
    res = kf.icp_multi(M.starts(3))
    assert [r.status for r in res] == [1, 1, 1]  # the dropped frame's maps hold no surface
    res, _ = kf.track_view(np.eye(4, dtype=f32), M.starts(3))
    assert [(r.status, r.stop_level, r.stop_iter) for r in res] == [(1, 2, 0)] * 3
    assert kf.synchronize() == KFX_TRACKING_LOST
    assert kf.synchronize() == KFX_OK
    kf.close()


# ---- 5. kfx_track_view ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def world(dims):
    """The oracle pipeline over the scene: tsdf, poses, the last frame's CUR maps per level, intrinsics, parameters."""
    intr, bgr, dep = VC.scene()
    I, p = Intrinsics.from_any(intr), VC.params(dims)
    pipe = O.Pipeline(I, p)
    for k in range(VC.N_FRAMES):
        assert pipe.process(bgr[k], dep[k]) == 0
    cur = [(pipe.map(0, 1, l), pipe.map(0, 2, l)) for l in range(p.pyramid_height)]
    return pipe.volume()[0], pipe.poses(), cur, I, p


def view_pose(dims, which):
    poses = world(dims)[1]
    if which == "frame2":
        return poses[1].astype(f32)
    return dict((n, pose) for n, _, pose in VC.views(poses[-1]))["miss"]  # view_cases' turned-away camera


def oracle_levels(dims, which):
    """CUR of the last frame against the oracle's raycast of the volume from the view, at each level's intrinsics."""
    tsdf, _, cur, I, p = world(dims)
    vol = O.Volume((dims,) * 3, (VC.RANGE_M,) * 3)
    c2v, Rinv = VC.cam2vol(p, view_pose(dims, which))
    out = []
    for l in range(p.pyramid_height):
        _, v, n, _ = O.raycast_slab(tsdf, vol, I.level(l), c2v, Rinv, 0, dims, 0, dims)
        out.append(M.level_of(cur[l][0], cur[l][1], v, n, I.level(l)))
    return out


def fused(dims):
    if ("fused", dims) not in _ctx:
        intr, bgr, dep = VC.scene()
        kf = KinectFusion(Intrinsics.from_any(intr), VC.params(dims))
        for k in range(VC.N_FRAMES):
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        assert np.array_equal(kf.pose_record, world(dims)[1])
        _ctx[("fused", dims)] = kf
    return _ctx[("fused", dims)]


@pytest.mark.parametrize("dims", VC.DIMS)
def test_track_view(dims):
    kf = fused(dims)
    _, poses, cur, I, p = world(dims)
    iters = tuple(p.icp_iter_count[:p.pyramid_height])
    view, st = view_pose(dims, "frame2"), M.starts(12)
    ref = [M.loop_from(oracle_levels(dims, "frame2"), iters, s, p.icp_dist_threshold, p.icp_angle_threshold) for s in st]
    assert max(r.theta_max for r in ref) < 0.5 and [r.status for r in ref] == [0] * M.FAR + [1, 0, 0]
    res, wl, rec = kf.track_view(view, st, quality=True)
    assert fields(res) == fields(ref)
    # the same from the library's own view maps, level by level
    own = []
    for l in range(p.pyramid_height):
        _, v, n, _ = kf.render_view(I.level(l), view, "normal", maps=True)
        assert n.any()
        own.append(M.level_of(cur[l][0], cur[l][1], v, n, I.level(l)))
    assert fields(res) == fields([M.loop_from(own, iters, s, p.icp_dist_threshold, p.icp_angle_threshold) for s in st])
    for k in range(len(st)):  # world = view * pose in float32, pose_mul's order
        want = M.pose_mul_f32(view, res[k].pose.matrix())
        assert np.array_equal(wl[k].matrix().view(np.uint32), want.view(np.uint32)), k
    ms = kf.icp_multi_ms()
    assert ms["view"] > 0.0 and ms["loop"] > 0.0 and ms["score"] > 0.0
    assert rec[0].n[0] > 4000 and rec[M.FAR].n[0] == 0  # (the oracle's frames accept 4331 .. 67951 at the identity)
    # sanity, not parity: from the identity start the recovered pose is nearer frame 4's than the view is
    got, tracked = wl[0].matrix()[:3, 3], poses[3][:3, 3].astype(f32)
    print(dims, "recovered", np.linalg.norm(got - tracked), "view", np.linalg.norm(view[:3, 3] - tracked))
    assert np.linalg.norm(got - tracked) < np.linalg.norm(view[:3, 3] - tracked)
    # a turned-away camera: nothing to match at the coarsest level
    away = view_pose(dims, "away")
    res, wl = kf.track_view(away, st)
    assert [(r.status, r.stop_level, r.stop_iter, r.solves) for r in res] == [(1, 2, 0, 0)] * len(st)
    assert fields(res) == fields([M.loop_from(oracle_levels(dims, "away"), iters, s, p.icp_dist_threshold,
                                              p.icp_angle_threshold) for s in st])
    assert np.array_equal(wl[3].matrix(), M.pose_mul_f32(away, st[3]))


# ---- 6. kfx_resume_at -----------------------------------------------------------

@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("graph", [0, 1])
def test_resume_on_a_restored_volume(graph, overlap):
    intr, bgr, dep = VC.scene()
    I, p = Intrinsics.from_any(intr), VC.params(64)
    a, b = KinectFusion(I, p), KinectFusion(I, p)
    try:
        for kf in (a, b):
            kf.set_graph_mode(graph)
            kf.set_frame_overlap(overlap)
        for k in range(3):
            assert a.pipeline(bgr[k], dep[k]) == KFX_OK
        b.upload_tsdf(a.download_tsdf())
        assert b.frame_count == 1 and len(b.pose_record) == 1
        b.resume_at(a.pose_record[-1])
        assert b.frame_count == 2 and len(b.pose_record) == 2
        assert np.array_equal(b.pose_record[-1].view(np.uint32), a.pose_record[-1].view(np.uint32))
        assert _same_maps(_prev(a), _prev(b)) and any(n.any() for _, n in _prev(b))
        assert a.volume_checksum() == b.volume_checksum()
        if overlap:  # the overlapped route: staged frames
            for kf in (a, b):
                kf.stage_frames(bgr[3:4], dep[3:4])
                kf.pipeline_staged(0)
                assert kf.synchronize() == KFX_OK
        else:
            assert a.pipeline(bgr[3], dep[3]) == KFX_OK and b.pipeline(bgr[3], dep[3]) == KFX_OK
        assert len(b.pose_record) == 3 and len(a.pose_record) == 4
        assert np.array_equal(b.pose_record[-1].view(np.uint32), a.pose_record[-1].view(np.uint32))
        assert not np.array_equal(a.pose_record[-1], a.pose_record[-2])
        assert _same_maps(_prev(a), _prev(b)) and a.volume_checksum() == b.volume_checksum()
        # on a context that is already tracking the count grows by one, and so does the record
        assert (a.frame_count, b.frame_count) == (5, 3)
        b.resume_at(a.pose_record[1])
        assert b.frame_count == 4 and len(b.pose_record) == 4
        assert np.array_equal(b.pose_record[-1], a.pose_record[1]) and a.volume_checksum() == b.volume_checksum()
    finally:
        a.close()
        b.close()


def test_resume_slabs_and_full_record():
    intr, bgr, dep = VC.scene()
    I, p = Intrinsics.from_any(intr), VC.params(64)
    L = kfx.lib()
    a, one, two = KinectFusion(I, p), KinectFusion(I, p, slab=(0, 1)), KinectFusion(I, p, slab=(0, 2))
    try:
        for k in range(3):
            assert a.pipeline(bgr[k], dep[k]) == KFX_OK
        one.upload_tsdf(a.download_tsdf())
        one.resume_at(a.pose_record[-1])  # world 1 is accepted: the same PREV maps
        assert _same_maps(_prev(a), _prev(one))
        pose = Pose.from_matrix(a.pose_record[-1])
        assert L.kfx_resume_at(two._h, C.byref(pose)) == -4
        st = (Pose * 1)(Pose.identity())
        out = (IcpResult * 1)()
        assert L.kfx_track_view(two._h, C.byref(pose), st, 1, out, None, None) == -4
        assert L.kfx_icp_multi(two._h, st, 1, out, None) == KFX_OK  # the maps are replicated
    finally:
        for kf in (a, one, two):
            kf.close()
    # a full record: the smallest context, one append per call up to the log's 65536 entries
    tiny = default_params(dims=8, range_m=0.256)
    tiny.pyramid_height = 1
    kf = KinectFusion(Intrinsics(32, 32, 30.0, 30.0, 15.5, 15.5), tiny)
    try:
        ident = Pose.identity()
        t0 = time.time()
        for _ in range(65535):
            rc = L.kfx_resume_at(kf._h, C.byref(ident))
            if rc != KFX_OK:
                break
        print("65535 kfx_resume_at calls: %.2f s" % (time.time() - t0))
        n = C.c_int()
        assert rc == KFX_OK and L.kfx_get_pose_record(kf._h, None, 0, C.byref(n)) == KFX_OK and n.value == 65536
        assert L.kfx_resume_at(kf._h, C.byref(ident)) == -4 and b"full" in L.kfx_last_error()
        assert L.kfx_get_pose_record(kf._h, None, 0, C.byref(n)) == KFX_OK and n.value == 65536
    finally:
        kf.close()


# ---- 7. the runner ----------------------------------------------------------------

def test_runner_logs_track_view(tmp_path):
    import subprocess
    from test_gpu_dataset import RUNNER, _write
    intr = synth.Intrinsics.qvga()
    bgr, dep, _ = synth.sequence(5, intr, noise=True, dropout=0.01)
    root = str(tmp_path / "ds")
    _write(root, bgr, dep, intr)
    ds = kfx.Dataset(root)
    kf = KinectFusion(ds.intrinsics, default_params())  # the runner's parameters
    want = {}
    for k in range(len(ds)):
        c, d = ds.read(k)
        assert kf.pipeline(c, d) == KFX_OK
        if k > 0 and k % 2 == 0:
            rec = kf.pose_record
            res, wl, q = kf.track_view(rec[-3], [Pose.identity()], quality=True)
            want[k] = (res[0].status, np.linalg.norm(wl[0].matrix()[:3, 3].astype(np.float64) - rec[-1][:3, 3]),
                       "%.9g %.9g" % kfx.quality_figures(q[0]))
    kf.close()
    ds.close()
    args = [RUNNER, root, str(tmp_path / "poses.txt")] + [""] * 11 + ["2"]  # the fourteenth argument
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("track_view ")]
    assert [int(ln[1]) for ln in lines] == [2, 4] == sorted(want)  # one line per second frame
    for ln in lines:
        status, dist, figures = want[int(ln[1])]
        assert int(ln[2]) == status == KFX_OK and abs(float(ln[3]) - dist) <= 1e-6 * max(dist, 1e-3)
        assert " ".join(ln[5:7]) == figures and 0.0 <= float(ln[4]) < 0.05 and float(ln[3]) < 0.05
    r = subprocess.run(args[:3], capture_output=True, text=True, timeout=120)  # without it: as before
    assert r.returncode == 0 and "end!" in r.stdout and "track_view" not in r.stdout
