"""Integrate's per-frame tile kernel (k_int_tiles) against the
waves' own prologue.

With the tile kernel on, a block of two waves per column tile computes the
interval, the chunk cuts, vc at every chunk's start and the brick masks once, and the
integrate waves load them; with it off (kfx_debug_int_tiles(0)) every wave
computes them for itself, as before.  Each test runs the same input through
two contexts, one per path, and compares bit for bit: tsdf, weight and colour
of the whole volume, the settled-byte and skip counts (kfx_debug_get_settled,
kfx_debug_get_hidden), the poses and the PREV maps of every level.  The off
path is also held against the oracle, since the default has moved away from it.

64^3 volumes under the 160x120 / 320x240 cameras: 64 tiles, so 8 chunks per
tile and every chunk boundary is exercised.  No tolerance anywhere.
"""
import numpy as np
import pytest

import integrate_cases as IC
import oracle as O
from kfx import KFX_FRAME_PREV, KFX_OK, KFX_TRACKING_LOST, KinectFusion, synth
from kfx.abi import Intrinsics, default_params

pytestmark = pytest.mark.gpu

L_VOL = 2.048
N = 64


def feq(a, b):
    """Bit equality of float32 arrays with NaNs compared by position (test_gpu_parity.feq)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    z = np.float32(0)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, z, a).view(np.uint32),
                                                     np.where(nb, z, b).view(np.uint32))


def snapshot(kf, levels):
    """Everything the two paths must agree on, as the context stands."""
    t, w, c = kf.volume_soa()
    maps = [kf.frame_maps(KFX_FRAME_PREV, l)[1:] for l in range(levels)]
    return dict(t=t, w=w, c=c, settled=kf.debug_get_settled(), hidden=kf.debug_get_hidden(),
                poses=np.array(kf.pose_record), maps=maps)


def assert_snapshots_equal(a, b, what):
    for k in ("t", "w", "c"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k}, {(a[k] != b[k]).sum()} entries differ between the paths"
    assert a["settled"] == b["settled"], f"{what}: settled bytes / skipped bricks {a['settled']} against {b['settled']}"
    assert a["hidden"] == b["hidden"], f"{what}: hidden bricks {a['hidden']} against {b['hidden']}"
    assert a["poses"].shape == b["poses"].shape and np.array_equal(a["poses"], b["poses"]), f"{what}: poses"
    for l, ((av, an), (bv, bn)) in enumerate(zip(a["maps"], b["maps"])):
        assert feq(av, bv) and feq(an, bn), f"{what}: PREV maps level {l}"


def expect_tiles(dims):
    """Whether a whole-volume context of these dims keeps a tile table: more
    than one chunk per tile (24576 waves over the tiles, at most 8 chunks) and
    not the length-capped mode of 1024..2047 slices."""
    tiles = ((dims[0] + 7) // 8) * ((dims[1] + 7) // 8)
    return min(8, -(-24576 // tiles)) > 1 and not 1024 <= dims[2] < 2048


def both_paths(intr, params, run, what, index64=False, expect=True):
    """run(kf) -> list of snapshots, in a context per path; returns the off path's."""
    out = {}
    for on in (True, False):
        with KinectFusion(intr, params) as kf:
            assert kf.debug_int_tiles(on) == (on and expect), f"{what}: tile kernel in use"
            kf.debug_count_settled(True)
            if index64:
                kf.debug_force_index64(True)
            out[on] = run(kf)
    assert len(out[True]) == len(out[False]) > 0
    for k, (a, b) in enumerate(zip(out[True], out[False])):
        assert_snapshots_equal(a, b, f"{what} step {k}")
    return out[False]


# --------------------------------------------------------------------------
# the case table through the explicit-pose stage seam

def run_case(name, index64=False):
    case = IC.CASES[name]
    bgr, depth = IC.frame(case.frame)
    steps, vol = IC.oracle_zeroed(name)
    levels = case.params.pyramid_height

    def run(kf):
        snaps = []
        kf.stage_preprocess(bgr, depth)
        got = []
        for pose in case.poses:
            got.append(kf.stage_integrate(pose))
            snaps.append(snapshot(kf, 0))
        cam2vol = O.pose_inv(case.poses[-1])
        kf.stage_raycast(cam2vol, cam2vol.matrix()[:3, :3].T.copy())
        snaps.append(snapshot(kf, levels))
        snaps[-1]["counts"] = got
        return snaps

    off = both_paths(case.intr, case.params, run, name, index64=index64, expect=expect_tiles(case.dims))
    # the off path against the oracle
    for k, (snap, (cnt, t, w, c)) in enumerate(zip(off, steps)):
        assert off[-1]["counts"][k] == cnt, f"{name} launch {k}: counts"
        assert np.array_equal(snap["t"], t) and np.array_equal(snap["w"], w) and np.array_equal(snap["c"], c), \
            f"{name} launch {k}: the off path against the oracle"
    return off


@pytest.mark.parametrize("name", list(IC.CASES))
def test_case_table_both_paths(name):
    """Oblique and axis-swapping poses, empty intervals, columns on the IEEE
    path, odd depths, and the deep cases: deep2056 (8 geometric chunks of up to
    90 bricks: the first-64-bricks rule over several certificate rounds, chunk
    starts past KFX_FF_MIN) takes the table, deep1030 / deep1500 / deep_coarse
    (length-capped) keep the waves' prologue on both sides."""
    off = run_case(name)
    if name == "deep2056":
        assert all(s["hidden"][0] > 0 for s in off[:-1]), [s["hidden"] for s in off]


@pytest.mark.parametrize("name", ["oblique", "odd", "deep2056"])
def test_case_table_index64(name):
    run_case(name, index64=True)


# --------------------------------------------------------------------------
# whole frames: settled and hidden skips, reset, bootstrap, staged graphs

@pytest.fixture(scope="module")
def intr():
    return synth.Intrinsics.qvga()


def settled_volume(intr, depth_mm):
    """test_gpu_settled.settled_volume: free space at weight 64 and T*, the rest zero."""
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


def oracle_pipe(intr, frames, init=None):
    """The oracle's pipeline over (bgr, depth) frames, from an uploaded volume if given: (pipe, statuses)."""
    pipe = O.Pipeline(Intrinsics.from_any(intr), default_params(dims=N, range_m=L_VOL))
    if init is not None:
        n = N ** 3
        np.ctypeslib.as_array(O.lib().kfo_pipe_tsdf(pipe.h), shape=(n,))[:] = init[0]
        np.ctypeslib.as_array(O.lib().kfo_pipe_weight(pipe.h), shape=(n,))[:] = init[1]
        np.ctypeslib.as_array(O.lib().kfo_pipe_rgb(pipe.h), shape=(4 * n,))[:] = init[2]
    return pipe, [pipe.process(b, d) for b, d in frames]


def assert_oracle(snap, pipe, what):
    op = pipe.poses()
    assert snap["poses"].shape == op.shape and np.abs(snap["poses"] - op).max() == 0, f"{what}: poses against the oracle"
    for l, (gv, gn) in enumerate(snap["maps"]):
        assert feq(gv, pipe.map(1, 1, l)) and feq(gn, pipe.map(1, 2, l)), f"{what}: PREV maps level {l} against the oracle"
    ot, ow, oc = pipe.volume()
    assert np.array_equal(snap["t"], ot) and np.array_equal(snap["w"], ow) and np.array_equal(snap["c"], oc), \
        f"{what}: volume against the oracle"


@pytest.fixture(scope="module")
def moving(intr):
    """The moving trajectory of test_gpu_settled.py, the settled volume it starts from and the oracle's result."""
    bgr, dep, _ = synth.sequence(10, intr, noise=True, dropout=0.005, traj_seed=7, amp_t=0.16, period=60.0)
    dep = dep.astype(np.float32)
    init = settled_volume(intr, dep[0])
    pipe, st = oracle_pipe(intr, list(zip(bgr, dep)), init)
    assert st == [KFX_OK] * 10
    return bgr, dep, init, pipe


def frames_run(frames, init, statuses=None):
    def run(kf):
        if init is not None:
            kf.upload_tsdf(IC.records(*init))
        snaps = []
        for k, (b, d) in enumerate(frames):
            st = kf.pipeline(b, d)
            assert statuses is None or st == statuses[k], (k, st)
            snaps.append(snapshot(kf, 3))
        return snaps
    return run


def test_settled_volume_static_scene(intr):
    """An uploaded settled volume under a static scene: bytes are set in frame
    1, free bricks are skipped from frame 2 on, hidden ones in every frame, in
    the same waves."""
    scene = synth.Scene.default(L_VOL)
    fr = [synth.render(scene, intr, np.eye(4), noise_seed=100 + k, dropout=0.002) for k in range(3)]
    fr = [(b, d.astype(np.float32)) for b, d in fr]
    init = settled_volume(intr, fr[0][1])
    pipe, st = oracle_pipe(intr, fr, init)
    off = both_paths(Intrinsics.from_any(intr), default_params(dims=N, range_m=L_VOL), frames_run(fr, init, st), "static scene")
    assert_oracle(off[-1], pipe, "static scene")
    print("static scene: (set, free skips), (hidden, overhanging) per frame:", [(s["settled"], s["hidden"]) for s in off])
    assert off[1]["settled"][1] > 0 and off[2]["settled"][1] > 0 and all(s["hidden"][0] > 0 for s in off)


def test_settled_volume_moving_trajectory(intr, moving):
    bgr, dep, init, pipe = moving
    off = both_paths(Intrinsics.from_any(intr), default_params(dims=N, range_m=L_VOL),
                     frames_run(list(zip(bgr, dep)), init), "moving trajectory")
    assert_oracle(off[-1], pipe, "moving trajectory")
    assert sum(s["settled"][1] for s in off) > 0 and sum(s["hidden"][0] for s in off) > 0


def test_moving_trajectory_index64(intr, moving):
    bgr, dep, init, pipe = moving
    off = both_paths(Intrinsics.from_any(intr), default_params(dims=N, range_m=L_VOL),
                     frames_run(list(zip(bgr[:4], dep[:4])), init), "moving trajectory, 64-bit indices", index64=True)
    assert len(off) == 4


def test_bootstrap_reset_and_tracked_frames(intr, moving):
    """The bootstrap frame, tracked frames, a tracking failure (the reset
    frame: the table carries only the frame kind) and the frames after it."""
    bgr, dep, _, _ = moving
    fr = list(zip(bgr[:3], dep[:3])) + [(bgr[3], np.zeros_like(dep[3]))] + list(zip(bgr[4:7], dep[4:7]))
    pipe, st = oracle_pipe(intr, fr)
    assert st[3] == KFX_TRACKING_LOST and st[:3] == [KFX_OK] * 3 and st[4:] == [KFX_OK] * 3, st
    off = both_paths(Intrinsics.from_any(intr), default_params(dims=N, range_m=L_VOL), frames_run(fr, None, st),
                     "bootstrap, reset, tracked")
    assert (off[3]["w"] == 0).all() and (off[-1]["w"] > 0).any()
    assert_oracle(off[-1], pipe, "bootstrap, reset, tracked")


@pytest.mark.parametrize("gmode", [0, 1, 2])
def test_staged_overlapped_frames(intr, moving, gmode):
    """Overlapped staged frames, the tile kernel captured with the frame in graph modes 1 and 2."""
    bgr, dep, init, pipe = moving

    def run(kf):
        kf.upload_tsdf(IC.records(*init))
        kf.set_graph_mode(gmode)
        kf.set_frame_overlap(True)
        kf.stage_frames(bgr, dep)
        for k in range(10):
            kf.pipeline_staged(k)
        assert kf.synchronize() == KFX_OK
        return [snapshot(kf, 3)]

    off = both_paths(Intrinsics.from_any(intr), default_params(dims=N, range_m=L_VOL), run, f"staged frames, graph mode {gmode}")
    assert_oracle(off[0], pipe, f"staged frames, graph mode {gmode}")


# --------------------------------------------------------------------------
# the contexts that keep the waves' prologue

def test_slab_pair_and_capped_volume_keep_the_wave_prologue():
    """A Z-slab pair and a volume of 1024..2047 slices keep no tile table (the
    switch reports it) and still give the oracle's volume."""
    case = IC.CASES["slab300"]
    X, Y, Z = case.dims
    bgr, depth = IC.frame(case.frame)
    steps, _ = IC.oracle_zeroed("slab300")
    for r in range(2):
        with KinectFusion(case.intr, case.params, slab=(r, 2)) as kf:
            assert kf.debug_int_tiles(True) is False
            _, _, o0, o1 = kf.slab_info()
            kf.stage_preprocess(bgr, depth)
            for k, (pose, (_, t, w, c)) in enumerate(zip(case.poses, steps)):
                kf.stage_integrate(pose, counts=False)
                gt, gw, gc = kf.volume_soa()
                s, s4 = slice(o0 * X * Y, o1 * X * Y), slice(4 * o0 * X * Y, 4 * o1 * X * Y)
                assert np.array_equal(gt[s], t[s]) and np.array_equal(gw[s], w[s]) and np.array_equal(gc[s4], c[s4]), (r, k)
    case = IC.CASES["deep1030"]
    bgr, depth = IC.frame(case.frame)
    steps, _ = IC.oracle_zeroed("deep1030")
    with KinectFusion(case.intr, case.params) as kf:
        assert kf.debug_int_tiles(True) is False
        kf.stage_preprocess(bgr, depth)
        for k, (pose, (cnt, t, w, c)) in enumerate(zip(case.poses, steps)):
            assert kf.stage_integrate(pose) == cnt
            gt, gw, gc = kf.volume_soa()
            assert np.array_equal(gt, t) and np.array_equal(gw, w) and np.array_equal(gc, c), k
