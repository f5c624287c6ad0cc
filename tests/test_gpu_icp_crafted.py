"""The ICP's 27 int64 sums on the crafted cases of tests/icp_cases.py, through
every reduction path, each against the oracle and each exactly: the
one-launch-per-iteration kernel (kfx_stage_icp_accumulate), the persistent
kernel in its plain, cooperative, contiguous-span and group-strided forms
(kfx_stage_icp, read back with kfx_debug_get_icp_sums, the forms selected with
kfx_debug_cap_icp_blocks), and systems the solve must refuse.  The oracle
equals the numpy restatement on the same cases (test_icp_restatement.py).
Every test asserts the kernel form it names from the plan the library reports."""
import numpy as np
import pytest

import icp_cases as K
import oracle as O
from kfx import KFX_FRAME_CUR, KFX_FRAME_PREV, KFX_OK, KinectFusion
from kfx.abi import Pose, default_params

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (80, 48), (96, 32), (320, 240), (512, 288), (640, 480)]
PPL = {(32, 32): 1, (80, 48): 1, (96, 32): 1, (320, 240): 2, (512, 288): 3, (640, 480): 4}
MODES = {"launches": 0, "persistent": 1, "cooperative": 2}
sid = lambda s: f"{s[0]}x{s[1]}"

_ctx = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for kf, _ in _ctx.values():
        kf.close()
    _ctx.clear()


def ctx(I, dist, deg, iters=(1, 0, 0, 0), levels=1, dfilter=5.0):
    key = (I.width, I.height, I.fx, I.cx, I.cy, float(dist), deg, iters, levels, dfilter)
    if key not in _ctx:
        p = default_params(dims=64, range_m=2.048)
        p.pyramid_height, p.dfilter_dist = levels, dfilter
        p.icp_dist_threshold, p.icp_angle_threshold = dist, deg
        for k in range(4):
            p.icp_iter_count[k] = iters[k]
        _ctx[key] = (KinectFusion(I, p), p)
    return _ctx[key]


def load(kf, cases):
    for l, c in enumerate(cases):
        kf.set_frame_maps(KFX_FRAME_CUR, l, c.cur_v, c.cur_n)
        kf.set_frame_maps(KFX_FRAME_PREV, l, c.pre_v, c.pre_n)


def replay(cases, I, p):
    """kfo_icp_accumulate / kfo_icp_update up to the last iteration that runs:
    (status, pose, that iteration's sums)."""
    pose, last = Pose.identity(), None
    ang = float(K.sinf_deg(p.icp_angle_threshold))
    for l in reversed(range(p.pyramid_height)):
        c = cases[l]
        for _ in range(p.icp_iter_count[l]):
            last = O.icp_accumulate(c.cur_v, c.cur_n, c.pre_v, c.pre_n, I.level(l), pose, p.icp_dist_threshold, ang)
            st, pose, _ = O.icp_update(last, pose)
            if st:
                return 1, pose, last
    return 0, pose, last


def check_track(kf, p, cases, I, launch):
    """kfx_stage_icp against the replay: status, pose, the last iteration's
    sums; and the launch that ran is the one asked for (no quiet fallback)."""
    load(kf, cases)
    rc, gpose = kf.stage_icp()
    st, opose, osums = replay(cases, I, p)
    gsums = kf.debug_get_icp_sums()
    assert np.array_equal(gsums, osums), (gsums - osums).tolist()
    assert (rc == KFX_OK) == (st == 0), (rc, st)
    assert np.array_equal(gpose.matrix(), opose.matrix())
    assert kf.debug_icp_plan()["launch"] == launch


def set_plan(kf, cap, mode):
    plan = kf.debug_cap_icp_blocks(cap)
    assert kf.set_icp_persistent(mode) == plan["usable"]
    return plan


@pytest.mark.parametrize("size", SIZES, ids=sid)
@pytest.mark.parametrize("name", list(K.case_table()))
def test_accumulate_launch(name, size):
    """k_icp_acc (kfx_stage_icp_accumulate runs nothing else), identity and a moved pose."""
    case, dist, deg = K.crafted(name, *size)
    kf, p = ctx(case.I, dist, deg)
    load(kf, [case])
    for pose in (Pose.identity(), K.moved_pose()):
        g = kf.stage_icp_accumulate(0, pose)
        o = O.icp_accumulate(case.cur_v, case.cur_n, case.pre_v, case.pre_n, case.I, pose, p.icp_dist_threshold,
                             float(K.sinf_deg(deg)))
        assert np.array_equal(g, o), (g - o).tolist()
        assert np.array_equal(kf.debug_get_icp_sums(), o)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("iters", [(1, 0, 0, 0), (2, 0, 0, 0)], ids=["it1", "it2"])
@pytest.mark.parametrize("size", SIZES, ids=sid)
@pytest.mark.parametrize("name", K.DEFAULT_THRESHOLD_CASES)
def test_track_sums(name, size, iters, mode):
    """kfx_stage_icp: per-iteration launches, k_icp_track<false> plain and cooperative."""
    case, dist, deg = K.crafted(name, *size)
    kf, p = ctx(case.I, dist, deg, iters)
    plan = set_plan(kf, 0, MODES[mode])
    assert plan["usable"] and plan["stride"] == 0 and plan["span"] == [0] and plan["ppl"] == [PPL[size]]
    check_track(kf, p, [case], case.I, MODES[mode])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(K.case_table()))
def test_track_sums_three_levels_320x240(name, mode):
    I = K.crafted_intrinsics(320, 240)
    cases = [K.crafted(name, 320 >> l, 240 >> l)[0] for l in range(3)]
    for l, c in enumerate(cases):
        li = I.level(l)
        assert (c.I.fx, c.I.fy, c.I.cx, c.I.cy) == (li.fx, li.fy, li.cx, li.cy)
    _, dist, deg = K.crafted(name, 320, 240)
    kf, p = ctx(I, dist, deg, (2, 1, 1, 0), levels=3)
    plan = set_plan(kf, 0, MODES[mode])
    assert plan["usable"] and plan["stride"] == 0 and plan["ppl"] == [2, 1, 1]
    check_track(kf, p, cases, I, MODES[mode])


# 256x128: 32768 pixels, 128 pixel groups of 256.  The plan under a cap, from
# icp_persistent_ok: span = ceil(ceil(npix / cap) / 256) * 256 while one block
# may sum that many pixels exactly (46 398 at dfilter_dist 5, 1 680 at 30 with
# these intrinsics), else groups b, b + cap, ... ; with more than 16 groups per
# block (cap < 8 here) the plan is refused: one launch per iteration.
CAPS = {
    "span2048": (5.0, 16, dict(usable=True, stride=1, nblocks=16, span=[2048], groups=[16])),
    "span4096": (5.0, 8, dict(usable=True, stride=1, nblocks=8, span=[4096], groups=[8])),
    "span1536_short_last": (5.0, 24, dict(usable=True, stride=1, nblocks=24, span=[1536], groups=[22])),
    "groups_strided_8each": (30.0, 16, dict(usable=True, stride=1, nblocks=16, span=[0], groups=[128])),
    "groups_strided_16each": (30.0, 8, dict(usable=True, stride=1, nblocks=8, span=[0], groups=[128])),
    "fallback": (5.0, 4, dict(usable=False, stride=0)),  # 128 groups over 4 blocks: more than kIcpStrideMax each
}


def check_capped(kf, p, case, form):
    _, cap, want = CAPS[form]
    plan = set_plan(kf, cap, 1)
    assert {k: plan[k] for k in want} == want, plan
    check_track(kf, p, [case], case.I, 1 if want["usable"] else 0)
    return plan


@pytest.mark.parametrize("form", list(CAPS))
@pytest.mark.parametrize("name", list(K.case_table()))
def test_track_sums_capped_256x128(name, form):
    """k_icp_track<true>: contiguous spans (the last block short in one), whole groups strided, and the fallback."""
    case, dist, deg = K.crafted(name, 256, 128)
    kf, p = ctx(case.I, dist, deg, (2, 0, 0, 0), dfilter=CAPS[form][0])
    check_capped(kf, p, case, form)
    kf.debug_cap_icp_blocks(0)


@pytest.mark.parametrize("form", ["plain", "launches", "groups_strided_8each", "groups_strided_16each"])
@pytest.mark.parametrize("zfar,slant", [(12.0, False), (30.0, False), (30.0, True)],
                         ids=["f_wall_12m", "f_wall_30m", "f_slant_30m"])
def test_magnitude_256x128(zfar, slant, form):
    """Class f on a context that admits 30 m: the forms the derived bound
    leaves (no span: 2048 pixels exceed the 1 344 one block may sum), whose
    blocks' sums stay below 2^53 although 8192-pixel blocks' would not.
    (With the former literal span limit of 8192 pixels, measured once: spans of
    2048 and 4096 pixels, the latter 2^53.93 on the 30 m wall, also matched.)"""
    case = K.gen_magnitude(zfar, slant)
    kf, p = ctx(case.I, 0.015, 30.0, (1, 0, 0, 0), dfilter=30.0)
    if form in CAPS:
        plan = check_capped(kf, p, case, form)
    else:
        plan = set_plan(kf, 0, MODES["persistent" if form == "plain" else form])
        assert plan["usable"] and plan["stride"] == 0 and plan["nblocks"] == 128
        check_track(kf, p, [case], case.I, 1 if form == "plain" else 0)
    r = K.accumulate_np(case.cur_v, case.cur_n, case.pre_v, case.pre_n, case.I, Pose.identity(), 0.015,
                        K.sinf_deg(30.0))
    assert max(K.block_sum_report(r.terms, dict(plan, level=0)).max_sum_abs) < 2 ** 53
    kf.debug_cap_icp_blocks(0)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", [(80, 48), (640, 480)], ids=sid)
@pytest.mark.parametrize("name", [n for n in K.case_table() if n not in K.DEFAULT_THRESHOLD_CASES])
def test_track_sums_other_thresholds(name, size, mode):
    """The thresholds reach k_icp_track through IcpPlan::dist2_max / sine2_max: the 4 mm, bound-above-square and 8 degree ladders."""
    case, dist, deg = K.crafted(name, *size)
    kf, p = ctx(case.I, dist, deg, (2, 0, 0, 0))
    plan = set_plan(kf, 0, MODES[mode])
    assert plan["usable"] and plan["stride"] == 0 and plan["ppl"] == [PPL[size]]
    check_track(kf, p, [case], case.I, MODES[mode])


@pytest.mark.parametrize("mode", ["launches", "persistent"])
@pytest.mark.parametrize("kind", ["none", "one", "three", "six", "one_plane", "two_planes", "three_planes"])
def test_degenerate_systems_64x64(kind, mode):
    I = K.crafted_intrinsics(64, 64)
    case = K.gen_degenerate(kind, I)
    kf, p = ctx(I, 0.015, 30.0, (2, 0, 0, 0))
    set_plan(kf, 0, MODES[mode])
    check_track(kf, p, [case], I, MODES[mode])
    st, _, _ = replay([case], I, p)
    if kind in ("none", "one", "three", "one_plane"):
        assert st == 1
    if kind == "three_planes":
        assert st == 0
    # the replay's status of the two systems the geometry does not decide (the exact figures are
    # tests/solve_cases.py's, from the integer sums in rational arithmetic):
    if kind == "six":  # exact rank 6 at both iterations, exact det 9.2e-3: healthy by twelve orders
        assert st == 0
    if kind == "two_planes":  # exact rank 5, exact det 0, det P 4.9e8: det P * det S rounds below 1e-15 here
        assert st == 1
