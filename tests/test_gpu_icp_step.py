"""The ICP step on the device over the crafted systems of tests/solve_cases.py,
through every site that runs the solve: wave 0 of k_icp_acc's last block (one
launch per iteration), every wave of k_icp_track<false> (persistent, plain and
cooperative), k_icp_track<true> (the grid capped below a level's pixel groups)
and k_icp_solve (kfx_stage_icp's sharded route on a slab context of world 1).
Each run asserts the route from the plan the library reports, then against the
oracle's replay: the status, the 27 sums of the last iteration that ran, the
increment x[6] as doubles with == (kfx_debug_get_icp_step), the pose with ==
where every step has theta < 0.5, else the translation with == and R within one
float32 ulp per entry; and the device's R against the mpmath Rodrigues matrix
of its own float32 rotation vector, so a mistake the oracle shared would show.
A track that ends KFX_TRACKING_LOST is followed at once, on the same context,
by a healthy one.  tests/test_solve_cases.py holds the oracle to the exact
reference on the same table."""
import numpy as np
import pytest

import solve_cases as S
from kfx import KFX_FRAME_CUR, KFX_FRAME_PREV, KFX_OK, KFX_TRACKING_LOST, KinectFusion
from kfx.abi import default_params

pytestmark = pytest.mark.gpu
f32 = np.float32

ROUTES = ["launches", "persistent", "cooperative", "strided", "solve"]
LAUNCH = {"launches": 0, "persistent": 1, "cooperative": 2, "strided": 1, "solve": 3}
_ctx, _oracle = {}, {}
ocml_arm = {"runs": 0, "entries": 0, "differ": 0}  # R entries of steps with theta >= 0.5, and those that differ at all


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for kf in _ctx.values():
        kf.close()
    _ctx.clear()
    print("ocml arm: %(runs)d runs, %(differ)d of %(entries)d R entries differ from the oracle's" % ocml_arm)


def ctx(c, route):
    """One context per (parameters, kind): the three-level strided form needs
    dfilter_dist 30 (at 5 a block may sum a whole 2048-pixel share in one span);
    the solve route a slab context of world 1 with the partial all-reduce on."""
    levels = len(c.levels)
    dfilter = 30.0 if (route == "strided" and levels == 3) else 5.0
    key = (c.size, levels, c.dist, c.deg, c.iters, dfilter, route == "solve")
    if key not in _ctx:
        p = default_params(dims=64, range_m=2.048)
        p.pyramid_height, p.dfilter_dist = levels, dfilter
        p.icp_dist_threshold, p.icp_angle_threshold = c.dist, c.deg
        for k in range(4):
            p.icp_iter_count[k] = c.iters[k]
        kf = KinectFusion(c.levels[0].I, p, slab=(0, 1) if route == "solve" else None)
        if route == "solve":
            kf.set_icp_allreduce(True)
        _ctx[key] = kf
    return _ctx[key]


def set_route(kf, c, route):
    """Select the route and assert the plan the library reports for it."""
    if route == "solve":
        plan = kf.debug_icp_plan()
    elif route == "strided":
        three = len(c.levels) == 3
        plan = kf.debug_cap_icp_blocks(8 if three else 2)
        assert kf.set_icp_persistent(1) and plan["usable"] and plan["stride"] == 1, plan
        if three:  # level 0: 64 groups of 256 pixels over 8 blocks, whole groups strided
            assert plan["nblocks"] == 8 and plan["span"][0] == 0 and plan["groups"][0] > plan["nblocks"], plan
        else:      # 1024 pixels over 2 blocks: contiguous spans of 512
            assert plan["nblocks"] == 2 and plan["span"] == [512], plan
        plan = kf.debug_icp_plan()
    else:
        plan = kf.debug_cap_icp_blocks(0)
        assert plan["usable"] and plan["stride"] == 0, plan
        assert kf.set_icp_persistent(LAUNCH[route]) == plan["usable"]
        plan = kf.debug_icp_plan()
    assert plan["launch"] == LAUNCH[route], plan
    return plan


def oracle_of(c):
    if c.name not in _oracle:
        _oracle[c.name] = S.oracle_loop(c)
    return _oracle[c.name]


def ulp_apart(g, o):
    """|g - o| in float32 ulps at the larger magnitude, per entry."""
    g, o = np.asarray(g, f32), np.asarray(o, f32)
    return np.abs(g.astype(np.float64) - o.astype(np.float64)) / np.spacing(np.maximum(np.abs(g), np.abs(o))).astype(np.float64)


def track_and_check(kf, c, route):
    for l, L in enumerate(c.levels):
        kf.set_frame_maps(KFX_FRAME_CUR, l, L.cur_v, L.cur_n)
        kf.set_frame_maps(KFX_FRAME_PREV, l, L.pre_v, L.pre_n)
    rc, gpose = kf.stage_icp()
    assert kf.debug_icp_plan()["launch"] == LAUNCH[route]  # no quiet fallback
    its, status, opose = oracle_of(c)
    assert rc == (KFX_TRACKING_LOST if status else KFX_OK), (rc, status)
    if not its:  # no iteration ran: the identity, and nothing else is defined
        assert np.array_equal(gpose.matrix(), np.eye(4, dtype=f32))
        return rc
    gsums = kf.debug_get_icp_sums()
    assert np.array_equal(gsums, its[-1].sums), (gsums - its[-1].sums).tolist()
    solved = [r for r in its if r.status == 0]
    G, O = gpose.matrix(), opose.matrix()
    if rc == KFX_OK:
        last = solved[-1]
        gx = kf.debug_get_icp_step()
        assert np.array_equal(gx, last.x), (gx - last.x).tolist()  # the solve precedes sincos: == on both arms
        thetas = [float(S.theta_mp(np.array(r.x[:3], f32))) for r in solved]
        assert all(t < 0.5 for t in thetas[:-1])  # (the table puts a theta >= 0.5 step last only)
        if thetas[-1] < 0.5:
            assert np.array_equal(G, O), (G - O).tolist()
        else:
            assert np.array_equal(G[:3, 3], O[:3, 3])
            d = ulp_apart(G[:3, :3], O[:3, :3])
            ocml_arm["runs"] += 1
            ocml_arm["entries"] += 9
            ocml_arm["differ"] += int((d > 0).sum())
            print(f"ocml arm {c.name} {route}: theta {thetas[-1]:.9g}, {int((d > 0).sum())} of 9 entries differ, max {d.max():.3g} ulp")
            assert d.max() <= 1.0, d.tolist()
        # the device's R against mpmath's of the device's own float32 rv: 2 ulps of 1.0f per entry of the
        # increment; composed with the incoming rotation Ra that is 2 * sum_k |Ra_jk| ulps plus 1.5 for the three
        # products' and two sums' roundings of values at most 1 (Ra = identity: 2 ulps, no more)
        _, Rmp = S.rodrigues_mp(np.array(gx[:3], f32))
        Ra = np.array(last.pose_in.R[:], np.float64).reshape(3, 3)
        want = Ra @ np.array([float(v) for v in Rmp]).reshape(3, 3)
        ident = np.array_equal(Ra, np.eye(3))
        bound = (2.0 if ident else 2.0 * np.abs(Ra).sum(axis=1, keepdims=True) + 1.5) * S.ULP1
        assert np.all(np.abs(G[:3, :3].astype(np.float64) - want) <= bound), (c.name, route)
    else:
        assert np.array_equal(G, O)  # the pose the failing iteration was entered with
    return rc


_healthy = {}


def healthy_like(c):
    """The healthy twelve-correspondence system(s) for c's context (same thresholds and iteration counts)."""
    if len(c.levels) == 1:
        return S.case("det_double")
    if c.iters not in _healthy:
        _healthy[c.iters] = S._loop("healthy_%d%d%d" % c.iters[:3], S.healthy_levels(), c.iters[:3])
    return _healthy[c.iters]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", S.SINGLE + S.LOOP)
def test_icp_step(name, route):
    c = S.case(name)
    kf = ctx(c, route)
    set_route(kf, c, route)
    rc = track_and_check(kf, c, route)
    if rc == KFX_TRACKING_LOST:
        # straight after the early exit: the persistent kernel's exit ticket must have cleared IcpSync's slots,
        # counters and release flags; the per-launch routes their shards and ticket
        h = healthy_like(c)
        assert (h.dist, h.deg, h.iters, len(h.levels)) == (c.dist, c.deg, c.iters, len(c.levels))
        assert track_and_check(kf, h, route) == KFX_OK
    if route == "strided":
        kf.debug_cap_icp_blocks(0)
