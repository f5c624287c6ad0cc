"""The crafted ICP cases (tests/icp_cases.py) judged on the CPU alone: the C++
oracle's kfo_icp_accumulate equals the numpy restatement on every one of them,
all 27 sums, the per-pixel labels the generators intend are the restatement's,
and every case does what it is for (no vacuous class)."""
import numpy as np
import pytest

import icp_cases as K
from kfx.abi import Pose

SIZES = [(32, 32), (80, 48), (96, 32), (256, 128), (320, 240), (160, 120), (80, 60), (512, 288), (640, 480)]


def _run(case, dist, deg, pose, **kw):
    return K.accumulate_np(case.cur_v, case.cur_n, case.pre_v, case.pre_n, case.I, pose, dist, K.sinf_deg(deg), **kw)


def _oracle(oracle_lib, case, dist, deg, pose):
    return oracle_lib.icp_accumulate(case.cur_v, case.cur_n, case.pre_v, case.pre_n, case.I, pose, dist,
                                     float(K.sinf_deg(deg)))


def _tagged(case, r, prefix):
    ks = [k for k, t in enumerate(case.tags) if t.startswith(prefix)]
    return np.isin(case.tag, ks)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(K.case_table()))
def test_oracle_equals_restatement_and_labels(name, size, oracle_lib):
    case, dist, deg = K.crafted(name, *size)
    r = _run(case, dist, deg, Pose.identity(), keep_scaled=True)
    assert np.array_equal(K.sums_i64(r.sums), _oracle(oracle_lib, case, dist, deg, Pose.identity()))
    assert np.array_equal(r.label, case.label), np.argwhere(r.label != case.label)[:8]
    moved = _run(case, dist, deg, K.moved_pose())
    assert np.array_equal(K.sums_i64(moved.sums), _oracle(oracle_lib, case, dist, deg, K.moved_pose()))
    assert moved.accepted.sum() > moved.accepted.size // 2  # the moved pose still exercises the products

    # not vacuous, on the reference alone
    assert r.rejected["nan"].sum() <= r.label.size // 2
    assert r.accepted.any()
    cls = name[0]
    if cls == "a":
        for g in K.GATES:
            assert r.rejected[g].any(), g
        for t in ("cur_nx", "cur_ny", "z_zero", "z_negzero", "z_neg", "z_denormal", "v_zero", "v_nan_x", "m_nan_x",
                  "mn_nan_x", "mn_zero"):
            assert _tagged(case, r, t).any(), t
        assert np.all(r.label[_tagged(case, r, "cur_ny")] == K.ANGLE)  # not the isnan gate
        zero_n = _tagged(case, r, "mn_zero")
        assert np.all(r.accepted[zero_n]) and not r.terms[zero_n.ravel()].any()  # accepted, zero rows
    if cls == "b":
        assert r.rejected["proj"].any()
        for axis, p in ((0, r.pu), (1, r.pv)):
            tie = (p - np.floor(p) == 0.5) & (_tagged(case, r, "tie_") | _tagged(case, r, "left_tie")
                                              | _tagged(case, r, "right_tie") | _tagged(case, r, "top_tie")
                                              | _tagged(case, r, "bottom_tie"))
            q = (r.px, r.py)[axis]
            assert (tie & (q > p)).any() and (tie & (q < p)).any(), axis  # a tie up and a tie down
        w, h = size
        for t, lab in (("left_tie_in", K.ACCEPT), ("left_out", K.PROJ), ("right_tie_out", K.PROJ),
                       ("right_in", K.ACCEPT), ("right_exact", K.ACCEPT), ("top_tie_in", K.ACCEPT),
                       ("bottom_tie_out", K.PROJ), ("bottom_exact", K.ACCEPT)):
            m = _tagged(case, r, t)
            assert m.any() and np.all(r.label[m] == lab), t
        assert (r.accepted & (r.px == w - 1)).any() and (r.accepted & (r.py == h - 1)).any()
        xe, ye = K.region(w, h)
        if w > xe:
            assert (r.accepted & (r.px >= xe)).any()
        if h > ye:
            assert (r.accepted & (r.py >= ye)).any()
    if cls in "cd":
        gate, val = ("dist", r.dist2) if cls == "c" else ("angle", r.sine2)
        lad = _tagged(case, r, "rung")
        assert (lad & r.accepted).any() and (lad & r.rejected[gate]).any()  # the ladder straddles
        for k in K.RUNGS:  # and sits where it was aimed, ulp by ulp
            m = _tagged(case, r, f"rung{k:+d}")
            assert m.any() and np.all(val[m] == K.step(case.bound, k)), k
        assert np.sqrt(case.bound) <= case.thr < np.sqrt(K.step(case.bound, 1))
        if name.endswith("above_square"):
            assert case.bound > case.thr * case.thr
    if cls == "e":
        sc = r.scaled[_tagged(case, r, "halves").ravel()].astype(np.float64)
        rounded = np.rint(sc)
        frac = sc - np.floor(sc)
        for sign in (1, -1):
            tie = (frac == 0.5) & (np.sign(sc) == sign)
            assert (tie & (rounded > sc)).any() and (tie & (rounded < sc)).any(), sign
            assert ((frac == 0.25) & (np.sign(sc) == sign)).any() and ((frac == 0.75) & (np.sign(sc) == sign)).any()
        sub = _tagged(case, r, "subnormal")
        n = r.row[sub][:, 3:6].astype(np.float64)
        assert np.all(np.abs(n[:, 0] * n[:, 1]) < 2.0 ** -126) and np.all(n != 0)
        assert not r.terms[sub.ravel()].any()  # every product of a 2^-70 row rounds to 0
        assert r.terms[_tagged(case, r, "unit").ravel()][:, 0:27].any()


@pytest.mark.parametrize("zfar,slant", [(12.0, False), (30.0, False), (30.0, True)],
                         ids=["f_wall_12m", "f_wall_30m", "f_slant_30m"])
def test_magnitude_cases_cross_2_53_where_stated(zfar, slant, oracle_lib):
    """Class f on the reference alone: the 12 m wall keeps every 8192-pixel
    block's sums below 2^53, the 30 m scenes do not, and 1024-pixel blocks stay
    below it in all three (the form the derived bound leaves for them)."""
    case = K.gen_magnitude(zfar, slant)
    dist, ang = 0.015, K.sinf_deg(30.0)
    r = K.accumulate_np(case.cur_v, case.cur_n, case.pre_v, case.pre_n, case.I, Pose.identity(), dist, ang)
    assert np.array_equal(K.sums_i64(r.sums), oracle_lib.icp_accumulate(case.cur_v, case.cur_n, case.pre_v,
                                                                         case.pre_n, case.I, Pose.identity(), dist,
                                                                         float(ang)))
    assert r.accepted.all()
    big, small = K.block_sum_report(r.terms, 8192), K.block_sum_report(r.terms, 1024)
    print(f"zfar {zfar} slant {slant}: largest |block sum| 2^{np.log2(max(big.max_abs_sum)):.2f} per 8192 pixels, "
          f"2^{np.log2(max(small.max_abs_sum)):.2f} per 1024")
    assert (max(big.max_abs_sum) >= 2 ** 53) == (zfar == 30.0)
    assert max(small.max_sum_abs) < 2 ** 53


@pytest.mark.parametrize("kind", ["none", "one", "three", "six", "one_plane", "two_planes", "three_planes"])
def test_degenerate_systems_on_the_oracle(kind, oracle_lib):
    I = K.crafted_intrinsics(64, 64)
    case = K.gen_degenerate(kind, I)
    r = K.accumulate_np(case.cur_v, case.cur_n, case.pre_v, case.pre_n, I, Pose.identity(), 0.015, K.sinf_deg(30.0))
    sums = oracle_lib.icp_accumulate(case.cur_v, case.cur_n, case.pre_v, case.pre_n, I, Pose.identity())
    assert np.array_equal(K.sums_i64(r.sums), sums)
    counts = {"none": 0, "one": 1, "three": 3, "six": 6}
    if kind in counts:
        assert r.accepted.sum() == counts[kind]
    else:
        assert r.accepted.sum() > r.accepted.size // 2
    st, _, _ = oracle_lib.icp_update(sums, Pose.identity())
    if kind in ("none", "one", "three", "one_plane"):
        assert st == 1  # rank-deficient: the solve must refuse
    if kind == "three_planes":
        assert st == 0
