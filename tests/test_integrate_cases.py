"""The integrate case table (integrate_cases.py) is not vacuous: every case
reaches what it is listed for, judged on the oracle alone (no GPU).

Floors are conditions, about half of the populations the oracle showed when
the table was written; a case that falls below one no longer tests its path
and must be re-aimed, whatever the device kernel computes.
"""
import numpy as np
import pytest

import integrate_cases as IC


@pytest.mark.parametrize("name", [n for n in IC.CASES if n not in IC.EMPTY])
def test_populations(name):
    case = IC.CASES[name]
    steps, _ = IC.oracle_zeroed(name)
    floors = IC.FLOORS[name]
    assert len(steps) == len(floors) == len(case.poses)
    for k, (((nu, nc), t, w, _), (fu, fc, fn)) in enumerate(zip(steps, floors)):
        neg = int((t < 0).sum())
        print(f"{name} launch {k}: updated {nu} coloured {nc} negative {neg} weight>=2 {int((w >= 2).sum())}")
        assert nu >= fu >= (500 if name == "odd" else 1000), (k, nu)
        if fc is not None:
            assert nc >= fc >= 100, (k, nc)
        if fn is not None:
            assert neg >= fn >= 100, (k, neg)
        if k > 0:  # a later launch of a sequence meets voxels the earlier ones wrote
            assert int((w >= 2).sum()) >= 1000, (k, int((w >= 2).sum()))


@pytest.mark.parametrize("name", IC.EMPTY)
def test_empty_cases_update_nothing(name):
    steps, _ = IC.oracle_zeroed(name)
    ((nu, nc), t, w, c), = steps
    assert (nu, nc) == (0, 0) and not t.any() and not w.any() and not c.any()
    # ... and nothing of an uploaded volume either (what the GPU test starts from)
    case = IC.CASES[name]
    init = IC.random_volume(case.dims)
    (((nu, nc), t, w, c),), _ = IC.integrate_steps(case, init)
    assert (nu, nc) == (0, 0)
    assert np.array_equal(t, init[0]) and np.array_equal(w, init[1]) and np.array_equal(c, init[2])


def _tiles(name):
    case = IC.CASES[name]
    steps, _ = IC.oracle_zeroed(name)
    upd = IC.tiles_of(IC.updated_columns(case, steps[0][2]))
    slow = IC.tiles_of(~IC.column_fast(case, case.poses[0]))
    return upd, slow


@pytest.mark.parametrize("name", ["axis_x_cos", "tilt_1e-6"])
def test_every_updated_tile_takes_the_ieee_loop(name):
    upd, slow = _tiles(name)
    assert upd.sum() >= 24 and not (upd & ~slow).any(), (int(upd.sum()), int((upd & ~slow).sum()))
    # every column, not only one per tile: the deciding component is the pose's
    case = IC.CASES[name]
    assert not IC.column_fast(case, case.poses[0]).any()


def test_fast_cases_take_the_fast_loop():
    """The control, and the exact twin of axis_x_cos: no slow column at all."""
    for name in ("base", "axis_x", "plane", "oblique"):
        case = IC.CASES[name]
        assert IC.column_fast(case, case.poses[0]).all(), name


def test_mixed_has_slow_and_fast_tiles():
    upd, slow = _tiles("mixed")
    ns, nf = int((upd & slow).sum()), int((upd & ~slow).sum())
    print(f"mixed: {ns} slow and {nf} fast updated tiles")
    assert ns >= 5 and nf >= 30
    case = IC.CASES["mixed"]
    fast = IC.column_fast(case, case.poses[0])
    assert not fast[:, 5].any() and fast[:, :5].all() and fast[:, 6:].all()  # column 5 alone decides


def test_plane_has_exact_zeros():
    case = IC.CASES["plane"]
    vc = IC.accumulated(case, case.poses[0])  # (Z, Y, X, 3)
    steps, _ = IC.oracle_zeroed("plane")
    upd = IC.updated_columns(case, steps[0][2])
    assert (vc[8, ..., 2] == 0.0).all() and (vc[9, ..., 2] > 0).all()
    assert (vc[0, :, 32, 0] == 0.0).all() and upd[:, 32].any()
    assert IC.column_fast(case, case.poses[0]).all()  # ... in the fast loop
    # the same sums in double: the float adds were exact
    vc0, zs = IC.columns(case, case.poses[0])
    assert np.array_equal(vc[-1].astype(np.float64), vc0.astype(np.float64) + 63 * zs.astype(np.float64))


def test_clip_branches_by_pose():
    """sz == 0 exactly, sz tiny, sz < 0: the signs of beta the clips meet."""
    zs = {n: IC.columns(IC.CASES[n], IC.CASES[n].poses[0])[1] for n in IC.CASES}
    assert zs["axis_x"][2] == 0.0 and zs["axis_y"][2] == 0.0
    assert 0 < abs(zs["axis_x_cos"][2]) < 2.0 ** -55
    assert zs["reversed"][2] == -zs["base"][2] < 0 and zs["reversed"][0] == 0.0
    assert zs["reversed_gen"][2] < 0 and zs["reversed_gen"][0] != 0
    assert min(abs(zs["oblique"])) > 0.2 * max(abs(zs["oblique"]))
    # vc.z is constant along a column there.  axis_x: whole columns beyond the
    # far clip (alpha < 0 under beta == 0) beside columns inside it
    case = IC.CASES["axis_x"]
    vc0, _ = IC.columns(case, case.poses[0])
    zfar = (float(IC.depth_maps(case.frame).max()) + case.params.volu_trun_dist) * 1.02 + 0.01
    assert (vc0[..., 2] > zfar + 0.01).sum() >= 64 and (vc0[..., 2] < zfar - 0.05).sum() >= 64
    # axis_x_behind: whole columns behind the camera beside columns in front of it
    case = IC.CASES["axis_x_behind"]
    vc0, _ = IC.columns(case, case.poses[0])
    assert (vc0[..., 2] < -0.05).sum() >= 64 and (vc0[..., 2] > 0.05).sum() >= 64
    # inside: vc.z changes sign along columns
    case = IC.CASES["inside"]
    vz = IC.accumulated(case, case.poses[0])[..., 2]
    assert ((vz[0] < 0) & (vz[-1] > 0)).sum() >= 1000


def test_deep_coarse_tiles_differ_in_length():
    case = IC.CASES["deep_coarse"]
    steps, _ = IC.oracle_zeroed("deep_coarse")
    spans = IC.tile_spans(case, steps[0][2])
    print(f"deep_coarse: {spans.size} updated tiles, spans {spans.min()}..{spans.max()} slices")
    assert spans.size >= 12 and spans.max() >= 2 * spans.min()


def test_uploaded_volume_covers_the_weight_range():
    t, w, c = IC.random_volume((64, 64, 64))
    assert w.min() == 0 and w.max() == 255 and (w > 64).sum() > 100000 and (t < 0).sum() > 10000
    case = IC.CASES["oblique"]
    steps, _ = IC.integrate_steps(case, (t, w, c))
    (nu, nc), _, w1, _ = steps[0]
    assert nu >= 46000 and ((w == 255) & (w1 == 64)).sum() >= 100  # weights fall from 255 to 64
