"""The raycast kernels over ray space against the oracle, bit for bit: every
case of ray_cases.py (exact-zero direction components, NaN prologues, origins
on faces and lattice points, tiny and subnormal components, NaN-normal
resumes, surfaces in the first and last bricks of the occupancy words) through
each hand-kept copy of the march:

  k_raycast<idx32>, k_raycast<idx64>   stage_raycast, plain and forced 64-bit index
  k_raycast<.., kSlab>                 stage_raycast on a slab context of world 1
  k_view                               kfx_render_view at the pose that gives the case's cam2vol
  k_world_view                         kfx_world_view with the box equal to the window (equal to
                                       k_view's bytes), and for the axis-aligned sphere32 / blob64
                                       cases with the box one brick inside the window (the
                                       oracle's raycast on the dense assembly of the cut bricks)

Every pixel is compared, none masked; NaNs are matched by position.  What each
case reaches is asserted on the oracle alone in test_ray_cases.py.  Multi-slab
groups have no staged raycast entry: test_ray_chain_slab_group is their test.

Each test holds one context of at most 64^3 or 16 x 16 x 1040 voxels and
launches one to four raycasts of at most 64 x 48 pixels.
"""
import numpy as np
import pytest

import ray_cases as RS
import ref_cases as R
import world_view_cases as W
from kfx import KFX_FRAME_PREV, KinectFusion
from test_gpu_ray_chain import feq

pytestmark = pytest.mark.gpu
NAMES = list(RS.CASES)


def context(case, path="idx32"):
    kf = KinectFusion(case.intr, case.params, slab=(0, 1) if path == "slab" else None)
    if path == "idx64":
        kf.debug_force_index64(True)
    kf.upload_tsdf(RS.records(case))
    return kf


def assert_maps(got_v, got_n, want_v, want_n, what):
    for tag, g, w in (("vmap", got_v, want_v), ("nmap", got_n, want_n)):
        n, first = R.differing(np.ascontiguousarray(g, np.float32), np.ascontiguousarray(w, np.float32))
        assert n == 0 and feq(g, w), f"{what} {tag}: {n} of {w.size} elements differ, first at {first}"


@pytest.mark.parametrize("path", ["idx32", "idx64", "slab"])
@pytest.mark.parametrize("name", NAMES)
def test_staged_raycast(name, path):
    """stage_raycast's maps of levels 0, 1 and 2 against O.raycast and
    O.resize_points_normals; the plain path also against the digest recorded
    from the reference's own kernel.  The slab context owns the whole volume
    (world 1): kfx_stage_raycast expands the slab kernel's payload into the
    same maps.  Its pre-skip does not engage there (the march starts at tnear,
    inside the stored slices, so nf < 2 for every ray) and its own-range exits
    lie outside the volume: test_ray_chain_slab_group holds those."""
    case = RS.CASES[name]
    want = RS.expected(name)["maps"]
    out = []
    with context(case, path) as kf:
        kf.stage_raycast(case.cam2vol, case.Rinv)
        for l, (ov, on) in enumerate(want):
            _, gv, gn = kf.frame_maps(KFX_FRAME_PREV, l)
            assert_maps(gv, gn, ov, on, f"{name} {path} level {l}")
            out += [(f"vmap{l}", gv), (f"nmap{l}", gn)]
    if path == "idx32":
        cid = f"rayspace/{name}"
        assert R.recorded(cid, out) == R.golden()["cases"][cid]


def assert_view(got, ref, what):
    img, v, n, ts = got
    assert_maps(v, n, ref["vmap"], ref["nmap"], what)
    assert feq(ts, ref["ts"]), f"{what} ts"
    assert np.array_equal(img, ref["normal"]), f"{what} normal image"


@pytest.mark.parametrize("force64", [False, True], ids=["idx32", "idx64"])
@pytest.mark.parametrize("name", NAMES)
def test_views(name, force64):
    """kfx_render_view (vmap, nmap, ts and the normal-colour image against the
    oracle), kfx_world_view with the window's own bricks and the box equal to
    the window (kfx_render_view's bytes, normal and fused-colour images), and
    for the axis-aligned sphere32 / blob64 cases the box one brick inside."""
    case = RS.CASES[name]
    e = RS.expected(name)
    ref = dict(vmap=e["slab_maps"][0], nmap=e["slab_maps"][1], ts=e["ts"], normal=e["normal"])
    with context(case, "idx64" if force64 else "idx32") as kf:
        dense = {k: kf.render_view(case.intr, case.pose, k, maps=True) for k in ("normal", "color")}
        assert_view(dense["normal"], ref, f"{name} render_view")
        bricks = kf.world_bricks()
        assert bricks.tobytes() == RS.window_bricks(case).tobytes()
        kf.world_view_load(bricks, box=((0, 0, 0), case.dims))
        for k, d in dense.items():
            got = kf.world_view(case.intr, case.pose, k, maps=True)
            for tag, a, b in zip(("image", "vmap", "nmap", "ts"), got, d):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{name} world_view {k} {tag}"
        if name in RS.AXIS_ALIGNED_BOX:
            kf.world_view_load(bricks, box=RS.tight_box(case))
            W.assert_view(("normal", kf.world_view(case.intr, case.pose, "normal", maps=True)), RS.box_reference(name),
                          f"{name} tight box")
