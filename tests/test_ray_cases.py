"""Every case of ray_cases.py reaches what it is named for, asserted on the
oracle alone (no GPU): the classes below are counted from the oracle's maps and
from the float32 restatement of the rays and of the march in ray_cases.py.

Classes (pixels):
  zx_hit / zy_hit / zz_hit  hits whose dir.x / dir.y / dir.z is exactly zero
                            (float32, the oracle's written order)
  zero_miss     rays with an exact-zero component that cross the volume
                (ray0 < tfar) and end without a hit
  nan_prologue  a component of tbot / ttop is NaN (inf 0)
  graze         tnear == tfar > 0, finite: the ray meets an edge of the volume
  tiny(_hit)    a non-zero component below 2^-40 that is not subnormal
  subnormal     a subnormal component
  resumed       the first +/- candidate did not become the hit: its normal was
                NaN and the march went on; resumed_hit: and hit further on
  stop_last     the ray ended at a -/+ event whose sample is voxel z = dim - 2
  prev_exact    hits whose sample before the event is the named voxel slice:
                tall1040's sheets facing -z at s.5 have it at floor(s), those
                facing +z at ceil(s); TALL_BRICKS names the brick, brick word
                and super-brick word that slice lies in

MEASURED holds what the oracle gave when the table was written; a test asserts
at least half of it, never less than 8 pixels.  Found unreachable: a NaN normal
seen from inside a volume of cubic voxels (ray_cases.py's docstring):
shell32_pz_inside is named for stop_last instead, and the resumes are reached
from outside (shell32_*_outside) and with three voxel sizes (aniso52_*).
"""
import numpy as np
import pytest

import oracle as O
import ray_cases as RS
from kfx.abi import Pose
from test_gpu_ray_chain import feq

MEASURED = {
    "sphere32_pz_tie_even": {"zx_hit": 31, "zy_hit": 33, "zero_miss": 48},
    "sphere32_pz_tie_odd": {"zx_hit": 32, "zy_hit": 30, "zero_miss": 50},
    "sphere32_pz_lattice": {"zx_hit": 34, "zy_hit": 33, "zero_miss": 45},
    "sphere32_pz_control": {"hits": 822},
    "sphere32_pz_x0": {"nan_prologue": 48, "zy_hit": 13, "zero_miss": 18},
    "sphere32_pz_xrange": {"nan_prologue": 48, "zy_hit": 11, "zero_miss": 21},
    "sphere32_nz_farface": {"zx_hit": 47, "zy_hit": 48, "zero_miss": 17},
    "sphere32_pz_inside": {"zx_hit": 48, "zy_hit": 64},
    "sphere32_px_tie": {"zy_hit": 32, "zz_hit": 33, "zero_miss": 47},
    "sphere32_nx_lattice": {"zy_hit": 31, "zz_hit": 30, "zero_miss": 51},
    "sphere32_py_tie": {"zx_hit": 31, "zz_hit": 31, "zero_miss": 50},
    "sphere32_ny_lattice": {"zx_hit": 33, "zz_hit": 33, "zero_miss": 46},
    "sphere32_px_cos": {"tiny": 48, "tiny_hit": 33, "zy_hit": 32, "zero_miss": 32},
    "sphere32_py_cos": {"tiny": 64, "tiny_hit": 31, "zx_hit": 31, "zero_miss": 17},
    "sphere32_nz_cos": {"tiny": 48, "tiny_hit": 31, "zy_hit": 31, "zero_miss": 33},
    "sphere32_px_sub": {"subnormal": 111, "hits": 836},
    "sphere32_pz_sub": {"subnormal": 111, "hits": 807},
    "sphere32_obl": {"hits": 930},
    "sphere32_px_plane_z0": {"nan_prologue": 64, "zy_hit": 12, "zero_miss": 11},
    "sphere32_px_plane_zrange": {"nan_prologue": 64, "zy_hit": 12, "zero_miss": 12},
    "sphere32_pz_corner": {"graze": 48, "zy_hit": 18, "zero_miss": 77},
    "sphere32_pz_behind": {"zero_pixels": 111},
    "blob64_pz_corner8": {"zx_hit": 10, "zy_hit": 9, "zero_miss": 93},
    "blob64_px_corner8": {"zy_hit": 10, "zz_hit": 9, "zero_miss": 93},
    "blob64_obl_corner8": {"hits": 120},
    "blob64_pz_corner32_inside": {"zx_hit": 11, "zy_hit": 11, "zero_miss": 90},
    "blob64_ny_corner32_inside": {"zx_hit": 11, "zz_hit": 11, "zero_miss": 90},
    "blob64_nx_cos_corner32_inside": {"tiny": 48, "tiny_hit": 9, "zy_hit": 10, "zero_miss": 54},
    "blob64_obl_corner32_inside": {"hits": 162},
    "shell32_pz_outside": {"resumed": 3071, "resumed_hit": 360, "zx_hit": 19, "zy_hit": 17},
    "shell32_nx_cos_outside": {"tiny": 48, "tiny_hit": 16, "zy_hit": 16, "resumed": 3072, "resumed_hit": 348},
    "shell32_pz_inside": {"stop_last": 840, "zx_hit": 37, "zy_hit": 46},
    "aniso52_pz": {"resumed": 176, "zx_hit": 41, "zy_hit": 28},
    "aniso52_px": {"resumed": 71, "zy_hit": 27, "zz_hit": 57},
    "aniso52_obl": {"hits": 2145, "resumed": 382},
    "tall1040_pz_508.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
    "tall1040_pz_511.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
    "tall1040_pz_512.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
    "tall1040_pz_519.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
    "tall1040_pz_1020.5": {"prev_exact": 729, "zx_hit": 27, "zy_hit": 27},
    "tall1040_pz_1027.5": {"prev_exact": 729, "zx_hit": 27, "zy_hit": 27},
    "tall1040_pz_1036.5": {"prev_exact": 729, "zx_hit": 27, "zy_hit": 27},
    "tall1040_nz_3.5": {"prev_exact": 729, "zx_hit": 27, "zy_hit": 27},
    "tall1040_nz_7.5": {"prev_exact": 729, "zx_hit": 27, "zy_hit": 27},
    "tall1040_nz_8.5": {"prev_exact": 729, "zx_hit": 27, "zy_hit": 27},
    "tall1040_nz_503.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
    "tall1040_nz_511.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
    "tall1040_nz_512.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
    "tall1040_nz_519.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
    "tall1040_pz_inside_1020.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
    "tall1040_nz_inside_519.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
    "tall1040_nz_inside_512.5": {"prev_exact": 1024, "zx_hit": 32, "zy_hit": 32},
}

# sheet -> (voxel slice of the sample before the event, its brick, brick word, super-brick word)
TALL_BRICKS = {
    ("pz", 508.5): (508, 63, 0, 0), ("pz", 511.5): (511, 63, 0, 0), ("pz", 512.5): (512, 64, 1, 0),
    ("pz", 519.5): (519, 64, 1, 0), ("nz", 503.5): (504, 63, 0, 0),
    ("pz", 1020.5): (1020, 127, 1, 0), ("pz", 1027.5): (1027, 128, 2, 1), ("pz", 1036.5): (1036, 129, 2, 1),
    ("nz", 3.5): (4, 0, 0, 0), ("nz", 7.5): (8, 1, 0, 0), ("nz", 8.5): (9, 1, 0, 0),
    ("nz", 511.5): (512, 64, 1, 0), ("nz", 512.5): (513, 64, 1, 0), ("nz", 519.5): (520, 65, 1, 0),
}


def floor_of(measured):
    return max(8, measured // 2)


def measure(name):
    case = RS.CASES[name]
    p = RS.populations(name)
    if case.vname == "tall1040":
        z = TALL_BRICKS[case.rot, case.vol[1]][0]
        p["prev_exact"] = RS.prev_in(p, 2, z, z)
    if name == "shell32_pz_inside":
        p["stop_last"] = int((p["_stop"] & (p["_stop_vox"][..., 2] == case.dims[2] - 2)).sum())
    return p


def test_table_shape():
    assert 40 <= len(RS.CASES) <= 60 and sorted(MEASURED) == sorted(RS.CASES)
    assert all(v >= 8 for m in MEASURED.values() for v in m.values())
    for (rot, s), (z, b, bw, sw) in TALL_BRICKS.items():
        assert (z >> 3, z >> 9, z >> 10) == (b, bw, sw)
    Z = RS.GEOM["tall1040"][0][2]
    assert ((Z + 7) // 8 + 63) // 64 == 3 and ((Z + 31) // 32 + 31) // 32 == 2
    # the first and last bricks of brick words 0 / 1 / 2 and of super-brick words 0 / 1 are all named
    assert {b for _, b, _, _ in TALL_BRICKS.values()} >= {0, 63, 64, 127, 128, 129}
    assert {(z >> 5) for z, *_ in TALL_BRICKS.values()} >= {0, 31, 32}


@pytest.mark.parametrize("name", list(RS.CASES))
def test_case_reaches_its_classes(name):
    case = RS.CASES[name]
    p = measure(name)
    print(name, {k: v for k, v in p.items() if not k.startswith("_")})
    for cls, was in MEASURED[name].items():
        assert p[cls] >= floor_of(was), (name, cls, p[cls], was)
    if name.endswith("control") or case.rot == "obl":
        assert p["zero_pixels"] == 0 and p["nan_prologue"] == 0
    if name.endswith("behind"):
        assert p["crossing"] == 0 and p["hits"] == 0
    if case.rot.endswith("_sub"):
        assert p["zero_pixels"] == 0  # the components survive as subnormals on the host
    if "plane" in name or "_x0" in name or "xrange" in name:
        # a ray in a face plane, or the zero column on one: fmin / fmax drop the NaN, the ray never marches
        r = RS.rays(case)
        nan = np.zeros(r.ray0.shape, bool)
        for a in r.tb + r.tt:
            nan |= np.isnan(a)
        with np.errstate(invalid="ignore"):
            assert not (nan & (r.ray0 < r.tfar)).any()


@pytest.mark.parametrize("name", list(RS.CASES))
def test_case_inputs_are_what_the_gpu_paths_assume(name):
    """The camera pose handed to kfx_render_view gives the case's cam2vol bit
    for bit under the library's pose arithmetic (subnormal entries included),
    the full-range slab restatement equals the plain raycast, and the numpy
    march agrees with the oracle where it is used: every hit has a candidate,
    and a hit made of the first candidate has Ts within one step before it."""
    case = RS.CASES[name]
    c2v = O.pose_mul(O.pose_inv(case.params.volu_pose), Pose.from_matrix(case.pose))
    for a, b in ((c2v.R, case.cam2vol.R), (c2v.t, case.cam2vol.t)):
        assert np.array_equal(np.array(a[:], np.float32).view(np.uint32), np.array(b[:], np.float32).view(np.uint32))
    e = RS.expected(name)
    assert feq(e["slab_maps"][0], e["maps"][0][0]) and feq(e["slab_maps"][1], e["maps"][0][1])
    hit = RS.hit_mask(e["maps"][0][1])
    assert np.array_equal(hit, e["ts"] != 0)
    m = RS.march(case)
    assert not (hit & ~(m.cand_len > 0)).any()
    p = RS.populations(name)
    first = p["_first"]
    step = np.float32(case.range[0]) / np.float32(case.dims[0])
    ts = e["ts"]
    assert (ts[first] <= m.cand_len[first]).all() and (ts[first] >= m.cand_len[first] - step * np.float32(1.001)).all()


@pytest.mark.parametrize("name", RS.AXIS_ALIGNED_BOX)
def test_tight_box_reference(name):
    """The tighter box of the world view moves the validity limit into the
    volume: the reference differs from the window's, and still sees the sphere."""
    ref = RS.box_reference(name)
    e = RS.expected(name)
    hits = int(ref["hit"].sum())
    print(name, "box hits", hits, "window hits", int((e["ts"] != 0).sum()))
    if name.startswith("sphere32") and not name.endswith("behind"):
        assert hits >= 60  # measured 120 .. 2959
        assert not np.array_equal(ref["ts"], e["ts"])
    if name.startswith("blob64") and "corner8" in name:
        assert hits == 0  # the box's first valid voxel is 9: the blob's voxels 7 / 8 lie outside it
    if name.startswith("blob64") and "corner32" in name:
        assert hits >= 60  # measured 121
