"""k_raycast's sample-index march bound against the oracle, bit for bit.

The march carries sample indices instead of ray_len (kend from
kfx::ray_sample_end once per ray, a hit's ray_len from one ff_add); these
cases walk every way a ray can end through kend and the hit / resume state,
each on the plain, the forced 64-bit-index and the 2-slab kernels.

Volumes are fused by the oracle from three 160x120 frames of the synthetic
scene (64^3 at 32 mm; one 64x64x128) and uploaded; each case raycasts one
through stage_raycast from its own camera pose.  kfx_raycast_stats marches
from the pipeline's tracked pose and the three-level ICP does not track at
160x120, so the classes only the kernel's counters show (blocked lookups, a
resumed normal pass) are asserted on tracked 320x240 frames, single volume and
2-slab group; the resume needs the face placement with non-cubic voxels
(FUSED["facez"], and FUSED["facet"], which a slab's halo still covers).

Populations of each case, from the oracle's maps alone (hit pixels / pixels
whose ray crosses the volume and ends without a hit / hits whose trilinear
cell has gx & 7 == 7 / gy & 7 == 7):
    outside   15109 / 4091 / 1425 / 1795    inside    17433 / 1767 / 2264 / 2033
    leaving    6181 / 13019 / 564 / 1218    face       8109 / 11091 / 581 / 1047
    tall      15096 / 4104 / 1528 / 1852
Tracked 320x240 frames, hits / pixels without: cube 58729 / 18071, face
40255 / 36545, tall 59352 / 17448, facez 4589 / 72211, facet 60908 / 15892.
"""
import math

import numpy as np
import pytest

import oracle as O
from kfx import KFX_FRAME_PREV, KFX_OK, KinectFusion, pipeline_group, synth
from kfx.abi import Intrinsics, Pose, default_params

pytestmark = pytest.mark.gpu

L_VOL = 2.048
VS = L_VOL / 64
WALL_Z = 0.5 + 0.9 * L_VOL  # the scene's back wall (synth.Scene.default)
VS_THIN = VS / 1.034


def feq(a, b):
    """Bit equality of float32 arrays with NaNs compared by position."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    z = np.float32(0)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(
        np.where(na, z, a).view(np.uint32), np.where(nb, z, b).view(np.uint32))


def records(t, w, c):
    rec = np.zeros(t.size, dtype=np.dtype([("tsdf", "<i2"), ("weight", "<i2"), ("rgb", "u1", 3), ("pad", "u1")]))
    rec["tsdf"], rec["weight"] = t, w
    rec["rgb"] = c.reshape(-1, 4)[:, :3]
    return rec


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = [x, y, z]
    return m


def rot_y(a):
    m = np.eye(4)
    c, s = math.cos(a), math.sin(a)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s, -s, c
    return m


# volume -> world placement the scene is fused under, and its z dimension
FUSED = {
    "cube": (translate(-L_VOL / 2, -L_VOL / 2, 0.5), 64, L_VOL),
    # the back wall 1.5 voxels inside the far z face
    "face": (translate(-L_VOL / 2, -L_VOL / 2, WALL_Z + 1.5 * VS - L_VOL), 64, L_VOL),
    # 64 x 64 x 128: the scene spans z bricks 2 .. 11
    "tall": (translate(-L_VOL / 2, -L_VOL / 2, -0.6), 128, 2 * L_VOL),
    # the face placement with 128 slices of 16 mm over the same range.  The
    # reference steps a ray's samples by dir * voxel_size per axis but its
    # ray_len by voxel_size.x (tsdf_volume.cu:210-260), so with thinner slices
    # a hit's vertex org + dir * Ts runs ahead of the samples in z: behind the
    # front half of the volume it lies past the far face, the interpolation is
    # invalid, the normal NaN, and the march resumes
    "facez": (translate(-L_VOL / 2, -L_VOL / 2, WALL_Z + 1.5 * VS - L_VOL), 128, L_VOL),
    # the same effect kept within a slab's halo: 64 slices 3.4 % thinner than
    # the voxels are wide, the wall one slice inside the far face.  The vertex
    # leads its sample by up to 2.1 slices at the far face (64 * 0.034), so the
    # normal reads at most 4 slices past the sample and
    # the wall's hits whose vertex passes slice 62.5 resume
    "facet": (translate(-L_VOL / 2, -L_VOL / 2, WALL_Z + 1.0 * VS_THIN - 64 * VS_THIN), 64, 64 * VS_THIN),
}
# case: fused volume, camera -> world pose of the raycast's camera relative to
# the fusing camera (the volume pose of the case's context is its inverse
# applied to the fused placement)
CASES = {
    "outside": ("cube", np.eye(4)),                                # every ray has tnear > 0
    "inside": ("cube", translate(0.0, -0.1, 0.8)),                 # camera inside the volume: tnear <= 0
    "leaving": ("cube", translate(0.3, 0.0, 0.3) @ rot_y(0.5)),   # most rays leave through the +x face
    "face": ("face", np.eye(4)),
    "tall": ("tall", np.eye(4)),
}


def case_params(name):
    fused, cam = CASES[name]
    vpose, dimz, rangez = FUSED[fused]
    p = default_params(dims=64, range_m=L_VOL)
    p.volu_dims[2] = dimz
    p.volu_range[2] = rangez
    p.volu_trun_dist = default_params(dims=64, range_m=L_VOL).volu_trun_dist
    # camera at the world origin: the volume moves instead
    p.volu_pose = Pose.from_matrix(np.linalg.inv(cam) @ vpose)
    return p


def fuse(fused, intr, bgr, dep, gt):
    """The oracle's volume of three frames under FUSED[fused]."""
    vpose, dimz, rangez = FUSED[fused]
    I = Intrinsics.from_any(intr)
    p = default_params(dims=64, range_m=L_VOL)
    vol = O.Volume((64, 64, dimz), (L_VOL, L_VOL, rangez))
    vp = Pose.from_matrix(vpose)
    for k in range(3):
        ds, _, _ = O.preprocess(dep[k].astype(np.float32), I, p)
        vol2cam = O.pose_mul(O.pose_inv(Pose.from_matrix(gt[k])), vp)
        O.integrate(vol, p.volu_trun_dist, I, vol2cam, ds[0], bgr[k])
    return vol


def populations(vol, intr, cam2vol, ov, on):
    """(hits, crossing rays without a hit, hits at gx & 7 == 7, at gy & 7 == 7)."""
    c2v = cam2vol.matrix()
    hit = (on != 0).any(-1) & ~np.isnan(on).any(-1)
    u, v = np.meshgrid(np.arange(intr.width, dtype=np.float64), np.arange(intr.height, dtype=np.float64))
    d = np.stack([(u - intr.cx) / intr.fx, (v - intr.cy) / intr.fy, np.ones_like(u)], -1) @ c2v[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (0.0 - c2v[:3, 3]) / d
        t1 = (vol.range.astype(np.float64) - c2v[:3, 3]) / d
    tnear = np.minimum(t0, t1).max(-1)
    tfar = np.maximum(t0, t1).min(-1)
    crossing = np.maximum(tnear, 0.0) + VS < tfar
    pv = (ov[hit].astype(np.float64) @ c2v[:3, :3].T + c2v[:3, 3]) / VS
    g = np.floor(pv).astype(int)
    return int(hit.sum()), int((crossing & ~hit).sum()), int(((g[:, 0] & 7) == 7).sum()), int(((g[:, 1] & 7) == 7).sum())


@pytest.fixture(scope="module")
def seq():
    intr = synth.Intrinsics.qqvga()
    return (intr,) + synth.sequence(3, intr, noise=True, dropout=0.01)


@pytest.fixture(scope="module")
def fused(seq):
    return {k: fuse(k, *seq) for k in {fz for fz, _ in CASES.values()}}


@pytest.fixture(scope="module")
def expected(seq, fused):
    """Oracle maps of every case (levels 0..2), computed once."""
    intr = seq[0]
    I = Intrinsics.from_any(intr)
    out = {}
    for name, (fz, _) in CASES.items():
        p = case_params(name)
        cam2vol = O.pose_inv(p.volu_pose)
        Rinv = cam2vol.matrix()[:3, :3].T.copy()
        ov, on = O.raycast(fused[fz], I, cam2vol, Rinv)
        maps = [(ov, on)]
        for _ in (1, 2):
            maps.append(O.resize_points_normals(*maps[-1]))
        out[name] = (p, cam2vol, Rinv, maps)
    return out


@pytest.mark.parametrize("index64", [False, True], ids=["idx32", "idx64"])
@pytest.mark.parametrize("name", list(CASES))
def test_ray_chain_bit_exact(name, index64, seq, fused, expected):
    """Vertex and normal maps of every level against the oracle's, with the
    case's classes populated in the oracle's own output: >= 200 hits, >= 200
    rays that cross the volume and end without a hit (through kend inside a
    skip run, inside a batch or by the clear-box early end), >= 200 hits in
    cells on a tile's last column and on its last row.

    Not asserted here: blocked lookups > 0 per case (kfx_raycast_stats marches
    from the pipeline's tracked pose, not a staged one; the tracked tests
    below assert it), and which of the three ends through kend a case's
    no-hit rays take: nothing counts them apart, only the bit equality of
    every pixel with the oracle covers them."""
    intr = seq[0]
    vol = fused[CASES[name][0]]
    p, cam2vol, Rinv, maps = expected[name]
    hits, gone, ex, ey = populations(vol, intr, cam2vol, *maps[0])
    print(f"{name}: oracle hits {hits} crossing-without-hit {gone} gx7 {ex} gy7 {ey}")
    assert hits >= 200 and gone >= 200 and ex >= 200 and ey >= 200, (hits, gone, ex, ey)
    kf = KinectFusion(Intrinsics.from_any(intr), p)
    if index64:
        kf.debug_force_index64(True)
    kf.upload_tsdf(records(vol.tsdf, vol.weight, vol.rgb))
    kf.stage_raycast(cam2vol, Rinv)
    for l, (ov, on) in enumerate(maps):
        _, gv, gn = kf.frame_maps(KFX_FRAME_PREV, l)
        assert feq(gv, ov), f"vmap level {l}"
        assert feq(gn, on), f"nmap level {l}"
    kf.close()


@pytest.fixture(scope="module")
def seq_qvga():
    intr = synth.Intrinsics.qvga()
    return (intr,) + synth.sequence(3, intr, noise=True, dropout=0.01)


def tracked_params(fz):
    vpose, dimz, rangez = FUSED[fz]
    p = default_params(dims=64, range_m=L_VOL)
    p.volu_dims[2] = dimz
    p.volu_range[2] = rangez
    p.volu_pose = Pose.from_matrix(vpose)
    # facez: the second frame tracks against the first frame's measured maps;
    # a third would have only this raycast's few hits to track against
    return p, (2 if fz == "facez" else 3)


@pytest.mark.parametrize("index64", [False, True], ids=["idx32", "idx64"])
@pytest.mark.parametrize("fz", ["cube", "tall", "facez", "facet"])
def test_ray_chain_tracked_stats(fz, index64, seq_qvga):
    """Tracked 320x240 frames against the oracle pipeline, every level bit for
    bit, and the kernel's own counters of the last raycast: blocked lookups
    > 0, and for the face placement (the back wall 1.5 voxels inside the far z
    face) normal_candidates greater than the written hits, i.e. a resume.

    With cubic voxels the resume class stays empty at this size: a hit lies
    between two valid samples (voxel coordinates in (0.5, dim - 1.5)), so its
    six interpolations, half a voxel either way, stay inside the volume unless
    the accumulated sample positions and org + dir * Ts round apart, about
    3e-5 voxels at 64^3 (measured on the cubic face placement: 40255
    candidates, 40255 hits).  The face case therefore uses FUSED["facez"]:
    every ray that meets a surface behind the volume's front half has a NaN
    normal there and marches on.  The oracle alone: 4589 written hits, 72211
    pixels without, where the cubic placement of the same frames writes 40255
    (each of those rays meets its first +/- event either way).  Counters
    measured (idx32 = idx64): facez 59377 candidates for 4589 hits; facet
    60998 for 60908 (90 resumed passes); cube 58729 = 58729, tall 59352 =
    59352."""
    intr, bgr, dep, _ = seq_qvga
    I = Intrinsics.from_any(intr)
    p, frames = tracked_params(fz)
    pipe = O.Pipeline(I, p)
    kf = KinectFusion(I, p)
    if index64:
        kf.debug_force_index64(True)
    for k in range(frames):
        d = dep[k].astype(np.float32)
        assert pipe.process(bgr[k], d) == KFX_OK
        assert kf.pipeline(bgr[k], d) == KFX_OK
    on = pipe.map(1, 2, 0)
    hits = int(((on != 0).any(-1) & ~np.isnan(on).any(-1)).sum())
    for l in range(3):
        _, gv, gn = kf.frame_maps(KFX_FRAME_PREV, l)
        assert feq(gv, pipe.map(1, 1, l)), f"vmap level {l}"
        assert feq(gn, pipe.map(1, 2, l)), f"nmap level {l}"
    st = kf.raycast_stats()
    kf.close()
    print(f"tracked {fz}: oracle hits {hits} stats {st}")
    assert hits >= 200 and on.shape[0] * on.shape[1] - hits >= 200
    assert st["rays"] > 0 and st["blocked_lookups"] > 0 and st["skip_lookups"] > 0, st
    assert st["normal_candidates"] >= hits, st
    if fz in ("facez", "facet"):
        assert st["normal_candidates"] > hits, (st["normal_candidates"], hits)


@pytest.mark.parametrize("fz", ["cube", "face", "tall", "facet"])
def test_ray_chain_slab_group(fz, seq_qvga):
    """The slab kernels' index arithmetic (pre-skip, pass bound, own-range
    exits) and resume state on a 2-slab group of tracked frames against the
    oracle pipeline (320x240: the three-level ICP needs it), every level bit
    for bit; tall is the 128-slice volume, facet the placement whose wall hits
    resume (90 resumed passes on the single volume; the wall lies in the
    second slab's owned slices; facez is left out: its vertices lie tens
    of slices from their samples, outside any slab's halo).

    Members' summed counters measured: blocked lookups 277900 / 263170 /
    271628 / 266421 and normal_candidates 59150 / 41192 / 59640 / 61237 for
    cube / face / tall / facet, against 58729 / 40255 / 59352 / 60908 written
    hits.  The sum exceeds the hits in every placement, since each slab also
    counts its own first event on rays another slab ends earlier: the facet
    assertion below shows a populated class, while that the resumes happen in
    these frames rests on test_ray_chain_tracked_stats[facet-*]."""
    intr, bgr, dep, _ = seq_qvga
    I = Intrinsics.from_any(intr)
    p, frames = tracked_params(fz)
    pipe = O.Pipeline(I, p)
    members = [KinectFusion(I, p, slab=(r, 2)) for r in range(2)]
    for k in range(frames):
        d = dep[k].astype(np.float32)
        assert pipe.process(bgr[k], d) == KFX_OK
        assert pipeline_group(members, bgr[k], d) == KFX_OK
    on = pipe.map(1, 2, 0)
    hit = (on != 0).any(-1) & ~np.isnan(on).any(-1)
    print(f"slab {fz}: oracle hits {int(hit.sum())} without {int((~hit).sum())}")
    assert hit.sum() >= 200 and (~hit).sum() >= 200
    blocked = cands = 0
    for m in members:
        for l in range(3):
            _, gv, gn = m.frame_maps(KFX_FRAME_PREV, l)
            assert feq(gv, pipe.map(1, 1, l)), f"vmap level {l}"
            assert feq(gn, pipe.map(1, 2, l)), f"nmap level {l}"
        st = m.raycast_stats()
        blocked += st["blocked_lookups"]
        cands += st["normal_candidates"]
        m.close()
    print(f"slab {fz}: blocked {blocked} normal_candidates {cands}")
    assert blocked > 0
    if fz == "facet":
        assert cands > hit.sum(), (cands, int(hit.sum()))
