"""Inputs and references of the world view (kfx_world_view), shared by
test_world_view_restatement.py (CPU) and test_gpu_world_view.py.

The reference of a world view is the oracle's raycast on the dense assembly of the bricks: the box
as a dense int16 volume (absent bricks 0), Volume.voxel_size and Volume.range set to the
contract's values (the context's voxel size; the range of kfx.h), the box pose by the shift's
formula (shift_cases.volume_pose), then oracle.render and view_cases' restated vertex and colour
blend with the box's dims.  Everything the GPU is compared with comes from here.

march() restates the march's sample positions and first events in numpy; it is used only to show
that the inputs have the properties they were chosen for, never as a reference."""
import functools

import numpy as np

import oracle as O
import shift_cases as SC
import stream_cases as ST
import view_cases as VC
import world_cases as WC
from kfx import BRICK_DTYPE, synth
from kfx.abi import Intrinsics, Pose, default_params

F = np.float32
KINDS = ("phong", "normal", "color")


# ---- the contract's box --------------------------------------------------------------------

def default_box(bricks):
    """(origin, dims): the list's bounding box in bricks padded by one brick on every side."""
    b = np.asarray(bricks["b"], np.int64)
    lo, hi = b.min(0), b.max(0)
    return tuple(int(8 * (x - 1)) for x in lo), tuple(int(8 * (h - l + 3)) for l, h in zip(lo, hi))


def box_range(p, dims):
    """range_k = volu_range[k] where dims_k == volu_dims[k], else (float)dims_k * vs_k."""
    vs = WC.voxel_size(p)
    return np.array([F(p.volu_range[k]) if int(dims[k]) == int(p.volu_dims[k]) else F(F(int(dims[k])) * vs[k])
                     for k in range(3)], F)


def box_params(p, origin, dims):
    """The context's parameters with the box in place of the window: its pose (the shift's formula
    from the creation pose), dims and range.  view_cases.cam2vol / restate_vertex read the pose."""
    q = SC.copy_params(p)
    q.volu_pose = SC.volume_pose(p, origin)
    rng = box_range(p, dims)
    for k in range(3):
        q.volu_dims[k] = int(dims[k])
        q.volu_range[k] = float(rng[k])
    return q


def assemble(bricks, origin, dims):
    """The box as dense x-fastest arrays: (tsdf (Z*Y*X,) int16, rgb (Z*Y*X, 4) uint8); voxel
    (x, y, z) = world voxel origin + (x, y, z); absent bricks 0; voxels past the box dropped."""
    bricks = np.asarray(bricks, BRICK_DTYPE).ravel()
    assert all(int(o) % 8 == 0 for o in origin)
    nb = [(int(d) + 7) // 8 for d in dims]
    q = np.asarray(bricks["b"], np.int64) - np.array([int(o) // 8 for o in origin])
    inside = ((q >= 0) & (q < np.array(nb))).all(1)
    q, bricks = q[inside], bricks[inside]
    t = np.zeros((nb[2], nb[1], nb[0], 8, 8, 8), np.int16)
    c = np.zeros((nb[2], nb[1], nb[0], 8, 8, 8, 4), np.uint8)
    t[q[:, 2], q[:, 1], q[:, 0]] = bricks["tsdf"].reshape(-1, 8, 8, 8)
    c[q[:, 2], q[:, 1], q[:, 0]] = bricks["rgb"].reshape(-1, 8, 8, 8, 4)
    X, Y, Z = (int(d) for d in dims)
    t = t.transpose(0, 3, 1, 4, 2, 5).reshape(8 * nb[2], 8 * nb[1], 8 * nb[0])[:Z, :Y, :X]
    c = c.transpose(0, 3, 1, 4, 2, 5, 6).reshape(8 * nb[2], 8 * nb[1], 8 * nb[0], 4)[:Z, :Y, :X]
    return np.ascontiguousarray(t).reshape(-1), np.ascontiguousarray(c).reshape(-1, 4)


def filtered(bricks, origin, dims):
    """The bricks of the list that lie in the box."""
    nb = np.array([(int(d) + 7) // 8 for d in dims])
    q = np.asarray(bricks["b"], np.int64) - np.array([int(o) // 8 for o in origin])
    return bricks[((q >= 0) & (q < nb)).all(1)]


def restate_colour(vs, dims, P, hit, rgb, phong):
    """view_cases.restate_colour with the voxel size given (the box's range / dims need not
    reproduce the context's voxel size bit for bit): the colour image of DESIGN.md §18 with "lies
    in the volume" read as "lies in the box".  Pinned to view_cases' on the window box by
    test_world_view_restatement.py."""
    X, Y, Z = (int(d) for d in dims)
    cf = P * (F(1) / np.asarray(vs, F))
    gf = np.floor(cf)
    q = ((cf - gf) * F(256)).astype(np.int64)
    g = gf.astype(np.int64)
    sw = np.zeros(hit.shape, np.int64)
    sc = np.zeros(hit.shape + (3,), np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                x, y, z = g[..., 0] + dx, g[..., 1] + dy, g[..., 2] + dz
                inside = hit & (x >= 0) & (x < X) & (y >= 0) & (y < Y) & (z >= 0) & (z < Z)
                idx = np.where(inside, x + y * X + z * X * Y, 0)
                c = rgb[idx, :3].astype(np.int64)
                counts = inside & (c.any(axis=-1))
                W = np.where(counts, (q[..., 0] if dx else 256 - q[..., 0]) * (q[..., 1] if dy else 256 - q[..., 1]) *
                             (q[..., 2] if dz else 256 - q[..., 2]), 0)
                sw += W
                sc += W[..., None] * c
    assert sw.max() <= 1 << 24
    col = hit & (sw > 0)
    den = np.where(col, sw, 1)
    img = ((sc + (den >> 1)[..., None]) // den[..., None]).astype(np.uint8)
    return np.where(col[..., None], img, np.where(hit[..., None], phong, 0)).astype(np.uint8), col


def reference(p, bricks, intr, pose, box=None):
    """Everything a world view must equal (view_cases.reference's dict, plus the restated vertex P
    in box coordinates, the box and its dense tsdf)."""
    origin, dims = default_box(bricks) if box is None else box
    t, rgb = assemble(bricks, origin, dims)
    pb = box_params(p, origin, dims)
    vs = WC.voxel_size(p)
    vol = O.Volume(dims, [float(r) for r in box_range(p, dims)])
    vol.voxel_size = np.array(vs, F)
    vol.range = box_range(p, dims)
    pose = np.asarray(pose, F)
    c2v, Rinv = VC.cam2vol(pb, pose)
    Z = int(dims[2])
    _, v, n, ts = O.raycast_slab(t, vol, intr, c2v, Rinv, 0, Z, 0, Z)
    eye = pose[:3, 3]
    phong = O.render(v, n, eye, "phong")
    hit = ts != 0
    P, _ = VC.restate_vertex(pb, intr, pose, ts)
    color, col = restate_colour(vs, dims, P, hit, rgb, phong)
    return dict(vmap=v, nmap=n, ts=ts, phong=phong, normal=O.render(v, n, eye, "normal"), color=color, hit=hit,
                coloured=col, P=P, origin=origin, dims=dims, tsdf=t, c2v=c2v)


def assert_view(got, ref, what):
    """got = (image, vmap, nmap, ts) of one kind against the reference, as bytes over whole images."""
    kind, (img, v, n, ts) = got
    assert np.array_equal(ts.view(np.uint32), ref["ts"].view(np.uint32)), (what, kind, "ts")
    assert np.array_equal(v.view(np.uint32), ref["vmap"].view(np.uint32)), (what, kind, "vmap")
    assert np.array_equal(n.view(np.uint32), ref["nmap"].view(np.uint32)), (what, kind, "nmap")
    assert np.array_equal(img, ref[kind]), (what, kind, "image")


# ---- the march, restated for the input properties --------------------------------------------

def march(p, ref, intr, present):
    """The reference's sample loop in numpy float32 on ref's box, up to each ray's first +/-
    candidate.  Returns (cand_len, crossed): cand_len = the loop's ray_len at the candidate (0: the
    ray ends or stops at a -/+ event first), so a hit made of that candidate has Ts in [cand_len -
    step, cand_len) and a later or missing hit means its normal was NaN and the march resumed;
    crossed = a sample before the candidate fell into a cell where `present` ((nbz, nby, nbx) over
    the box's bricks, present_cells) is 0."""
    vs = WC.voxel_size(p)
    dims = np.array(ref["dims"], np.int64)
    rng = box_range(p, ref["dims"])
    c2v = ref["c2v"]
    R, org = np.array(c2v.R[:], F), np.array(c2v.t[:], F)
    H, W = intr.height, intr.width
    x = np.arange(W, dtype=F)[None, :]
    y = np.arange(H, dtype=F)[:, None]
    p0 = np.broadcast_to((F(1) * (x - F(intr.cx))) / F(intr.fx), (H, W))
    p1 = np.broadcast_to((F(1) * (y - F(intr.cy))) / F(intr.fy), (H, W))
    v = [R[3 * i] * p0 + R[3 * i + 1] * p1 + R[3 * i + 2] * F(1) for i in range(3)]
    nrm = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    d = [(v[i] / nrm).astype(F) for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = [F(1) / d[i] for i in range(3)]
        tb = [inv[i] * (F(0) - org[i]) for i in range(3)]
        tt = [inv[i] * (rng[i] - org[i]) for i in range(3)]
    tmin = [np.minimum(tt[i], tb[i]) for i in range(3)]
    tmax = [np.maximum(tt[i], tb[i]) for i in range(3)]
    tnear = np.maximum(np.maximum(tmin[0], tmin[1]), np.maximum(tmin[0], tmin[2]))
    tfar = np.minimum(np.minimum(tmax[0], tmax[1]), np.minimum(tmax[0], tmax[2]))
    ray0 = np.maximum(tnear, F(0))
    step = vs[0]
    ray_len = (ray0 + step).astype(F)
    live = ray0 < tfar
    nextp = [(org[i] + d[i] * ray_len).astype(F) for i in range(3)]
    vstep = [(d[i] * vs[i]).astype(F) for i in range(3)]
    vinv = [F(1) / vs[i] for i in range(3)]
    t = ref["tsdf"].reshape(int(dims[2]), int(dims[1]), int(dims[0]))

    def read(pp):
        g = [np.rint(pp[i] * vinv[i]) for i in range(3)]
        ok = np.ones((H, W), bool)
        for i in range(3):
            ok &= (g[i] >= 1) & (g[i] <= dims[i] - 2)
        gi = [np.where(ok, g[i], 1).astype(np.int64) for i in range(3)]
        val = np.where(ok, t[gi[2], gi[1], gi[0]], 0).astype(np.int64)
        cell = np.where(ok, present[gi[2] >> 3, gi[1] >> 3, gi[0] >> 3], -1)
        return np.sign(val), cell

    sprev, _ = read(nextp)
    cand_len = np.zeros((H, W), F)
    crossed = np.zeros((H, W), bool)
    seen_absent = np.zeros((H, W), bool)
    for _ in range(4 * int(dims.max()) + 8):
        live = live & (ray_len < tfar)
        if not live.any():
            break
        nextp = [(nextp[i] + vstep[i]).astype(F) for i in range(3)]
        s, cell = read(nextp)
        hit = live & (sprev > 0) & (s < 0)
        stop = live & (sprev < 0) & (s > 0)
        cand_len = np.where(hit, ray_len, cand_len)
        crossed |= hit & seen_absent
        seen_absent |= live & (cell == 0)
        live = live & ~hit & ~stop
        sprev = s
        ray_len = (ray_len + step).astype(F)
    return cand_len, crossed


def present_cells(ref, bricks):
    """march()'s `present` for a list on ref's box: 1 where the list has the brick, 0 where it has
    none inside the list's own bounding box, -1 in the padding around it."""
    nb = [(int(d) + 7) // 8 for d in ref["dims"]]
    q = np.asarray(bricks["b"], np.int64) - np.array([int(o) // 8 for o in ref["origin"]])
    out = np.full((nb[2], nb[1], nb[0]), -1, np.int64)
    lo, hi = q.min(0), q.max(0)
    out[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = 0
    out[q[:, 2], q[:, 1], q[:, 0]] = 1
    return out


# ---- 1. the window ---------------------------------------------------------------------------

def fused_bricks(dims=64):
    """view_cases.fused(dims) as the world_bricks() of a context that holds it: the non-empty
    bricks of the window at origin 0."""
    t, w, c, _ = VC.fused(dims)
    d = (dims,) * 3
    ne = ST.nonempty_bricks(t, w, c.reshape(-1), d)
    return WC.bricks_of(t, w, c[:, :3], d, ne)


def fused_records(dims=64):
    """The same volume as the 8-byte records upload_tsdf takes."""
    import extract_cases as EC
    t, w, c, _ = VC.fused(dims)
    return EC.records(t, w, c[:, :3])


# ---- 2. the sparse world ---------------------------------------------------------------------

SPARSE_BOX = (40, 32, 24)  # 5 x 4 x 3 bricks
SPARSE_BASES = ((0, 0, 0), (-2, 1, -3))
# voxel sizes and creation pose whose products with brick coordinates are exact in float32 (dyadic
# values, a quarter turn about z): moving list and camera by whole bricks then leaves cam2vol, and
# with it every sample, bit for bit the same.  Three different voxel sizes; R0 is not the identity.
SPARSE_VS = (1 / 32, 3 / 128, 3 / 64)


def sparse_params():
    p = default_params(dims=32, range_m=1.0)
    for k, d in enumerate((32, 24, 16)):
        p.volu_dims[k] = d
        p.volu_range[k] = d * SPARSE_VS[k]
    m = np.eye(4)
    m[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    m[:3, 3] = [-0.5, 0.25, 0.125]
    p.volu_pose = Pose.from_matrix(m)
    assert np.array_equal(WC.voxel_size(p), np.array(SPARSE_VS, F))
    return p


@functools.lru_cache(maxsize=None)
def sparse_scene():
    """A tilted plane with a sphere in front of it on SPARSE_BOX: the signed distance in voxels
    (positive towards low z, where the cameras stand), truncated at 3 voxels, as int16; every
    voxel observed; colours varying by voxel.  Returns (keep, t, w, rgb): four bricks the surface
    crosses and three it does not (all positive, in front of it) are taken out."""
    X, Y, Z = SPARSE_BOX
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    nrm = np.array([0.2, 0.3, 0.93])
    nrm /= np.linalg.norm(nrm)
    plane = -((x - 20) * nrm[0] + (y - 16) * nrm[1] + (z - 17) * nrm[2])
    sphere = np.sqrt((x - 27.0) ** 2 + (y - 13.0) ** 2 + (z - 9.0) ** 2) - 5.5
    sdf = np.minimum(plane, sphere)
    t = np.clip(np.rint(np.clip(sdf / 3.0, -1, 1) * 32767), -32767, 32767).astype(np.int16).ravel()
    w = np.ones(X * Y * Z, np.int16)
    rgb = np.stack([(7 * x + 3 * y + 40) % 256, (11 * y + 5 * z + 90) % 256, (13 * z + 2 * x + 17) % 256], -1)
    rgb = rgb.reshape(-1, 3).astype(np.uint8)
    tb = ST.to_bricks(t, SPARSE_BOX)[:, :, 0]
    crossing = np.nonzero((tb < 0).any(1) & (tb > 0).any(1))[0]
    clear = np.nonzero((tb > 0).all(1))[0]
    keep = np.ones(len(tb), bool)
    keep[crossing[[1, 5, 9, 13]]] = False
    keep[clear[[0, 3, 7]]] = False
    t, w, rgb = WC.zero_absent(t, w, rgb, SPARSE_BOX, keep)
    for a in (keep, t, w, rgb):
        a.setflags(write=False)
    return keep, t, w, rgb, tuple(int(i) for i in crossing[[1, 5, 9, 13]]), tuple(int(i) for i in clear[[0, 3, 7]])


def sparse_bricks(base):
    keep, t, w, rgb = sparse_scene()[:4]
    return WC.bricks_of(t, w, rgb, SPARSE_BOX, keep, base)


def _look(eye, at, up=(0.0, -1.0, 0.0)):
    """Camera-to-frame 4x4 with +z from eye to at (float32 entries)."""
    eye, at = np.array(eye, np.float64), np.array(at, np.float64)
    f = at - eye
    f /= np.linalg.norm(f)
    r = np.cross(np.array(up, np.float64), f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2] = r, u, f
    m[:3, 3] = eye
    return m.astype(F).astype(np.float64)


def _snap(v, bits=10):
    """Positions on a 2^-bits grid: sums with the box's dyadic translation stay exact."""
    return np.round(np.array(v, np.float64) * (1 << bits)) / (1 << bits)


def local_metric(vox, vs=SPARSE_VS):
    return _snap([vox[k] * vs[k] for k in range(3)])


def sparse_views(base):
    """[(name, Intrinsics, camera-to-world pose)] for the list at brick base `base`: the camera is
    given in the list's own frame (metres from world voxel 8 base) and moved with it."""
    p = sparse_params()
    frame = SC.volume_pose(p, tuple(8 * b for b in base)).matrix().astype(np.float64)
    q = synth.Intrinsics.qvga()

    def intr(W, H, s):
        return Intrinsics(W, H, float(F(q.fx * s)), float(F(q.fy * s * 1.02)), float(F(W / 2 - 0.5 + 3.25)),
                          float(F(H / 2 - 0.5 - 1.5)))

    cams = [
        ("odd", intr(97, 61, 0.45), _look(local_metric((22, 14, -40)), local_metric((20, 16, 14)))),
        ("off", intr(200, 152, 1.0), _look(local_metric((-25, 2, -30)), local_metric((22, 16, 14)))),
        # along the seam x = 16 (bricks 1 | 2), grazing the plane
        ("graze", intr(160, 120, 0.45), _look(local_metric((16, -40, 6)), local_metric((16, 20, 14)), up=(0, 0, -1))),
        # inside the box, between the sphere and the plane's near side
        ("inside", intr(128, 96, 0.3), _look(local_metric((12, 12, 4)), local_metric((27, 14, 12)))),
    ]
    out = []
    for name, i, local in cams:
        m = frame @ local
        assert np.array_equal(m.astype(F).astype(np.float64), m), name  # exact in float32
        out.append((name, i, m.astype(F)))
    return out


@functools.lru_cache(maxsize=None)
def sparse_refs(base):
    p = sparse_params()
    b = sparse_bricks(base)
    return [(name, i, pose, reference(p, b, i, pose)) for name, i, pose in sparse_views(base)]


# ---- 3. far-apart clusters -------------------------------------------------------------------

CLUSTER_GAP = 20  # absent bricks between the clusters along x


def cluster_params():
    """Cubic voxels of 1 / 32 m (the sparse world has three sizes), a shifted creation pose."""
    p = default_params(dims=32, range_m=1.0)
    m = np.eye(4)
    m[:3, 3] = [-0.75, -0.25, 0.5]
    p.volu_pose = Pose.from_matrix(m)
    return p


@functools.lru_cache(maxsize=None)
def cluster_bricks():
    """Two 2 x 2 x 2-brick clusters, each a sphere of radius 5 voxels in its middle, 20 bricks
    apart along x: bricks x = 0, 1 and 22, 23 at base (3, -2, 1)."""
    z, y, x = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    out = []
    for k, (cx, cy, cz, r) in enumerate(((7.5, 8.0, 7.0, 5.0), (8.0, 7.0, 8.5, 5.5))):
        sdf = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r
        t = np.clip(np.rint(np.clip(sdf / 3.0, -1, 1) * 32767), -32767, 32767).astype(np.int16).ravel()
        rgb = np.stack([(9 * x + 60 + 100 * k) % 256, (5 * y + 3 * z + 30) % 256, (7 * z + 120) % 256], -1)
        b = WC.bricks_of(t, np.ones(16 ** 3, np.int16), rgb.reshape(-1, 3).astype(np.uint8), (16, 16, 16),
                         np.ones(8, bool), (3 + (CLUSTER_GAP + 2) * k, -2, 1))
        out.append(b)
    b = np.concatenate(out)
    b = b[np.lexsort((b["b"][:, 0], b["b"][:, 1], b["b"][:, 2]))]
    b.setflags(write=False)
    return b


def cluster_views():
    p = cluster_params()
    frame = SC.volume_pose(p, (24, -16, 8)).matrix().astype(np.float64)
    q = synth.Intrinsics.qvga()
    mid = 8 * (CLUSTER_GAP + 2) + 8
    cams = [
        # along x, a little off the axis so that rays pass the first sphere and reach the second
        ("along", Intrinsics(160, 120, float(F(q.fx * 1.1)), float(F(q.fy * 1.1)), 79.5, 59.5),
         _look(local_metric((-60, 20.0, 9.0), (1 / 32,) * 3), local_metric((mid, 7.5, 8.0), (1 / 32,) * 3))),
        ("oblique", Intrinsics(200, 150, float(F(q.fx * 0.45)), float(F(q.fy * 0.45)), 99.5, 74.5),
         _look(local_metric((60, -90, -70), (1 / 32,) * 3), local_metric((mid / 2 + 8, 8, 8), (1 / 32,) * 3))),
    ]
    return [(name, i, (frame @ m).astype(F)) for name, i, m in cams]


@functools.lru_cache(maxsize=None)
def cluster_refs():
    p = cluster_params()
    return [(name, i, pose, reference(p, cluster_bricks(), i, pose)) for name, i, pose in cluster_views()]


# ---- 4. the excursion ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def excursion_world():
    """stream_cases.excursion_reference's end state as (params, world bricks, window bricks):
    the window merged with what the store still holds (test_gpu_world.test_excursion_world)."""
    sp, _ = ST.excursion_reference()
    dims = (64, 64, 64)
    win = ST.evict_bricks_ref(*sp.volume(), dims, sp.origin, (64, 0, 0))
    both = {tuple(int(x) for x in b["b"][::-1]): b for b in sp.store.values()}
    both.update({tuple(int(x) for x in b["b"][::-1]): b for b in win})
    world = np.array([both[k] for k in sorted(both)], BRICK_DTYPE)
    return SC.params(64), world, win


def excursion_views():
    sp, _ = ST.excursion_reference()
    first = sp.pose_matrices()[0].astype(F)
    q = Intrinsics.from_any(SC.qvga())
    off_i, off_p = VC.make_view((200, 152, 0.55, 0.5, -0.1, 0.35), first)  # turned towards the wall that left
    return [("first", q, first), ("off", off_i, off_p)]


@functools.lru_cache(maxsize=None)
def excursion_refs():
    p, world, _ = excursion_world()
    return [(name, i, pose, reference(p, world, i, pose)) for name, i, pose in excursion_views()]
