"""References of the bricks that leave and re-enter the moving volume, shared by
test_stream_restatement.py (CPU) and test_gpu_stream.py: kfx_evict_bricks and kfx_restore_bricks
restated in numpy on x-fastest SoA arrays, a volume with empty bricks, and StagePipeline with a
shift that loses nothing."""
import functools

import numpy as np

import integrate_cases as IC
import shift_cases as SC
from kfx import BRICK_DTYPE

EXCURSION = (8, 0, 0)      # out before frame 4, back before frame 8: the left wall leaves and returns
FREE_EXCURSION = (0, 0, 8)  # drops free space only (no negative tsdf)


def shift_table(dims):
    """test_gpu_shift.shift_table, restated (that module is marked gpu as a whole)."""
    X, Y, Z = dims
    one = [tuple(sg * m if k == a else 0 for k in range(3)) for a in range(3) for m in (8, 16) for sg in (1, -1)]
    # a depth that is no multiple of 8: along z, shifts that leave part of a brick group (the +-8 above too)
    part = [(0, 0, 40), (0, 0, -40), (8, 0, -40)] if Z % 8 else []
    return one + part + [(8, -16, 24), (-8, -8, -8), (X, 0, 0), (0, -Y, 0), (0, 0, (Z + 7) // 8 * 8 + 8),
                         (-X - 16, 8, 0), (0, 0, 0)]


def brick_counts(dims):
    return tuple((int(d) + 7) // 8 for d in dims)


def to_bricks(a, dims, per=1):
    """(Z*Y*X*per,) x-fastest -> (bricks, 512, per): bricks ascending (bz, by, bx), a brick's
    voxels in the device order 64*dz + 8*dy + dx; slices past Z are 0."""
    X, Y, Z = (int(d) for d in dims)
    nx, ny, nz = brick_counts(dims)
    assert X == 8 * nx and Y == 8 * ny
    g = np.zeros((8 * nz, Y, X, per), np.asarray(a).dtype)
    g[:Z] = np.asarray(a).reshape(Z, Y, X, per)
    g = g.reshape(nz, 8, ny, 8, nx, 8, per).transpose(0, 2, 4, 1, 3, 5, 6)
    return g.reshape(nz * ny * nx, 512, per)


def from_bricks(b, dims, per=1):
    """The inverse of to_bricks (slices past Z dropped)."""
    X, Y, Z = (int(d) for d in dims)
    nx, ny, nz = brick_counts(dims)
    g = np.asarray(b).reshape(nz, ny, nx, 8, 8, 8, per).transpose(0, 3, 1, 4, 2, 5, 6)
    return np.ascontiguousarray(g.reshape(8 * nz, Y, X, per)[:Z]).reshape(-1)


def brick_coords(dims):
    """(bricks, 3) window indices (cx, cy, cz) in to_bricks' order."""
    nx, ny, nz = brick_counts(dims)
    cz, cy, cx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([cx.ravel(), cy.ravel(), cz.ravel()], 1)


def dropped_bricks(dims, s):
    """(bricks,) bool: the bricks with a voxel that shift s does not keep."""
    lv = SC.leaving(tuple(int(d) for d in dims), s)
    return to_bricks(lv, dims).reshape(-1, 512).any(1)


def nonempty_bricks(t, w, c, dims):
    return (to_bricks(t, dims).reshape(-1, 512).any(1) | to_bricks(w, dims).reshape(-1, 512).any(1) |
            to_bricks(c, dims, 4).reshape(-1, 2048).any(1))


def evict_bricks_ref(t, w, c, dims, origin, s):
    """kfx_evict_bricks: the non-empty bricks with a voxel shift s drops, (N,) BRICK_DTYPE
    ascending (b[2], b[1], b[0])."""
    assert all(int(o) % 8 == 0 for o in origin)
    sel = dropped_bricks(dims, s) & nonempty_bricks(t, w, c, dims)
    out = np.zeros(int(sel.sum()), BRICK_DTYPE)
    out["b"] = brick_coords(dims)[sel] + np.array([int(o) // 8 for o in origin])
    out["tsdf"] = to_bricks(t, dims)[sel, :, 0]
    wb = to_bricks(w, dims)[sel, :, 0]
    assert wb.min(initial=0) >= 0 and wb.max(initial=0) <= 255
    out["weight"] = wb
    out["rgb"] = to_bricks(c, dims, 4)[sel]
    return out


def restore_ref(t, w, c, dims, origin, bricks):
    """kfx_restore_bricks: the bricks whose coordinate lies in the window written whole over the
    arrays.  Returns ((t, w, c), count)."""
    nx, ny, nz = brick_counts(dims)
    tb, wb, cb = to_bricks(t, dims).copy(), to_bricks(w, dims).copy(), to_bricks(c, dims, 4).copy()
    n = 0
    for br in np.asarray(bricks, BRICK_DTYPE).ravel():
        q = [int(br["b"][k]) - int(origin[k]) // 8 for k in range(3)]
        if not (0 <= q[0] < nx and 0 <= q[1] < ny and 0 <= q[2] < nz):
            continue
        i = (q[2] * ny + q[1]) * nx + q[0]
        tb[i, :, 0], wb[i, :, 0], cb[i] = br["tsdf"], br["weight"], br["rgb"]
        n += 1
    return (from_bricks(tb, dims), from_bricks(wb, dims), from_bricks(cb, dims, 4)), n


@functools.lru_cache(maxsize=None)
def sparse_volume(dims, seed=11):
    """integrate_cases.random_volume with about half of the bricks zeroed by a seeded brick mask
    (random_volume alone has no empty brick, so it cannot test the compaction), and three of the
    zeroed bricks non-empty through a single stored value only: one colour byte at brick (0, 0,
    0), one positive tsdf at the last brick of every axis, one weight at brick (0, last, 0).
    Every face slab of the volume holds one of them."""
    t, w, c = (np.array(a) for a in IC.random_volume(tuple(dims)))
    nx, ny, nz = brick_counts(dims)
    rng = np.random.default_rng(seed)
    keep = rng.integers(0, 2, nz * ny * nx).astype(bool)
    special = [0, (nz * ny * nx) - 1, (ny - 1) * nx]
    keep[special] = False
    tb, wb, cb = to_bricks(t, dims), to_bricks(w, dims), to_bricks(c, dims, 4)
    tb[~keep], wb[~keep], cb[~keep] = 0, 0, 0
    at = 64 * 2 + 8 * 5 + 3  # (dx, dy, dz) = (3, 5, 2): inside a short last group too
    cb[special[0], at, 1] = 200
    tb[special[1], at, 0] = 12345
    wb[special[2], at, 0] = 7
    out = (from_bricks(tb, dims), from_bricks(wb, dims), from_bricks(cb, dims, 4))
    ne = nonempty_bricks(*out, dims)
    assert ne[special].all() and 0.3 < ne.mean() < 0.7
    for a in out:
        a.setflags(write=False)
    return out


class StreamPipeline(SC.StagePipeline):
    """StagePipeline whose shift loses nothing: the bricks a shift drops go into a dict keyed by
    their world coordinate (a coordinate already held is replaced), and the bricks of the new
    window come back out of it."""

    def __init__(self, intr, p):
        super().__init__(intr, p)
        self.store = {}
        self.n_out = self.n_in = 0

    def shift(self, s):
        ev = evict_bricks_ref(*self.volume(), self.dims, self.origin, s)
        for br in ev:
            self.store[tuple(int(x) for x in br["b"])] = br.copy()
        self.n_out += len(ev)
        super().shift(s)
        nb = brick_counts(self.dims)
        lo = [self.origin[k] // 8 for k in range(3)]
        keys = sorted((k for k in self.store if all(lo[a] <= k[a] < lo[a] + nb[a] for a in range(3))),
                      key=lambda k: (k[2], k[1], k[0]))
        if keys:
            back = np.array([self.store.pop(k) for k in keys], BRICK_DTYPE)
            vol, n = restore_ref(*self.volume(), self.dims, self.origin, back)
            assert n == len(keys)
            self.set_volume(*vol)
            self.n_in += n


@functools.lru_cache(maxsize=None)
def excursion_reference(s=EXCURSION, stream=True):
    """The 12 frames of shift_cases.frames on 64^3 with shift s before frame 4 and -s before frame
    8, every frame tracked (a condition on the inputs).  stream: StreamPipeline, else the lossy
    StagePipeline.  Returns (pipe, level-0 model map after frame 8)."""
    bgr, dep, _ = SC.frames(12)
    sp = (StreamPipeline if stream else SC.StagePipeline)(SC.qvga(), SC.params(64))
    pv8 = None
    for k in range(12):
        if k == 4:
            sp.shift(s)
        if k == 8:
            sp.shift(tuple(-x for x in s))
        assert sp.process(bgr[k], dep[k]) == 0, f"frame {k} lost in the reference"
        if k == 8:
            pv8 = sp.pv[0].copy()
    return sp, pv8
