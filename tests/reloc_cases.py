"""Relocalisation restated, numpy and Python only: splitmix64
and the fern table, the frame code, brute-force distances and the match order,
kfx_relocalise's selection rule with Python integers, the blob parser, and the
retrieval family the CPU and GPU tests share."""
import functools
import struct

import numpy as np

from kfx.abi import FERN_DTYPE

M64 = (1 << 64) - 1
DEFAULT = dict(m=512, seed=2013, depth_mm=(400, 4000))
BLOB_MAGIC, BLOB_VERSION = 0x4B58464B, 1


class SplitMix64:
    def __init__(self, seed):
        self.state = seed & M64

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)


def grid(width, height, L):
    """(wL, hL, s) of the fern grid: pyramid level L - 1."""
    return width >> (L - 1), height >> (L - 1), 1 << (L - 1)


def table(width, height, L, m=512, seed=2013, depth_mm=(400, 4000)):
    wL, hL, _ = grid(width, height, L)
    r, t = SplitMix64(seed), np.zeros(m, FERN_DTYPE)
    for f in range(m):
        t[f]["x"] = r.next() % wL
        t[f]["y"] = r.next() % hL
        t[f]["tb"], t[f]["tg"], t[f]["tr"] = r.next() % 256, r.next() % 256, r.next() % 256
        mm = depth_mm[0] + r.next() % (depth_mm[1] - depth_mm[0] + 1)
        t[f]["td"] = np.float32(mm) / np.float32(1000.0)
    return t


def nibbles(bgr, dmap, tab, s):
    """The nibble of every fern: bgr (H, W, 3) uint8, dmap (hL, wL) float32 metres."""
    bgr = np.asarray(bgr, np.uint8)
    H, W, _ = bgr.shape
    blocks = bgr.reshape(H // s, s, W // s, s, 3).astype(np.int64).sum(axis=(1, 3))  # (hL, wL, 3) integer sums
    x, y = tab["x"].astype(np.int64), tab["y"].astype(np.int64)
    sums = blocks[y, x]
    thr = np.stack([tab["tb"], tab["tg"], tab["tr"]], axis=1).astype(np.int64) * (s * s)
    bits = (sums > thr).astype(np.uint8)
    d = np.asarray(dmap, np.float32)[y, x]
    return bits[:, 0] | (bits[:, 1] << 1) | (bits[:, 2] << 2) | ((d > tab["td"]).astype(np.uint8) << 3)


def pack(nib):
    nib = np.asarray(nib, np.uint64).reshape(-1, 16)
    sh = (np.arange(16, dtype=np.uint64) * np.uint64(4))
    return np.bitwise_or.reduce(nib << sh, axis=1)


def unpack(code):
    code = np.asarray(code, np.uint64).reshape(-1, 1)
    sh = (np.arange(16, dtype=np.uint64) * np.uint64(4))
    return ((code >> sh) & np.uint64(15)).astype(np.uint8).reshape(-1)


def encode(bgr, dmap, tab, s):
    return pack(nibbles(bgr, dmap, tab, s))


def distances(queries, codes):
    """(q, n) int: ferns whose nibbles differ, by unpacking (no bit tricks)."""
    queries = np.asarray(queries, np.uint64).reshape(len(queries), -1)
    out = np.zeros((len(queries), len(codes)), np.int64)
    if len(codes) == 0:
        return out
    codes = np.asarray(codes, np.uint64).reshape(len(codes), -1)
    cn = np.stack([unpack(c) for c in codes])
    for i, qc in enumerate(queries):
        out[i] = (cn != unpack(qc)[None, :]).sum(axis=1)
    return out


def search(queries, codes, k):
    """(q, k, 2) int32 of (id, distance), ascending (distance, id), -1 in unused slots."""
    d = distances(queries, codes)
    out = np.full((len(d), k, 2), -1, np.int32)
    for i, row in enumerate(d):
        order = sorted(range(len(row)), key=lambda j: (int(row[j]), j))[:k]
        for s, j in enumerate(order):
            out[i, s] = (j, row[j])
    return out


def better(a, b):
    """a beats b; a candidate is (n0, den, sum_r2, match, start) in Python integers."""
    if a[1] == 0 or b[1] == 0:
        if a[1] != 0:
            return True
        if b[1] != 0:
            return False
    else:
        l, r = a[0] * b[1], b[0] * a[1]
        if l != r:
            return l > r
        ea, eb = a[2] * b[0], b[2] * a[0]
        if ea != eb:
            return ea < eb
    return (a[3], a[4]) < (b[3], b[4])


def candidate(q, match, start):
    n = [int(v) for v in q.n]
    return (n[0], n[0] + n[2] + n[3] + n[4], int(q.sum_r2), match, start)


def select(cands):
    """Index of the winner, -1 when there is none."""
    best = -1
    for i, c in enumerate(cands):
        if best < 0 or better(c, cands[best]):
            best = i
    return best


def fitness(c):
    return c[0] / float(c[1]) if c[1] else 0.0


def blob_parse(blob):
    """dict(m, wL, hL, s, depth_mm, seed, table, poses (n, 12) float32, codes (n, m / 16) uint64)."""
    magic, version, m, wL, hL, s, dmin, dmax, seed, n = struct.unpack_from("<IIiiiiIIQq", blob, 0)
    assert magic == BLOB_MAGIC and version == BLOB_VERSION
    o = 48
    assert len(blob) == o + 16 * m + 48 * n + 8 * (m // 16) * n
    tab = np.frombuffer(blob, FERN_DTYPE, m, o)
    o += 16 * m
    poses = np.frombuffer(blob, np.float32, 12 * n, o).reshape(n, 12)
    o += 48 * n
    codes = np.frombuffer(blob, np.uint64, (m // 16) * n, o).reshape(n, m // 16)
    return dict(m=m, wL=wL, hL=hL, s=s, depth_mm=(dmin, dmax), seed=seed, table=tab, poses=poses, codes=codes)


# ---- the retrieval family ------------------------------------------------------
HARVEST_MIN_DISTANCE = 51


def params():
    from kfx.abi import default_params
    return default_params(dims=64, range_m=2.048)


@functools.lru_cache(maxsize=None)
def family(n_keyframes=30):
    """Keyframes every 4th pose of a 120-pose trajectory, queries two steps after each, and a same-pose revisit
    of every keyframe with other noise: dict(key, query, revisit) of (bgr, depth_mm, dmap at level L - 1, code)."""
    import oracle as O
    from kfx import synth
    from kfx.abi import Intrinsics
    intr = synth.Intrinsics.qvga()
    I, p = Intrinsics.from_any(intr), params()
    scene = synth.Scene.default()
    poses = synth.trajectory(120, seed=7, amp_t=0.25, amp_r_deg=15)
    tab = table(intr.width, intr.height, p.pyramid_height)
    s = 1 << (p.pyramid_height - 1)

    def frame(pose, seed):
        bgr, dep = synth.render(scene, intr, pose, noise_seed=seed, dropout=0.01)[:2]
        return bgr, dep.astype(np.float32)

    def coded(pose, seed):
        bgr, dep = frame(pose, seed)
        dmap = coarse_dmap(O, dep, I, p)
        return bgr, dep, dmap, encode(bgr, dmap, tab, s)

    key = [coded(poses[4 * k], 42 + k) for k in range(n_keyframes)]
    query = [coded(poses[4 * k + 2], 5000 + k) for k in range(min(n_keyframes, 29))]
    revisit = [coded(poses[4 * k], 9000 + k) for k in range(n_keyframes)]
    return dict(key=key, query=query, revisit=revisit, table=tab, s=s)


def coarse_dmap(O, depth_mm, I, p):
    """The oracle's filtered depth map of level L - 1, metres."""
    out = O.preprocess(depth_mm, I, p)
    return np.asarray(out[0][p.pyramid_height - 1], np.float32)
