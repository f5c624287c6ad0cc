"""The ICP residual map and quality record restated in numpy,
on top of icp_cases.accumulate_np (which already labels every pixel of the
floor-covered region and keeps the 7-entry row): the full-size label image
(5 outside the region), the residual image, the record's fields and the two
derived figures.  It shares no code with the kernels or the oracle."""
import math
from types import SimpleNamespace

import numpy as np

import icp_cases as K

f32 = np.float32
UNCOVERED = 5
SIZES_1PX = [(32, 32), (80, 48), (96, 32)]
sid = lambda s: f"{s[0]}x{s[1]}"


def quality_np(cur_v, cur_n, pre_v, pre_n, I, pose, dist, angle, level=0):
    """label (h, w) uint8, residual (h, w) float32, n (6 ints), sum_r2 (int),
    max_abs_r (float32), record = the fields as kfx.abi.IcpQuality.fields() gives them."""
    r = K.accumulate_np(cur_v, cur_n, pre_v, pre_n, I, pose, dist, angle)
    h, w = I.height, I.width
    ye, xe = r.label.shape
    label = np.full((h, w), UNCOVERED, np.uint8)
    label[:ye, :xe] = r.label.astype(np.uint8)
    residual = np.zeros((h, w), f32)
    res = np.where(r.accepted, r.row[..., 6], f32(0)).astype(f32)
    residual[:ye, :xe] = res
    acc = res[r.accepted]
    with np.errstate(all="ignore"):
        sq = (acc * acc) * K.FIX
    assert sq.dtype == f32 and np.all(np.isfinite(sq)) and np.all(sq < f32(2.0 ** 62))
    sum_r2 = sum(int(v) for v in np.rint(sq).astype(np.int64))
    max_abs = f32(np.abs(acc).max()) if acc.size else f32(0)
    n = [int((label == k).sum()) for k in range(6)]
    assert sum(n) == w * h
    return SimpleNamespace(label=label, residual=residual, n=n, sum_r2=sum_r2, max_abs_r=max_abs,
                           record=tuple(n) + (sum_r2, float(max_abs), level))


def figures_np(n, sum_r2):
    """(fitness, rmse) in double, in the order include/kfx.h states."""
    den = n[0] + n[2] + n[3] + n[4]
    fitness = float(n[0]) / float(den) if den else 0.0
    rmse = math.sqrt((float(sum_r2) / 4294967296.0) / float(n[0])) if n[0] else 0.0
    return fitness, rmse


def chunk_np(w, h, n):
    """kfx_quality_chunk's rule: poses per block of a batch of n."""
    pb = max(1, (w * h + 1023) // 1024)
    want = (512 + pb - 1) // pb
    return max(1, min(16, n // want))


_cache = {}


def crafted_ref(name, w, h, moved):
    """quality_np of a crafted case under the identity or the moved pose, computed once."""
    key = (name, w, h, moved)
    if key not in _cache:
        case, dist, deg = K.crafted(name, w, h)
        pose = K.moved_pose() if moved else K.Pose.identity()
        _cache[key] = quality_np(case.cur_v, case.cur_n, case.pre_v, case.pre_n, case.I, pose, dist, K.sinf_deg(deg))
    return _cache[key]


def pose_family(n):
    """The identity, the moved pose, then a fixed arithmetic family of small
    rotations and translations; poses repeat with period 40 from the third on."""
    out = [np.eye(4, dtype=f32), K.moved_pose().matrix()]
    for k in range(max(n - 2, 0)):
        q = k % 40
        a, b = 1e-4 * (q % 7 - 3), 2e-4 * (q % 5 - 2)
        m = np.eye(4)
        m[:3, :3] = [[1, -a, b], [a, 1, -a * b], [-b, a * b, 1]]
        m[:3, 3] = [1e-4 * (q % 3 - 1), -5e-5 * (q % 4), 2e-4 * (q % 6 - 2)]
        out.append(m.astype(f32))
    return out[:n]
