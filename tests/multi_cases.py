"""The multi-start ICP's reference, Python only: the tracker's
coarse-to-fine loop from a start pose, chained from the oracle's two steps, and
the inputs the CPU and GPU tests share: the start family and the noisy QVGA
frame pairs.

loop_from is solve_cases.oracle_loop with a start pose: per (level, iteration)
O.icp_accumulate at the pose so far, then O.icp_update; the first failing
update ends the loop with the pose it was entered with.  What it returns has
the fields of kfx_icp_result, and fields() gives them as kfx.abi.IcpResult's
does: the pose and x as bytes, the rest as integers.

starts(n) is one fixed list, cut to n: the identity; small twists of a few
mrad and a few mm; a start 1 m off (its coarsest sums are zero: lost at
(L - 1, 0)); repeats of the identity and of a twist, set beside the lost start;
FOUND, starts that are lost at a finer level than the coarsest and at a later
iteration than the first; then twists of growing size drawn with SEED, from
well inside the basin to past its edge (a loss there falls on some iteration of
the coarsest level).  FOUND came from a search: 6000 twists drawn with SEED at
six sizes up to (0.3 rad, 0.2 m), each rounded to four decimals, run through
loop_from on the QVGA pair of frame 3; 17 were lost below the coarsest level
(2013 at (2, 0), 1197 at (2, 1..9), 2773 converged) and the four kept are
those whose loops take no Rodrigues step of 0.4 rad or more.  tests/test_multi_cases.py asserts the
outcome on the reference (both statuses, the stop points, every Rodrigues
angle below 0.5, where the device and the oracle share one sincos), so a change
to the scene or the family that loses it is seen there and not as a GPU test
that passes on a batch that is all lost.
"""
import functools
from types import SimpleNamespace

import numpy as np

import icp_cases as K
from kfx.abi import Pose

f32 = np.float32
SEED = 20250607
FAR = 9  # starts(n)[FAR] is the 1 m start; FAR - 1 and FAR + 1 converge (the identity and its repeat)


class Result(SimpleNamespace):
    """pose (Pose), status, stop_level, stop_iter, solves, x (6 doubles); theta_max: the largest Rodrigues
    angle among the solves (not a field of kfx_icp_result)."""

    def fields(self):
        return (bytes(self.pose), int(self.status), int(self.stop_level), int(self.stop_iter), int(self.solves),
                np.ascontiguousarray(self.x, np.float64).tobytes())


def as_pose(p):
    return p if isinstance(p, Pose) else Pose.from_matrix(p)


def loop_from(levels, iters, start, dist, deg):
    """ICPRegistration::rigidTransform's loop over levels[l] (cur_v, cur_n,
    pre_v, pre_n, I; l = the pyramid level) from `start`: levels L-1 .. 0,
    iters[l] iterations each, thresholds dist (m) and deg (degrees)."""
    import oracle as O
    pose, ang = as_pose(start), float(K.sinf_deg(deg))
    solves, x, theta = 0, np.zeros(6), 0.0
    for l in reversed(range(len(levels))):
        L = levels[l]
        for it in range(iters[l]):
            sums = O.icp_accumulate(L.cur_v, L.cur_n, L.pre_v, L.pre_n, L.I, pose, dist, ang)
            st, out, xs = O.icp_update(sums, pose)
            if st:
                return Result(pose=pose, status=1, stop_level=l, stop_iter=it, solves=solves, x=x, theta_max=theta)
            pose, x, solves = out, xs, solves + 1
            theta = max(theta, float(np.linalg.norm(xs[:3].astype(f32).astype(np.float64))))
    return Result(pose=pose, status=0, stop_level=-1, stop_iter=-1, solves=solves, x=x, theta_max=theta)


def twist_matrix(rv, t):
    """exp of the rotation vector rv (Rodrigues, double) with translation t, as float32 4 x 4."""
    rv = np.asarray(rv, float)
    th = np.linalg.norm(rv)
    m = np.eye(4)
    if th > 0:
        k = rv / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        m[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    m[:3, 3] = t
    return m.astype(f32)


# (rotation in rad, translation in m) of the drawn twists, in turn: from inside the basin to its edge and past it
SIZES = ((0.004, 0.004), (0.02, 0.015), (0.05, 0.05), (0.1, 0.05), (0.15, 0.1), (0.2, 0.15))
# (rotation vector, translation, the stop point on the QVGA pair of frame 3)
FOUND = (((0.042, 0.0569, -0.0617), (0.0047, -0.1094, 0.112), (1, 0)),
         ((-0.0098, 0.0028, -0.0193), (-0.1459, -0.0139, 0.0744), (1, 0)),
         ((-0.0169, 0.01, -0.0014), (0.1303, 0.1959, 0.0846), (1, 1)),
         ((-0.2837, -0.0309, 0.0949), (0.0138, 0.0161, -0.0181), (0, 1)))
# draws left out: on the QVGA pair of frame 3 or on small_levels() their loop takes a Rodrigues step of 0.4 rad
# or more (a near-singular solve on a handful of correspondences); from 0.5 rad on the device's sincos is the
# math library's and may differ from the oracle's in the last place
SKIP = frozenset((17, 22, 34, 45, 57, 69, 76, 119))


@functools.lru_cache(maxsize=None)
def _family(n):
    eye = np.eye(4, dtype=f32)
    small = [twist_matrix((0.003, -0.002, 0.001), (0.002, 0.001, -0.003)),
             twist_matrix((-0.001, 0.004, 0.002), (-0.003, 0.002, 0.001)),
             twist_matrix((0.002, 0.001, -0.005), (0.001, -0.004, 0.002)),
             twist_matrix((0.0, 0.0, 0.0), (0.005, 0.0, 0.0)),
             twist_matrix((0.0, 0.006, 0.0), (0.0, 0.0, 0.0))]
    far = twist_matrix((0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    out = [eye] + small + [small[0], small[2], eye, far, eye, small[1]]
    assert np.array_equal(out[FAR], far)
    out += [twist_matrix(rv, t) for rv, t, _ in FOUND]
    rng = np.random.RandomState(SEED)
    k = 0
    while len(out) < n:
        rs, ts = SIZES[k % len(SIZES)]
        m = twist_matrix(rng.uniform(-1, 1, 3) * rs, rng.uniform(-1, 1, 3) * ts)
        if k not in SKIP:
            out.append(m)
        k += 1
    return tuple(out[:n])


def starts(n):
    """The first n of the family, 4 x 4 float32 matrices."""
    return list(_family(n))


def chunk_np(w, h, n):
    """kfx_icp_multi_chunk's rule: poses per block of a batch of n at a w x h level."""
    pb = max(1, ((w // 32) * 32 * ((h // 32) * 32) + 1023) // 1024)
    want = (512 + pb - 1) // pb
    return max(1, min(16, n // want))


def pose_mul_f32(a, b):
    """a * b as 4 x 4 float32 in pose_mul's operation order: each entry a sum of three float32 products
    added left to right from 0, the translation's sum then added to a's."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    out = np.eye(4, dtype=f32)
    for j in range(3):
        for i in range(3):
            v = f32(0)
            for k in range(3):
                v = f32(v + f32(a[j, k] * b[k, i]))
            out[j, i] = v
        d = f32(0)
        for k in range(3):
            d = f32(d + f32(a[j, k] * b[k, 3]))
        out[j, 3] = f32(d + a[j, 3])
    return out


# ---- the noisy QVGA frames ---------------------------------------------------

def level_of(cur_v, cur_n, pre_v, pre_n, I):
    return SimpleNamespace(cur_v=np.ascontiguousarray(cur_v, f32), cur_n=np.ascontiguousarray(cur_n, f32),
                           pre_v=np.ascontiguousarray(pre_v, f32), pre_n=np.ascontiguousarray(pre_n, f32), I=I)


@functools.lru_cache(maxsize=None)
def qvga_pairs():
    """The oracle pipeline over view_cases.scene() (four noisy QVGA frames): per tracked frame k = 1..3 the
    levels (CUR of frame k against PREV as frame k - 1 left it), and the pipeline's poses and parameters."""
    import oracle as O
    import view_cases as VC
    from kfx.abi import Intrinsics
    intr, bgr, dep = VC.scene()
    I, p = Intrinsics.from_any(intr), VC.params(64)
    pipe = O.Pipeline(I, p)
    pairs, prev = [], None
    for k in range(VC.N_FRAMES):
        assert pipe.process(bgr[k], dep[k]) == 0
        if prev is not None:
            pairs.append([level_of(pipe.map(0, 1, l), pipe.map(0, 2, l), prev[l][0], prev[l][1], I.level(l))
                          for l in range(p.pyramid_height)])
        prev = [(pipe.map(1, 1, l).copy(), pipe.map(1, 2, l).copy()) for l in range(p.pyramid_height)]
    return pairs, pipe.poses(), p


def qvga_levels(k=3):
    """The levels of tracked frame k (1..3)."""
    return qvga_pairs()[0][k - 1]


def qvga_iters():
    p = qvga_pairs()[2]
    return tuple(p.icp_iter_count[:p.pyramid_height])


def small_levels():
    """One 80 x 48 level: the top 48 rows of the QVGA pair's level 2 (80 x 60) with that level's intrinsics;
    its floor-covered region (64 x 32) is two pixel blocks."""
    from kfx.abi import Intrinsics
    L = qvga_levels()[2]
    I = Intrinsics(80, 48, L.I.fx, L.I.fy, L.I.cx, L.I.cy)
    return [level_of(L.cur_v[:48], L.cur_n[:48], L.pre_v[:48], L.pre_n[:48], I)]


@functools.lru_cache(maxsize=None)
def qvga_refs(n, k=3):
    """loop_from of starts(n) on the QVGA pair of frame k, computed once."""
    p = qvga_pairs()[2]
    return tuple(loop_from(qvga_levels(k), qvga_iters(), s, p.icp_dist_threshold, p.icp_angle_threshold)
                 for s in starts(n))


@functools.lru_cache(maxsize=None)
def small_refs(n, iters=(4,)):
    p = qvga_pairs()[2]
    return tuple(loop_from(small_levels(), iters, s, p.icp_dist_threshold, p.icp_angle_threshold) for s in starts(n))
