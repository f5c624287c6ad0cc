"""The multi-start ICP's reference and inputs, without a GPU:
multi_cases.loop_from against solve_cases.oracle_loop on the crafted loop cases
and against the oracle pipeline's own poses on the noisy QVGA frames; the
conditions the start family has to meet on the reference alone, so that no GPU
test can pass on a batch that is all lost (or all converged); the chunk rule of
the library against its restatement; the record's size; and the host-only
arithmetic (csrc/kfx_multi.h) as a stand-alone program, plain and under
ASan + UBSan.  tests/test_gpu_icp_multi.py holds the device to loop_from."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import multi_cases as M
import solve_cases as S
from kfx.abi import IcpResult, Pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOPS = ["iters_203", "iters_000", "chain", "fail_middle", "fail_second_iteration"]
SIZES = [(32, 32), (80, 48), (80, 60), (96, 32), (160, 120), (320, 240), (640, 480), (1280, 720), (2048, 2048)]
COUNTS = [1, 2, 3, 7, 8, 15, 16, 17, 20, 21, 127, 128, 129, 130, 255, 256, 257, 600, 4096, 65536]


@pytest.mark.parametrize("name", LOOPS)
def test_loop_from_identity_is_oracle_loop(oracle_lib, name):
    c = S.case(name)
    its, status, pose = S.oracle_loop(c)
    r = M.loop_from(c.levels, c.iters, Pose.identity(), c.dist, c.deg)
    solved = [i for i in its if i.status == 0]
    assert r.status == status and bytes(r.pose) == bytes(pose) and r.solves == len(solved)
    assert (r.stop_level, r.stop_iter) == ((its[-1].level, its[-1].it) if status else (-1, -1))
    assert (r.stop_level, r.stop_iter) == (c.stop if c.__dict__.get("stop") else (-1, -1))
    want_x = solved[-1].x if solved else np.zeros(6)
    assert np.array_equal(np.asarray(r.x).view(np.uint64), np.asarray(want_x, np.float64).view(np.uint64))
    assert r.theta_max < 0.5  # the device shares the oracle's sincos there


def test_loop_from_identity_is_the_pipelines_pose(oracle_lib):
    import oracle as O
    pairs, poses, p = M.qvga_pairs()
    assert len(pairs) == 3 and len(poses) == 4
    for k in (1, 2, 3):
        r = M.loop_from(M.qvga_levels(k), M.qvga_iters(), Pose.identity(), p.icp_dist_threshold, p.icp_angle_threshold)
        assert r.status == 0 and r.solves == sum(M.qvga_iters()) == 19 and (r.stop_level, r.stop_iter) == (-1, -1)
        world = O.pose_mul(Pose.from_matrix(poses[k - 1]), r.pose).matrix()
        assert np.array_equal(world.view(np.uint32), poses[k].astype(np.float32).view(np.uint32)), k
        assert np.array_equal(world, M.pose_mul_f32(poses[k - 1], r.pose.matrix()))  # the float32 composition restated


def test_start_family_on_the_reference(oracle_lib):
    """Conditions on the inputs: over the family at QVGA both statuses occur, the losses fall on at least three
    (level, iteration) points, one at a later iteration and one at a finer level than (L - 1, 0), at least a
    quarter of the starts converge and at least a tenth are lost, repeats are repeats, a lost start has
    converging neighbours, and no loop takes a Rodrigues step of 0.5 rad or more."""
    n = 130
    st = M.starts(n)
    assert len(st) == n and all(np.array_equal(a, b) for a, b in zip(M.starts(21), st))
    assert np.array_equal(st[0], np.eye(4)) and np.array_equal(st[0], st[8]) and np.array_equal(st[1], st[6])
    for name, refs, coarsest in (("qvga", M.qvga_refs(n), 2), ("small", M.small_refs(n), 0)):
        lost = [r for r in refs if r.status]
        stops = {(r.stop_level, r.stop_iter) for r in lost}
        print(name, len(lost), "lost of", n, sorted(stops), "largest step", max(r.theta_max for r in refs))
        assert 4 * (n - len(lost)) >= n and 10 * len(lost) >= n
        assert len(stops) >= 3 and (coarsest, 0) in stops
        assert any(l == coarsest and it > 0 for l, it in stops)
        assert max(r.theta_max for r in refs) < 0.5
        assert refs[M.FAR].status == 1 and (refs[M.FAR].stop_level, refs[M.FAR].stop_iter) == (coarsest, 0)
        assert refs[M.FAR].solves == 0 and bytes(refs[M.FAR].pose) == bytes(Pose.from_matrix(st[M.FAR]))
        assert refs[M.FAR - 1].status == 0 and refs[M.FAR + 1].status == 0
        assert refs[0].fields() == refs[8].fields() == refs[10].fields() and refs[1].fields() == refs[6].fields()
        assert len({r.fields() for r in refs}) > 100
    q = M.qvga_refs(n)
    assert any(r.status and r.stop_level < 2 for r in q)  # lost at a finer level
    for k, (_, _, stop) in enumerate(M.FOUND):
        assert (q[12 + k].status, q[12 + k].stop_level, q[12 + k].stop_iter) == (1,) + stop
    for m in (1, 3, 5, 21):  # the smaller batches are prefixes
        assert [r.fields() for r in M.qvga_refs(m)] == [r.fields() for r in q[:m]]


def test_chunk_rule(kfx_lib):
    L = kfx_lib.lib()
    for w, h in SIZES:
        for n in COUNTS:
            assert kfx_lib.icp_multi_chunk(w, h, n) == M.chunk_np(w, h, n), (w, h, n)
    assert M.chunk_np(320, 240, 130) == 16 and M.chunk_np(320, 240, 21) == 2 and M.chunk_np(80, 48, 130) == 1
    assert M.chunk_np(80, 48, 600) == 2 and M.chunk_np(80, 48, 600 + 1) == 2
    for bad in ((0, 240, 1), (320, 0, 1), (320, 240, 0), (1 << 14, 1 << 13, 1)):
        assert L.kfx_icp_multi_chunk(*bad) == -1
    # the ICP's pixel blocks, not the quality record's whole-image ones
    # (QVGA: 70 blocks of the 320 x 224 covered pixels, 8 chunks fill the grid; the record's 75 blocks need 7)
    assert kfx_lib.icp_multi_chunk(320, 240, 100) == 12 and kfx_lib.quality_chunk(320, 240, 100) == 14


def test_result_record_layout(kfx_lib):
    assert C.sizeof(IcpResult) == 112 and IcpResult.x.offset == 64 and IcpResult.status.offset == 48
    hdr = open(os.path.join(ROOT, "include", "kfx.h")).read()
    assert re.search(r"sizeof\(kfx_icp_result\) == 112", hdr)
    for sym in ("kfx_icp_multi", "kfx_track_view", "kfx_resume_at", "kfx_icp_multi_chunk", "kfx_get_icp_multi_ms"):
        assert sym in kfx_lib.EXPORTS and hasattr(C.CDLL(kfx_lib.LIB_PATH), sym)
    r = IcpResult()
    assert r.fields() == M.Result(pose=Pose(), status=0, stop_level=0, stop_iter=0, solves=0, x=np.zeros(6)).fields()


BUILDS = {
    "O2": ["-O2"],
    "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", list(BUILDS))
def test_host_arithmetic_program(tmp_path, build):
    """tests/multi/multi_check.cpp: kfx_multi.h's chunk rule and float32 pose product, as its own binary."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "multi_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", *BUILDS[build], "-I",
                    os.path.join(ROOT, "slam-kinectfusion_amd", "csrc"),
                    os.path.join(ROOT, "tests", "multi", "multi_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=300)
    m = re.search(r"bad (\d+) chunk (\d+) poses (\d+)", r.stdout)
    assert m and r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert (int(m.group(1)), int(m.group(3))) == (0, 20000) and int(m.group(2)) > 300
