"""Exact trip count of the raycast's march loop (csrc/kfx_raystep.h, CPU).

k_raycast bounds its march by a sample index: kfx::ray_sample_end gives the
number of iterations of the reference's `for (; ray_len < tfar; ray_len +=
step)` (tsdf_volume.cu:210-260) once per ray, and a hit's ray_len is
kfx::ff_add(L0, step, k).  Both must equal the plain float loop exactly:
tests/raystep/raystep_check.cpp compares them on 2.1 million seeded cases (the
configurations' real steps, starts beside binade edges, tfar within a few
steps of the start, on and one ulp beside a sequence value, NaN and +inf,
runs of up to 4096 samples out to 8 m), built plain (-O2, no contraction), and
on fewer cases under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "raystep", "raystep_check.cpp")
INC = os.path.join(ROOT, "slam-kinectfusion_amd", "csrc")


@pytest.mark.parametrize("flags,seeds,cases", [
    (["-O2"], (1, 2, 3), 700000),
    (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], (4,), 150000),
], ids=["O2", "asan_ubsan"])
def test_ray_sample_end_matches_plain_loop(tmp_path, flags, seeds, cases):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "raystep_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *flags, "-I", INC, SRC, "-o", exe],
                   check=True)
    for seed in seeds:
        r = subprocess.run([exe, str(seed), str(cases)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip() == "bad 0", (r.stdout[-2000:], r.stderr[-2000:])
