"""Free-space certificate of integrate's settled-brick skip (csrc/kfx_settled.h, CPU).

k_integrate steps over a brick (8x8 columns x 8 slices) whose settled byte is
set when kfx::brick_certified proves, from the frame's pose and min-depth grid,
that every voxel of the brick is either not updated or updated with ts = 1
outside the colour band.  tests/settled/settled_check.cpp
draws seeded intrinsics, poses, depth images with dropouts and depth steps,
and bricks (anywhere, a few centimetres in front of a surface, across the
image border) and evaluates every voxel of each certified brick with the
oracle's arithmetic; one voxel updated with ts < 1 or in the colour band fails
the run, and so does a run that certified no brick of one of the kinds.  Built
plain (-O2, no contraction) and, on fewer cases, under ASan + UBSan."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "settled", "settled_check.cpp")
INC = os.path.join(ROOT, "slam-kinectfusion_amd", "csrc")


@pytest.mark.parametrize("flags,seeds,cases", [
    (["-O2"], (1, 2, 3), 150),
    (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], (4,), 40),
], ids=["O2", "asan_ubsan"])
def test_certified_bricks_need_no_update(tmp_path, flags, seeds, cases):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "settled_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *flags, "-I", INC, SRC, "-o", exe],
                   check=True)
    for seed in seeds:
        r = subprocess.run([exe, str(seed), str(cases)], capture_output=True, text=True, timeout=300)
        m = re.search(r"bad (\d+) certified (\d+) of (\d+) near (\d+) edge (\d+)", r.stdout)
        assert m, (r.stdout[-2000:], r.stderr[-2000:])
        bad, cert, total, near, edge = map(int, m.groups())
        print(f"seed {seed}: certified {cert} of {total} bricks ({100.0 * cert / total:.1f} %), "
              f"{near} beside a surface, {edge} across the image border")
        assert r.returncode == 0 and bad == 0 and cert > 0 and near > 0 and edge > 0, r.stdout[-2000:]
