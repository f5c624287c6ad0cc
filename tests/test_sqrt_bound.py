"""tools/sqrt_bound_check.cpp checks a copy of sqrt_le_bound: the copy is
textually the function in kfx_kernels.hip, and the tool, built plain and with
UBSan as a stand-alone binary, finds (sqrtf(x) <= t) == (x <= bound(t)) over
every 4099th non-negative float (inf and NaNs included) and the 64 floats on
either side of each bound."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "sqrt_bound_check.cpp")
KERNELS = os.path.join(ROOT, "slam-kinectfusion_amd", "csrc", "kfx_kernels.hip")


def body(path):
    src = open(path).read()
    a = src.index("float sqrt_le_bound(float t) {")
    return src[a:src.index("\n}\n", a) + 3]


def test_tool_checks_the_kernel_files_function():
    assert body(TOOL) == body(KERNELS)
    assert "std::nextafter" in body(TOOL) and body(TOOL).count("\n") > 10


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "ubsan"])
def test_bound_holds_over_strided_floats(flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sqrt_bound_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *flags, TOOL, "-o", exe], check=True)
    r = subprocess.run([exe, "4099"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("mismatches=0") == 8, r.stdout
