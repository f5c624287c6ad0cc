"""tools/sqrt_bound_check.cpp checks the library's own sqrt_le_bound: it
includes csrc/kfx_sqrtbound.h (as the ICP's kernel file does) and defines no copy, and
the tool, built plain and with UBSan as a stand-alone binary, finds
(sqrtf(x) <= t) == (x <= bound(t)) over every 4099th non-negative float (inf
and NaNs included) and the 64 floats on either side of each bound."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "sqrt_bound_check.cpp")
CSRC = os.path.join(ROOT, "slam-kinectfusion_amd", "csrc")


def test_tool_checks_the_librarys_function():
    tool = open(TOOL).read()
    inc = re.search(r'^#include "(.*kfx_sqrtbound\.h)"', tool, re.M)
    assert inc, "the tool includes the header"
    header = os.path.normpath(os.path.join(os.path.dirname(TOOL), inc.group(1)))
    assert header == os.path.join(CSRC, "kfx_sqrtbound.h")
    assert not re.search(r"\bsqrt_le_bound\s*\(\s*float\b", tool), "the tool defines no copy"
    # the one definition, shared with the ICP plan
    body = open(header).read()
    assert len(re.findall(r"\bsqrt_le_bound\s*\(\s*float\b", body)) == 1
    assert "std::nextafter" in body
    assert any(f.endswith(".hip") and '#include "kfx_sqrtbound.h"' in open(os.path.join(CSRC, f)).read()
               for f in os.listdir(CSRC)), "the ICP's kernel file includes the header"
    others = [f for f in os.listdir(CSRC) if f != "kfx_sqrtbound.h"
              and re.search(r"\bsqrt_le_bound\s*\(\s*float\b", open(os.path.join(CSRC, f)).read())]
    assert others == []


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
