"""A chunk's brick masks from the tile kernel's certificate rounds (csrc/kfx_tilemask.h, CPU).

k_int_tiles evaluates the settled bytes and certificates once per brick of a
column tile's interval, in rounds of 64 bricks, and chunk_masks_round turns a
round's ballots into each chunk's skipm / setm.
tests/tilemask/tilemask_check.cpp holds that against the per-lane formula of an
integrate wave that computes its own masks (lane k <-> brick (za >> 3) + k,
its first 64 bricks only): exhaustively over the intervals inside [1, 600),
1..8 chunks, geometric, equal and random monotone brick-rounded cuts, with
random certificate bits, settled bytes and chunks without a live lane.  Every
working chunk's skipm, setm, free mask and overhang mask must be equal.

Against a vacuous pass the run must have compared chunks of more than 64
bricks (the first-64 rule over two rounds) and chunks with an overhanging
hidden brick, and the mutation (the free mask without the chunk's own `inside`
range) must fail.  Built plain (-O2) and, on every 13th interval start, under
ASan + UBSan as a stand-alone host program."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tilemask", "tilemask_check.cpp")
INC = os.path.join(ROOT, "slam-kinectfusion_amd", "csrc")

BUILDS = {
    "O2": (["-O2"], 1),
    "asan_ubsan": (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 13),
}
LINE = re.compile(r"bad (\d+) cases (\d+) chunks (\d+) deep (\d+) overhang (\d+) dead (\d+)")


@pytest.fixture(scope="module")
def executables(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = {}
    for name, (flags, _) in BUILDS.items():
        out[name] = str(tmp_path_factory.mktemp("tilemask_" + name) / "tilemask_check")
        subprocess.run(["g++", "-std=c++17", *flags, "-I", INC, SRC, "-o", out[name]], check=True)
    return out


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
    m = LINE.search(r.stdout)
    assert m, (r.stdout[-2000:], r.stderr[-2000:])
    return r, tuple(map(int, m.groups()))


@pytest.mark.parametrize("build", list(BUILDS))
def test_chunk_masks_equal_the_wave_formula(executables, build):
    step = BUILDS[build][1]
    r, (bad, cases, chunks, deep, overhang, dead) = run(executables[build], step)
    print(f"{cases} cases, {chunks} working chunks ({deep} of more than 64 bricks, {overhang} with an overhanging "
          f"hidden brick), {dead} chunks without work")
    assert r.returncode == 0 and bad == 0, r.stdout[-2000:]
    n_intervals = sum(600 - wl for wl in range(1, 600, step))
    assert cases == n_intervals * 8 * 3
    assert deep >= 1000 and overhang >= 1000 and dead >= 1000


def test_mutation_fails(executables):
    r, (bad, *_rest) = run(executables["O2"], 7, "mut")
    assert r.returncode != 0 and bad > 0
