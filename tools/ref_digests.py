#!/usr/bin/env python3
"""Writes tests/golden/ref_digests.json from the reference's own kernels
compiled for the host (oracle/_ref/libkfx_ref.so; `make -C oracle ref`).

Per case id of tests/ref_cases.py: one SHA-256 over the reference's output
arrays (little-endian, NaNs canonicalised to 0x7fc00000, signed zeros kept),
or, for ICP cases, the 27 sums themselves per pose; and the number of elements
the case masks (ref_cases.masks; cases that mask nothing are not listed).  CPU only.

  python tools/ref_digests.py            # rewrite the fixture
  python tools/ref_digests.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("slam-kinectfusion_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import ref_cases as R  # noqa: E402


def main():
    ref = R.reference()
    if ref is None:
        sys.exit("libkfx_ref.so is absent and the reference is not here to build it")
    cases, masked = {}, {}
    for cid, fn in R.CASES.items():
        out, masked[cid] = R.masked_outputs(cid, fn, fn(ref))
        cases[cid] = R.recorded(cid, out)
        print(cid, cases[cid] if isinstance(cases[cid], str) else "(sums)", flush=True)
    doc = {"format": "sha256 over name:kind+itemsize:shape; + little-endian bytes per output, NaN = 0x7fc00000",
           "cases": cases,
           "masked_elements": {cid: n for cid, n in masked.items() if n}}
    if "--check" in sys.argv:
        with open(R.GOLDEN) as f:
            old = json.load(f)
        bad = [c for c in cases if old["cases"].get(c) != cases[c]]
        print("differing:", bad)
        sys.exit(1 if bad or sorted(old["cases"]) != sorted(cases) else 0)
    os.makedirs(os.path.dirname(R.GOLDEN), exist_ok=True)
    with open(R.GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"wrote {R.GOLDEN}: {len(cases)} cases, {os.path.getsize(R.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
