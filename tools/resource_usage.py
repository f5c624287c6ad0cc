#!/usr/bin/env python3
"""Tabulate the kernel-resource-usage remarks of the shipped kernels (the
Makefile's resource-usage target: every csrc/*.hip with the library's flags)."""
import os
import re
import subprocess

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slam-kinectfusion_amd")
out = subprocess.run(["make", "-s", "-C", PKG, "resource-usage"], capture_output=True, text=True, check=True).stdout
rows, cur = {}, None
for line in out.splitlines():
    m = re.search(r"remark:\s+(.*?):\s+(.*?) \[-Rpass", line)
    if not m:
        continue
    k, v = m.group(1).strip(), m.group(2).strip()
    if k == "Function Name":
        cur = re.sub(r"^_ZN3kfx12_GLOBAL__N_1\d+", "", v)[:44]
        rows[cur] = {}
    elif cur:
        rows[cur][k] = v
for f, d in rows.items():
    print(f"{f:46s} VGPR {d.get('VGPRs', '?'):>4} SGPR {d.get('TotalSGPRs', '?'):>4} "
          f"scratch {d.get('ScratchSize [bytes/lane]', '?'):>4} occ {d.get('Occupancy [waves/SIMD]', '?')} "
          f"LDS {d.get('LDS Size [bytes/block]', '?')}")
