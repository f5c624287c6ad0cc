#!/usr/bin/env python3
"""Compare the device functions of two assembly directories (make asm) by
mangled name: instruction text (comments stripped, the function index in local
labels normalised) and the .amdhsa_* descriptor lines.  Prints same / DIFF per
function and the names on one side only; exit status 1 on either.
usage: tools/isa_same.py A_dir B_dir"""
import glob
import os
import re
import sys


def load(d):
    code, desc = {}, {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        pending, cur = set(), None
        for raw in open(path):
            line = re.sub(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+", r".\1", raw.split(";")[0]).strip()
            m = re.match(r"\.type\s+(\S+),@function", line)
            if m:
                pending.add(m.group(1))
            elif line.endswith(":") and line[:-1] in pending:
                cur = code.setdefault(line[:-1], [])
            elif line.startswith(".Lfunc_end"):
                cur = None
            elif line.startswith(".amdhsa_kernel "):
                cur = desc.setdefault(line.split()[1], [])
            elif line == ".end_amdhsa_kernel":
                cur = None
            elif cur is not None and line:
                cur.append(line)
    return code, desc


(ca, da), (cb, db) = load(sys.argv[1]), load(sys.argv[2])
bad = 0
for name in sorted(set(ca) | set(cb)):
    if name not in ca or name not in cb:
        print(f"ONLY in {sys.argv[1] if name in ca else sys.argv[2]}: {name}")
        bad += 1
        continue
    same_code, same_desc = ca[name] == cb[name], da.get(name) == db.get(name)
    bad += not (same_code and same_desc)
    print(f"{'same' if same_code else 'DIFF'} code ({len(ca[name])} lines)  "
          f"{'same' if same_desc else 'DIFF'} descriptor ({len(da.get(name, []))} lines)  {name}")
print(f"{len(set(ca) | set(cb))} device functions, {bad} differing or one-sided")
sys.exit(1 if bad else 0)
