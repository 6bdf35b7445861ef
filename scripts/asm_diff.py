#!/usr/bin/env python3
"""Compare two gfx950 assembly files (hipcc -S --offload-device-only) kernel by
kernel: instruction text only, comments, directives and block-label numbers
stripped.  ``--map OLD=NEW`` (repeatable) rewrites a substring of the first
file's kernel names, for a template parameter list that changed.

    python scripts/asm_diff.py old.s new.s --map ELb1ELi2ELb0EEEv=ELi0EEEv
"""
import argparse
import re


def kernels(path):
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        line = line.split(";")[0].rstrip()
        m = re.match(r"^(\w+):", line)
        if m and not line.startswith(".L"):
            cur = m.group(1) if m.group(1) in names else None
            out.setdefault(cur, [])
        elif line.strip().startswith(".end_amdhsa_kernel") or line.strip().startswith(".Lfunc_end"):
            cur = None
        elif cur and line.strip() and (not line.strip().startswith(".") or line.strip().endswith(":")):
            out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", line.strip()))
    out.pop(None, None)
    return out


ap = argparse.ArgumentParser()
ap.add_argument("old"), ap.add_argument("new"), ap.add_argument("--map", action="append", default=[])
a = ap.parse_args()
old, new = kernels(a.old), kernels(a.new)
for m in a.map:
    old = {k.replace(*m.split("=", 1)): v for k, v in old.items()}
for k in sorted(set(old) | set(new)):
    state = "only-old" if k not in new else "only-new" if k not in old else \
        "identical" if old[k] == new[k] else "DIFFERENT"
    print(f"{state:9} {len(old.get(k, [])):6} {len(new.get(k, [])):6}  {k}")
