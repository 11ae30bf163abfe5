#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files, matched by mangled name.

    hipcc <the Makefile's flags> --cuda-device-only -S csrc/UNIT.hip -o UNIT.s     (once per side)
    tools/kernel_isa_compare.py PARENT.s BRANCH.s [--match SUBSTRING ...]

Prints one line per kernel: identical or not (instruction text with block labels renumbered and comments dropped),
and on both sides .vgpr_count, .sgpr_count, LDS and scratch bytes and the number of instruction lines.  No assembly text.
Exit status 1 if a kernel exists on one side only or a kernel named by --match differs.
"""
import argparse
import re
import sys


def kernels(path):
    text = open(path).read().split("\n")
    body, cur, out = {}, None, None
    for line in text:
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L") and not line.startswith("\t"):
            cur, out = m.group(1), []
            body[cur] = out
            continue
        if line.startswith(".Lfunc_end"):
            cur = out = None
            continue
        if out is None:
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", s):
                out.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    meta, name, cur = {}, None, {}
    for line in text:   # the amdhsa.kernels metadata: one yaml record per kernel, .name among its keys
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if line.startswith("  - ."):
            cur = {}
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "name":
            meta[m.group(2).strip("'\"")] = cur
    res = {}
    for k, md in meta.items():
        if not body.get(k):
            sys.exit(f"{path}: kernel {k} is in the metadata but has no instructions under its label")
        ins = [l for l in body.get(k, []) if not l.endswith(":")]
        res[k] = dict(text=body.get(k, []), n=len(ins), vgpr=md.get("vgpr_count"), sgpr=md.get("sgpr_count"),
                      lds=md.get("group_segment_fixed_size"), scratch=md.get("private_segment_fixed_size"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--match", action="append", default=[], help="kernels whose name contains this must be identical")
    args = ap.parse_args()
    a, b = kernels(args.parent), kernels(args.branch)
    bad = 0
    print(f"# {args.parent}: {len(a)} kernels; {args.branch}: {len(b)} kernels")
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k} ONLY-IN-{'PARENT' if k in a else 'BRANCH'}")
            bad = 1
            continue
        x, y = a[k], b[k]
        same = x["text"] == y["text"]
        if not same and any(s in k for s in args.match):
            bad = 1
        print(f"{k} {'identical' if same else 'DIFFERENT'} vgpr {x['vgpr']}/{y['vgpr']} sgpr {x['sgpr']}/{y['sgpr']} "
              f"lds {x['lds']}/{y['lds']} scratch {x['scratch']}/{y['scratch']} instructions {x['n']}/{y['n']}")
    n_same = sum(1 for k in a if k in b and a[k]["text"] == b[k]["text"])
    print(f"# identical: {n_same} of {len(set(a) | set(b))}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
