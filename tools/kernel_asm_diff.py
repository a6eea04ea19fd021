#!/usr/bin/env python3
"""Compare two gfx950 assembly files (hipcc --cuda-device-only -S) kernel by kernel.

    kernel_asm_diff.py OLD.s NEW.s [--rename REGEX REPL]

Per kernel, the text from its entry label to .end_amdhsa_kernel (instruction stream + .amdhsa_* resource directives) is
compared after normalising the kernel's own symbol name, compiler-numbered local labels and comments.  --rename is applied
to OLD's kernel names before matching (a template parameter that was dropped).  Prints one line per kernel; exit status 1 if
the kernel sets differ or any kernel differs.  It only compares: no instruction is looked for.
"""
import argparse
import re
import sys


def kernels(path):
    lines = open(path).read().splitlines()
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        start = next(j for j in range(i, -1, -1) if lines[j].startswith(name + ":"))
        end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
        body = []
        for raw in lines[start:end + 1]:
            s = raw.split(";", 1)[0].strip()
            if not s or "__hip_cuid_" in s:
                continue
            s = s.replace(name, "KERNEL")
            s = re.sub(r"\.LBB\d+_", ".LBB_", s)
            s = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", s)
            body.append(s)
        out[name] = body
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", nargs=2, metavar=("REGEX", "REPL"))
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    if a.rename:
        old = {re.sub(a.rename[0], a.rename[1], k): v for k, v in old.items()}
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{'only in NEW' if name in new else 'only in OLD'}  {name}")
            bad += 1
        elif old[name] != new[name]:
            n = next((i for i, (x, y) in enumerate(zip(old[name], new[name])) if x != y), min(len(old[name]), len(new[name])))
            print(f"DIFFERS ({len(old[name])} vs {len(new[name])} lines, first at {n})  {name}")
            bad += 1
        else:
            print(f"identical ({len(new[name])} lines)  {name}")
    print(f"{len(new)} kernels, {bad} differing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
