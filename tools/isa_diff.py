#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly listings, instruction for instruction.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -Iinclude -S --cuda-device-only csrc/X.hip -o X.s   (per file, per build)
    cat old/*.s > old.s; cat new/*.s > new.s; python tools/isa_diff.py old.s new.s

Kernels are matched by symbol name, so one that moved to another translation unit still compares.  Comments, directives and
blank lines are dropped and the function number in .LBB<n>_<k> labels is masked; everything else must be equal.
Exit status 1 if a kernel present in both listings differs.
"""
import difflib
import re
import sys


def kernels(path):
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            if cur:
                out[cur] = []
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            cur = None
        s = line.split(";", 1)[0].strip()
        if cur is None or not s or (s.startswith(".") and not s.endswith(":")):
            continue
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    changed = [k for k in sorted(set(old) & set(new)) if old[k] != new[k]]
    print(f"kernels: {len(old)} -> {len(new)}; identical {len(set(old) & set(new)) - len(changed)}, changed {len(changed)}, "
          f"gone {len(gone)}, added {len(added)}")
    for k in gone:
        print(f"  gone     {k} ({len(old[k])} instructions)")
    for k in added:
        print(f"  added    {k} ({len(new[k])} instructions)")
    for k in changed:
        ops = [o for o in difflib.SequenceMatcher(None, old[k], new[k], autojunk=False).get_opcodes() if o[0] != "equal"]
        print(f"  changed  {k}: {len(old[k])} -> {len(new[k])} instructions, -{sum(o[2] - o[1] for o in ops)} "
              f"+{sum(o[4] - o[3] for o in ops)} in {len(ops)} hunk(s)")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
