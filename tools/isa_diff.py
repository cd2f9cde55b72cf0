#!/usr/bin/env python3
"""Per-kernel ISA comparison of two device-only assembly listings of the same source file:
    hipcc <the Makefile's release flags> -S --cuda-device-only csrc/X.hip -o old.s     (at the old commit; again at the new one)
    tools/isa_diff.py old.s new.s
A kernel's text is everything from its label to its .Lfunc_end, with the function's ordinal taken out of its local labels
(.LBB<n>_<k>, BB<n>_<k>: n counts the functions of the file, so it -- and the column of the comment behind it -- moves when
another kernel is dropped).  Prints the kernels only one side
has and whether every common kernel is identical; exit code 1 when a common kernel differs."""
import re
import subprocess
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel (\S+)", l))]
    out = {}
    for n in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(n + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        out[n] = [re.sub(r"\s+;", " ;", re.sub(r"BB\d+_", "BB_", l)) for l in lines[start + 1:end]]
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    syms = sorted(set(old) | set(new))
    dem = dict(zip(syms, subprocess.run(["c++filt"] + syms, capture_output=True, text=True, check=True).stdout.split("\n")))
    short = {s: re.sub(r"\(anonymous namespace\)::|\(.*\)$|^void ", "", dem[s]) for s in syms}
    common = [s for s in syms if s in old and s in new]
    differ = [s for s in common if old[s] != new[s]]
    print(f"{sys.argv[1]}: {len(old)} kernels, {sys.argv[2]}: {len(new)} kernels, {len(common)} in both, "
          f"{len(common) - len(differ)} identical, {len(differ)} differ")
    for tag, only in (("only old", [s for s in syms if s not in new]), ("only new", [s for s in syms if s not in old]),
                      ("DIFFER", differ)):
        for s in only:
            print(f"  {tag}: {short[s]}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
