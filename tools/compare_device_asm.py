"""Compare two device listings of one translation unit, kernel by kernel.

    hipcc <the build's flags> --cuda-device-only -S csrc/salnmf_nb.hip -o new.s      (and the same on the other commit)
    python tools/compare_device_asm.py old.s new.s

A function is the text from its ``; -- Begin function`` line to ``; -- End function`` (its resource directives included).  The
functions' index is taken out of their local labels (``.LBB3_7``, ``Header=BB3_7``, ``.Lfunc_end3``), so that a function removed
in front of a kernel does not make the kernel differ, and the compilation-unit id symbol is blanked.  Prints the functions only
one listing has, ``same`` or ``DIFFERENT`` for every other, and the differing lines outside the functions (the metadata).
Exit status 1 if a function both listings have differs."""
import difflib
import re
import sys


def split(path):
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    funcs, rest, cur, name = {}, [], None, None
    for line in text.splitlines():
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            name, cur = m.group(1), []
        if cur is None:
            rest.append(line)
            continue
        cur.append(re.sub(r"((?:\.L[A-Za-z_]*?|\bBB))\d+(_\d+)?\b", r"\1#\2", line))
        if "; -- End function" in line:
            funcs[name], cur = cur, None
    return funcs, rest


if __name__ == "__main__":
    (fa, ra), (fb, rb) = split(sys.argv[1]), split(sys.argv[2])
    print("only in the first:", sorted(set(fa) - set(fb)))
    print("only in the second:", sorted(set(fb) - set(fa)))
    both = sorted(set(fa) & set(fb))
    for n in both:
        print("same     " if fa[n] == fb[n] else "DIFFERENT", len(fa[n]), n)
    d = [line for line in difflib.unified_diff(ra, rb, lineterm="", n=0) if not line.startswith(("---", "+++", "@@"))]
    print("outside the functions:", len(d), "differing lines")
    for line in d:
        print("   ", line[:160])
    sys.exit(any(fa[n] != fb[n] for n in both))
