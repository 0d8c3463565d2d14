#!/usr/bin/env python3
"""Compares the k_filter_rows2 instantiations of two device assembly files (hipcc --cuda-device-only -S, or the
--save-temps .s of jxl_hip_api.hip): the function bodies between a symbol's label and its .Lfunc_end, with the symbols
named by their template arguments only, so that a template parameter added with a default does not count as a difference.
usage: isa_diff_rows2.py before.s after.s    (exit status 1 when an instantiation present in both differs)"""
import re
import sys


def bodies(path):
    out, name, cur = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"^(_ZN6jxlhip14k_filter_rows2I\w+):", line)
        if m:
            name, cur = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                name = None
            elif not line.lstrip().startswith((";", ".")) or line.lstrip().startswith(".LBB"):
                cur.append(line.split(";")[0].rstrip())
    return out


def key(sym):
    """Template arguments (U8SRGB, EPF, GAB, GREY) of a mangled k_filter_rows2 name; GREY defaults to 0."""
    args = re.match(r"_ZN6jxlhip14k_filter_rows2I((?:L[bi]\d+E)+)E", sym).group(1)
    vals = [int(v) for v in re.findall(r"L[bi](\d+)E", args)]
    return tuple(vals + [0] * (4 - len(vals)))


def main():
    a = {key(k): v for k, v in bodies(sys.argv[1]).items()}
    b = {key(k): v for k, v in bodies(sys.argv[2]).items()}
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print("k_filter_rows2<%s>: only in %s (%d instructions)" % (", ".join(map(str, k)), "after" if k in b else "before", len(b.get(k) or a.get(k))))
            continue
        strip = lambda body: [re.sub(r"_ZN6jxlhip14k_filter_rows2I\w+", "SYM", re.sub(r"\.LBB\d+_", ".LBB_", l)) for l in body]
        same = strip(a[k]) == strip(b[k])
        bad += not same
        print("k_filter_rows2<%s>: %d instructions, %s" % (", ".join(map(str, k)), len(a[k]), "identical" if same else "DIFFERENT (%d after)" % len(b[k])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
