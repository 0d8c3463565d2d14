#!/usr/bin/env python3
"""Compares the kernels of two device assembly files (hipcc --cuda-device-only -S of jxl_hip_api.hip, the Makefile's
other flags): for every function whose demangled name matches the pattern, the instructions between its label and its
.Lfunc_end, and the resources the compiler reports behind it. Local labels are renumbered; a kernel whose instructions
differ only in the name of a data symbol they address (a table that moved) is reported as such, not as identical.
usage: isa_diff_kernels.py before.s after.s [pattern] [--expect-different pattern]
exit status 1 when a kernel outside --expect-different is missing on one side or differs in more than symbol names."""
import re
import subprocess
import sys

RESOURCES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels(path):
    """{symbol: (instructions, {resource: value})} for the functions of an assembly file."""
    out, name, cur, last = {}, None, [], None
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, cur = m.group(1), []
            continue
        if name is not None:
            s = line.lstrip()
            if line.startswith(".Lfunc_end"):
                out[name] = (cur, {})
                last, name = name, None
            elif not s.startswith((";", ".")) or s.startswith(".LBB"):
                cur.append(line.split(";")[0].rstrip())
        elif last is not None:
            m = re.match(r"^; (\w+): (\d+)\b", line)
            if m and m.group(1) in RESOURCES:
                out[last][1].setdefault(m.group(1), int(m.group(2)))
    return out


def demangle(symbols):
    r = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True)
    names = r.stdout.split("\n") if r.returncode == 0 else symbols
    return dict(zip(symbols, [re.sub(r"^void ", "", n) for n in names]))


def normal(body, data_symbols):
    body = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in body]
    if data_symbols:
        body = [re.sub(r"[\w.$]+@(rel32@lo|rel32@hi|gotpcrel32@lo|gotpcrel32@hi)", r"DATA@\1", l) for l in body]
    return body


def main():
    args = sys.argv[1:]
    expect = None
    if "--expect-different" in args:
        i = args.index("--expect-different")
        expect = re.compile(args[i + 1])
        del args[i:i + 2]
    pattern = re.compile(args[2] if len(args) > 2 else "")
    a, b = kernels(args[0]), kernels(args[1])
    names = demangle(sorted(set(a) | set(b)))
    bad = 0
    for sym in sorted(names, key=names.get):
        n = names[sym]
        if not pattern.search(n):
            continue
        expected = bool(expect and expect.search(n))
        if sym not in a or sym not in b:
            print("%s: only in %s" % (n, "after" if sym in b else "before"))
            bad += not expected
            continue
        (ia, ra), (ib, rb) = a[sym], b[sym]
        if normal(ia, False) == normal(ib, False):
            verdict = "identical"
        elif normal(ia, True) == normal(ib, True):
            verdict = "identical but for the names of data symbols"
        else:
            verdict = "DIFFERENT" if not expected else "different (expected)"
            bad += not expected
        res = ", ".join("%s %s" % (k, ra.get(k) if ra.get(k) == rb.get(k) else "%s -> %s" % (ra.get(k), rb.get(k))) for k in RESOURCES)
        print("%s: %s; instructions %s; %s" % (n, verdict, len(ia) if len(ia) == len(ib) else "%d -> %d" % (len(ia), len(ib)), res))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
