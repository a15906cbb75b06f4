#!/usr/bin/env python3
"""Compares the device assembly text of kernels between two `hipcc -S
--cuda-device-only` outputs, labels aside: for every kernel symbol that
matches `pattern` in both files, the instruction lines and the .amdhsa_
directives must be equal once local labels (.LBBn_m, .Lfunc_*) are renumbered
in order of appearance and comments are dropped.

usage: asm_diff.py parent.s tree.s [pattern]     (exit status 1 on a difference)"""
import re
import sys


def kernels(path, pattern):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            if name:
                out[name] = body
            name, body = (m.group(1), []) if re.search(pattern, m.group(1)) else (None, [])
            continue
        if name is None:
            continue
        if line.startswith("\t.section") or line.startswith("\t.text"):
            out[name] = body
            name = None
            continue
        body.append(line)
    if name:
        out[name] = body
    return out


def normal(body):
    labels, out = {}, []
    for line in body:
        line = line.split(";")[0].rstrip()
        if not line.strip() or line.strip().startswith((".loc", ".file", ".cfi", ".p2align")):
            continue
        line = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), line)
        out.append(line)
    return out


def main():
    a, b = sys.argv[1], sys.argv[2]
    pattern = sys.argv[3] if len(sys.argv) > 3 else "k_table"
    ka, kb = kernels(a, pattern), kernels(b, pattern)
    bad = 0
    for name in sorted(ka):
        if name.endswith(".kd"):
            continue
        if name not in kb:
            print("missing in %s: %s" % (b, name))
            bad += 1
            continue
        na, nb = normal(ka[name]), normal(kb[name])
        same = na == nb
        print("%s %s (%d lines)" % ("same " if same else "DIFF ", name, len(na)))
        if not same:
            bad += 1
            for i, (x, y) in enumerate(zip(na, nb)):
                if x != y:
                    print("  first difference at line %d:\n    %s\n    %s" % (i, x, y))
                    break
    for name in sorted(set(kb) - set(ka)):
        print("new   %s" % name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
