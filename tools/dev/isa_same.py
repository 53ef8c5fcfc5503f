#!/usr/bin/env python3
"""usage: tools/dev/isa_same.py A.s B.s — are two device assemblies (hipcc --offload-device-only -S, e.g. tools/dev/isa.sh) the same
code?  Each file is cut by kernel symbol: a kernel's text runs from its .globl line to the next kernel's, so it holds the code, the
.amdhsa_kernel descriptor block and the resource summary; what follows the last kernel is compared as "(metadata)".  Lines naming
__hip_cuid_ (the per-compilation id) are ignored.  Prints the kernels only one file has and the kernels whose text differs;
exit status 1 if there are any.  A comparison of text, nothing else."""
import re
import sys


def kernels(path):
    lines = [l for l in open(path).read().split("\n") if "__hip_cuid_" not in l]
    names = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    out, cur = {}, "(preamble)"
    for l in lines:
        m = re.match(r"\s*\.globl\s+(\S+)", l)
        if m and m.group(1) in names:
            cur = m.group(1)
        elif l.lstrip().startswith(".amdgpu_metadata"):
            cur = "(metadata)"
        out.setdefault(cur, []).append(l)
    return out, len(names)


(a, na), (b, nb) = kernels(sys.argv[1]), kernels(sys.argv[2])
only = sorted(set(a) ^ set(b))
differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
for k in only:
    print("only in %s: %s" % (sys.argv[1] if k in a else sys.argv[2], k))
for k in differ:
    print("differs: %s (%d / %d lines)" % (k, len(a[k]), len(b[k])))
print("%d / %d kernels, %d only in one file, %d differ" % (na, nb, len(only), len(differ)))
sys.exit(1 if only or differ else 0)
