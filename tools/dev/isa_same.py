#!/usr/bin/env python3
"""usage: tools/dev/isa_same.py [--labels] A.s B.s — are two device assemblies (hipcc --offload-device-only -S, e.g. tools/dev/isa.sh) the same
code?  Each file is cut by kernel symbol: a kernel's text runs from its .globl line to the next kernel's, so it holds the code, the
.amdhsa_kernel descriptor block and the resource summary; what follows the last kernel is compared as "(metadata)".  Lines naming
__hip_cuid_ (the per-compilation id) are ignored.  Prints the kernels only one file has and the kernels whose text differs;
exit status 1 if there are any.  A comparison of text, nothing else.
--labels: for two sources that do not hold the same SET of kernels.  The compiler numbers the functions of a file and writes the
number into every local label (.LBB<f>_<n>, BB<f>_<n> in loop comments, .Lfunc_end<f>, .LJTI<f>_<n>), and a kernel's text as cut
above ends with the section header of whatever function follows it: a kernel added or removed elsewhere changes both without
changing an instruction.  With --labels the function number is taken out of the labels and the lines that open the following
function's section (.section / .protected / .weak / .hidden, and the "-- Begin function" comment) are dropped; a kernel's text ends
with its resource summary ("; Kernel info:" comments), only kernels are compared, and the blanks in front of a trailing comment
(padding to a column, which moves when a function number gains a digit) count as one."""
import re
import sys


LABELS = "--labels" in sys.argv
if LABELS:
    sys.argv.remove("--labels")


def normal(l):
    if not LABELS:
        return l
    if re.match(r"\s*\.(section|protected|weak|hidden)\s", l) or "-- Begin function" in l:
        return None
    # (the blanks in front of a label's trailing comment pad it to a column: a function number with one digit more moves them)
    return re.sub(r"\s+;", " ;", re.sub(r"(\.LBB|\bBB|\.Lfunc_end|\.Lfunc_begin|\.LJTI)\d+", r"\1", l))


def kernels(path):
    lines = [l for l in open(path).read().split("\n") if "__hip_cuid_" not in l]
    names = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    out, cur, info = {}, "(preamble)", False
    for l in lines:
        m = re.match(r"\s*\.globl\s+(\S+)", l)
        if m and m.group(1) in names:
            cur, info = m.group(1), False
        elif LABELS and l.startswith("; Kernel info:"):
            info = True
        elif LABELS and info and not l.startswith(";") and cur != "(metadata)":
            cur = "(between)"  # what follows a kernel's resource summary belongs to no kernel
        elif l.lstrip().startswith(".amdgpu_metadata"):
            cur = "(metadata)"
        l = normal(l)
        if l is not None:
            out.setdefault(cur, []).append(l)
    return out, len(names)


(a, na), (b, nb) = kernels(sys.argv[1]), kernels(sys.argv[2])
only = sorted(set(a) ^ set(b))
differ = sorted(k for k in set(a) & set(b) if a[k] != b[k] and not (LABELS and k in ("(between)", "(metadata)", "(preamble)")))
for k in only:
    print("only in %s: %s" % (sys.argv[1] if k in a else sys.argv[2], k))
for k in differ:
    print("differs: %s (%d / %d lines)" % (k, len(a[k]), len(b[k])))
print("%d / %d kernels, %d only in one file, %d differ" % (na, nb, len(only), len(differ)))
sys.exit(1 if only or differ else 0)
