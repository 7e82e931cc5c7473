#!/usr/bin/env python3
"""Compare two `hipcc -S --cuda-device-only` listings kernel by kernel (comments, directives and label numbers ignored).
    python tools/isa_diff.py before.s after.s
A kernel whose parameter types were renamed or moved has another mangled name on each side: kernels left over on both sides are paired
by their own name (`k_ploc_apply`) where that is unique, and reported as RENAMED.
Used in round 4 to show that moving the experiments out of rt_trace_wave.h left the production kernels' ISA unchanged."""
import re
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    # (functions only: a data symbol's label -- a constant table in front of a kernel -- would swallow the kernel behind it)
    for m in re.finditer(r'^\s*\.type\s+(_Z\w+),@function\n(?:[^\n]*\n)*?\1:[^\n]*\n(.*?)^\.Lfunc_end\d+:', txt, re.S | re.M):
        lines = []
        for l in m.group(2).split('\n'):
            t = l.split(';')[0].rstrip()
            if not t.strip() or t.strip().startswith('.'):
                continue
            lines.append(re.sub(r'\.LBB\d+_', '.LBB_', t))
        out[m.group(1)] = lines
    return out


def own_name(mangled):
    """k_name of _ZN12_GLOBAL__N_16k_nameE... or _Z6k_name..."""
    m = re.match(r'_ZN?(?:12_GLOBAL__N_1)?(\d+)', mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else mangled


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
left_a, left_b = [k for k in a if k not in b], [k for k in b if k not in a]
for k in left_a:
    twins = [j for j in left_b if own_name(j) == own_name(k)]
    if len(twins) == 1 and sum(own_name(j) == own_name(k) for j in left_a) == 1:
        print("  RENAMED %s: %s -> %s" % (own_name(k), k[:110], twins[0][:110]))
        b[k] = b.pop(twins[0])
same = [k for k in a if k in b and a[k] == b[k]]
diff = [k for k in a if k in b and a[k] != b[k]]
print("kernels: %d before, %d after; identical %d, different %d" % (len(a), len(b), len(same), len(diff)))
for k in diff:
    print("  DIFFERENT %s: %d -> %d instructions" % (k[:110], len(a[k]), len(b[k])))
for k in a:
    if k not in b:
        print("  only before:", k[:110])
for k in b:
    if k not in a:
        print("  only after:", k[:110])
