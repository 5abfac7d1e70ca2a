#!/usr/bin/env python3
"""Counts the vector instructions between a kernel's step-loop header and the second v_rsq_f64 after it -- on the fast path that is k1's two square
roots, i.e. the segment holds the queue test, the sine / cosine and the potentials of k1 (profiles/fast_ray_consts_ab.txt).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -munsafe-fp-atomics -fno-fast-math --cuda-device-only -S kr_trace.hip -o a.s
    scripts/isa_segment.py a.s [b.s] SUBSTR...        (SUBSTR: part of the mangled kernel name, e.g. trace_kernelIdLi1ELb0ELb1ELb0)

Works on the compiler's assembly (labels and the "Loop Header" comments), not on a disassembly."""
import collections
import re
import sys


def segment(path, key):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(key) + r"\S*:", l))
    header = next(i for i in range(start, len(lines)) if "Loop Header" in lines[i])
    ops, roots = [], 0
    for l in lines[header + 1:]:
        t = l.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        op = t.split()[0]
        if op.startswith("v_"):
            ops.append(op)
        if op.startswith("v_rsq_f64"):
            roots += 1
            if roots == 2:
                break
    return ops


def main():
    files = [a for a in sys.argv[1:] if a.endswith(".s")]
    for key in [a for a in sys.argv[1:] if not a.endswith(".s")]:
        counts = [collections.Counter(segment(f, key)) for f in files]
        differ = {k: tuple(c[k] for c in counts) for k in sorted(set().union(*counts)) if len({c[k] for c in counts}) > 1}
        print(key, " / ".join(str(sum(c.values())) for c in counts), "vector instructions", differ or "")


if __name__ == "__main__":
    main()
