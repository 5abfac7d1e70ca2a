#!/usr/bin/env python3
"""Counts, by opcode, the vector instructions on the HOT PATH of a fast Euler / RK4 trace kernel's step loop: one iteration in which every lane holds a
ray and nothing rare happens (profiles/fast_step_diet_ab.txt).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -munsafe-fp-atomics -fno-fast-math --cuda-device-only -S kr_trace.hip -o a.s
    scripts/isa_hot_path.py a.s [b.s] SUBSTR... [--blocks]      (SUBSTR: part of the mangled kernel name, e.g. trace_kernelIdLi1ELb0ELb1ELb0)

Works on the compiler's assembly (labels, "Loop Header" comments), like scripts/isa_segment.py.  The walk starts at the loop header and ends where the
step's arm of the loop ends (the target of the first s_cbranch_execz after the header: beyond it lies the queue visit; the second one, "this lane holds a
ray", is walked through).  On the way
  * a wave-uniform forward branch (s_cbranch_vccz / vccnz / scc0 / scc1) is TAKEN: such branches jump over what a wave rarely needs -- the landing
    clips, the ERGO and NEG_ENERGY flags, the pole reflection -- unless its target lies BEHIND the step's arm of the loop: that is a rare arm the compiler
    moved out of line (the code behind the quiet-step and cap guards; it branches back), and the walk falls through;
  * an s_cbranch_execz whose span holds a call (s_swappc_b64) is taken too, if the step's arithmetic goes on behind its target: the libm fallback of
    the sine / cosine and the redo of the three stages.  ("No polar turning point" spans the rest of the step: it is walked through, and its else arm --
    the block behind its target, where a lane that did turn counts its step -- is left out);
  * a basic block that negates an integer sign (v_sub_u32 vN, 0, vN: the turning points, the pole reflection) or sets a status bit (v_or_b32 vN, 2 / 16 /
    32, vN) is left out;
  * every other block is walked through, an unconditional forward s_branch followed.
--blocks prints the labels of what was skipped, so that the walk can be checked against the listing."""
import collections
import re
import sys

UNIFORM = ("s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_scc0", "s_cbranch_scc1")
FP64 = re.compile(r"^v_(fma|fmac|mul|add)_f64")
RARE = (re.compile(r"^v_sub_u32_e32 (v\d+), 0, \1$"), re.compile(r"^v_or_b32_e32 (v\d+), (2|16|32), \1$"))


def kernel_lines(path, key):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(key) + r"\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    return lines[start:end]


def is_label(t):
    return bool(re.match(r"^\.LBB\d+_\d+:", t)) or t.startswith("; %bb.")


def label_name(t):
    return t.split(":")[0] if t.startswith(".LBB") else t.split()[1]


def hot_path(path, key):
    lines = [l.strip() for l in kernel_lines(path, key)]
    where = {label_name(t): i for i, t in enumerate(lines) if t.startswith(".LBB")}
    i = next(j for j, t in enumerate(lines) if "Loop Header" in t)
    stop, own, ops, skipped, else_arm = None, 0, [], [], None
    while i < len(lines) and (stop is None or i < stop):
        # one basic block: [i, j)
        j = i + 1
        while j < len(lines) and not is_label(lines[j]):
            j += 1
        body = [t for t in lines[i:j] if t and not t.startswith((";", ".")) and not is_label(t)]
        if else_arm is not None and i > else_arm and lines[i].startswith("; %bb."):
            skipped.append(label_name(lines[i]) + " (polar turning point)")
            else_arm = None
            i = j
            continue
        if any(r.match(t) for t in body for r in RARE):
            skipped.append(label_name(lines[i]) + " (sign flip / status bit)")
            i = j
            continue
        nxt = j
        for t in body:
            op = t.split()[0]
            if op.startswith("v_"):
                ops.append(op)
            if op.startswith("s_cbranch") or op == "s_branch":
                target = where.get(t.split()[1])
                if target is None or target <= i:
                    continue          # (the loop's back edge)
                if op == "s_cbranch_execz" and own < 2:
                    own += 1          # the loop's own two: the step's arm (it ends at the first one's target), the lanes that hold a ray
                    stop = target if stop is None else stop
                elif op in UNIFORM and stop is not None and target >= stop:
                    skipped.append(f"{t.split()[1]} (out of line)")       # a rare arm the compiler moved behind the loop (it branches back): not taken
                elif op in UNIFORM or op == "s_branch":
                    if target > j:
                        skipped.append(f"{label_name(lines[j]) if j < len(lines) else '?'} .. {t.split()[1]} (uniform branch)")
                    nxt = target
                elif op == "s_cbranch_execz" and any("s_swappc_b64" in u for u in lines[j:target]) and any(FP64.match(u) for u in lines[target:stop]):
                    skipped.append(f"{label_name(lines[j])} .. {t.split()[1]} (holds a call)")
                    nxt = target
                elif op == "s_cbranch_execz" and any("s_swappc_b64" in u for u in lines[j:target]):
                    else_arm = target
        i = nxt
    return ops, skipped


def main():
    files = [a for a in sys.argv[1:] if a.endswith(".s")]
    show = "--blocks" in sys.argv
    for key in [a for a in sys.argv[1:] if not a.endswith(".s") and not a.startswith("--")]:
        walks = [hot_path(f, key) for f in files]
        counts = [collections.Counter(w[0]) for w in walks]
        print(key, " / ".join(str(sum(c.values())) for c in counts), "vector instructions on the hot path;",
              " / ".join(str(sum(v for k, v in c.items() if "f64" in k and "cvt" not in k and "cmp" not in k)) for c in counts), "of them fp64 arithmetic")
        for k in sorted(set().union(*counts)):
            row = [c[k] for c in counts]
            print(f"    {k:24s}", " / ".join(f"{v:3d}" for v in row), "" if len(set(row)) == 1 else "   <--")
        if show:
            for f, w in zip(files, walks):
                print("  skipped in", f, *w[1], sep="\n      ")


if __name__ == "__main__":
    main()
