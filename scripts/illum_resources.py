#!/usr/bin/env python3
"""Kernel resource usage of kr_line.hip and kr_response.hip in two trees, for profiles/illum_pass_resources.txt: every kernel instance that the first
tree (the parent commit) has must keep its SGPRs, VGPRs, AGPRs, scratch, LDS and occupancy in the second (this tree), and every ILLUM instance must have
the occupancy of its flat twin.  Cross-compiles for gfx950 with -Rpass-analysis=kernel-resource-usage; no GPU needed.

  python scripts/illum_resources.py PARENT_TREE [THIS_TREE]  > profiles/illum_pass_resources.txt

Kernel names are compared demangled, with the new trailing template argument ILLUM = false removed, and with it the line kernels' trailing kernel
argument IllumTab<false> and the response kernels' RespArg<false> read as the RespDev it is."""
import os
import re
import subprocess
import sys

FILES = ("kr_line.hip", "kr_response.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics", "-fno-fast-math", "-Rpass-analysis=kernel-resource-usage"]
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def listing(tree, src):
    """{demangled kernel name: {field: value}} of one source file of one tree."""
    csrc = os.path.join(tree, "raytrace_cpu_amd", "csrc")
    err = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-c", src, "-o", os.devnull], cwd=csrc, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            out[name] = {}
            continue
        m = re.search(r"remark: +([A-Za-z \[\]/]+): (\d+)", line)
        if m and name and m.group(1) in FIELDS:
            out[name][m.group(1)] = int(m.group(2))
    return out


def short(name):
    name = name.replace("kr::(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\(.*", "", name)


def flat_name(name):
    """The parent's name of an instance with ILLUM = false; None for an ILLUM = true instance."""
    if "IllumTab<true>" in name or "RespArg<true>" in name:
        return None
    name = name.replace(", kr::IllumTab<false>)", ")").replace("RespArg<false>", "RespDev")
    if re.search(r"(reduce_line_kernel|post_line_limb_kernel|response_kernel)<", name):
        name = re.sub(r", false>\(", ">(", name, count=1)         # the new trailing template argument
    return name


def main():
    parent, this = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(__doc__.split("\n\n")[0].replace("in two trees, for profiles/illum_pass_resources.txt", "before and after the ILLUM flavour") + "\n")
    print('"before": the parent commit; "after": this tree.  hipcc ' + " ".join(FLAGS) + "\n")
    changed = missing = 0
    new = []
    for src in FILES:
        before, after = listing(parent, src), listing(this, src)
        by_flat = {}
        for name, res in after.items():
            f = flat_name(name)
            if f is None:
                new.append((src, name, res))
            else:
                by_flat[f] = res
        for name, res in before.items():
            # (a trailing template argument that the parent left defaulted is printed in both trees, so the names match as they are)
            cands = [f for f in by_flat if f == name or f.replace(", false>(", ">(") == name]
            if len(cands) != 1:
                missing += 1
                print(f"{'MISSING' if not cands else 'AMBIGUOUS'} after: {src} {short(name)}")
                continue
            if by_flat[cands[0]] != res:
                changed += 1
                print(f"CHANGED: {src} {short(name)}\n    before {res}\n    after  {by_flat[cands[0]]}")
        print(f"{src}: kernel instances before {len(before)}, after with ILLUM = false or no such parameter {len(by_flat)}, after with ILLUM = true (new) "
              f"{sum(1 for s, _, _ in new if s == src)}")
    print(f"\ninstances present before and missing or ambiguous after: {missing}\ninstances whose {', '.join(FIELDS)} differ: {changed}\n")
    print("The new instances, each with the occupancy of its flat twin (the same template arguments with ILLUM = false) beside it:\n")
    worse = 0
    for src in FILES:
        after = listing(this, src)
        for s, name, res in new:
            if s != src:
                continue
            twin = name.replace("IllumTab<true>", "IllumTab<false>").replace("RespArg<true>", "RespArg<false>")
            twin = re.sub(r", true>\(", ", false>(", twin, count=1)
            t = after.get(twin)
            occ, tocc = res["Occupancy [waves/SIMD]"], (t or {}).get("Occupancy [waves/SIMD]")
            worse += tocc is None or occ < tocc
            print(f"{src:16s} {short(name)}\n    " + "  ".join(f"{k.split(' [')[0]}={res[k]}" for k in FIELDS) + f"\n    flat twin: VGPRs={(t or {}).get('VGPRs')}  Occupancy={tocc}")
    print(f"\nILLUM instances with a lower occupancy than their flat twin: {worse}")


if __name__ == "__main__":
    main()
