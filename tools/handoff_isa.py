#!/usr/bin/env python3
"""Register budget and hand-off instruction counts of every k_fused instantiation.

Per kernel: VGPRs, scratch and LDS as the assembler directives state them, and - inside the tile loop (the largest
backward branch span, as tools/check_prefetch.py finds it) - how many v_readlane, v_cndmask, v_mov_b32_e32,
v_mov_b32_dpp, s_cselect and s_nop the loop holds (static counts: both arms of a branch are counted).

    python tools/handoff_isa.py [-DNAME=VALUE ...] [rtlfm_hip.s]        one line per kernel
    python tools/handoff_isa.py --diff before.s after.s                  only the kernels whose instructions differ

exit 1 if a kernel exceeds the VGPRs its waves per SIMD leave it (128 from three passes on) or has scratch.
"""
import re
import sys

from check_prefetch import compile_asm, instrs, kernels

COUNTED = ["v_readlane", "v_cndmask", "v_mov_b32_e32", "v_mov_b32_dpp", "s_cselect", "s_nop"]


def tile_loop(body):
    ins = instrs(body)
    labels = {m.group(1): i for i, t in enumerate(ins) for m in [re.match(r"^(\.LBB\d+_\d+):", t)] if m}
    best = None
    for i, t in enumerate(ins):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            span = (i - labels[m.group(1)], labels[m.group(1)], i)
            if best is None or span > best:
                best = span
    return ins[best[1]:best[2] + 1] if best else []


def table(asm):
    out = {}
    for name, body in kernels(asm):
        m = re.match(r"_ZN5rtlfm5fused7k_fusedILi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name)
        tag = "<%s,%s,%s,%s,%s,%s>" % m.groups() if m else name
        # the kernel descriptor follows the function body
        at = asm.index(".amdhsa_kernel " + name)
        desc = asm[at:asm.index(".end_amdhsa_kernel", at)]
        row = {k: int(re.search(r"\.amdhsa_%s\s+(\d+)" % d, desc).group(1))
               for k, d in (("vgpr", "next_free_vgpr"), ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"))}
        loop = tile_loop(body)
        row["loop"] = len(loop)
        row["body"] = hash("\n".join(instrs(body)))  # --diff: "unchanged" means the same instructions throughout
        for c in COUNTED:
            row[c] = sum(1 for t in loop if t.startswith(c))
        out[tag] = row
    return out


def fmt(row):
    return ("vgpr %3d scratch %d lds %5d | loop %4d: " % (row["vgpr"], row["scratch"], row["lds"], row["loop"])
            + " ".join("%s %d" % (c.replace("v_mov_b32_", "mov_"), row[c]) for c in COUNTED))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--diff":
        a, b = table(open(args[1]).read()), table(open(args[2]).read())
        same = 0
        for tag in b:
            if a.get(tag) == b[tag]:
                same += 1
                continue
            print(tag)
            print("    before: " + (fmt(a[tag]) if tag in a else "-"))
            print("    after:  " + fmt(b[tag]))
        print(f"{same} kernel(s) with the same instructions throughout")
        t = b
    else:
        defs = [x for x in args if x.startswith("-D")]
        given = [x for x in args if not x.startswith("-")]
        t = table(open(given[0]).read() if given else compile_asm(defs))
        for tag, row in t.items():
            print(f"{tag:16s} {fmt(row)}")
    # the kernels' launch bounds: two waves per SIMD with one pass, three with two, four from three passes on
    budget = lambda tag: {"1": 256, "2": 168}.get(tag[1], 128)
    bad = [tag for tag, row in t.items() if row["vgpr"] > budget(tag) or row["scratch"]]
    for tag in bad:
        print(f"{tag}: over budget ({t[tag]['vgpr']} VGPRs, {t[tag]['scratch']} B scratch)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
