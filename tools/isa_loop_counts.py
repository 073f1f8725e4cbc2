#!/usr/bin/env python3
"""Static VALU counts per basic block of one kernel, from the assembly hipcc writes with -S.

    hipcc <the Makefile's flags> --cuda-device-only -S csrc/cf_mbconv3.hip -o mbconv3.s
    python tools/isa_loop_counts.py mbconv3.s 'expdw_mx_kernelILi5ELi6'          # substring of the mangled name

Every basic block (a label up to the next one) is printed with its VALU instructions split into the classes the loop-overhead
survey uses (profiles/r07_loop_overhead.md):
    trans   v_exp / v_rcp / v_log / v_rsq / v_sqrt / v_sin / v_cos      (quarter-rate transcendental pipe)
    arith   v_pk_* / v_fma / v_mul_f32 / v_add_f32 / v_cvt* / v_perm / v_dot / v_max_f / v_min_f / v_med3_f / v_ldexp ...  (the op's arithmetic)
    select  v_cndmask
    move    v_mov / v_accvgpr / v_readlane / v_readfirstlane / v_writelane
    addr    integer work: v_mad_u64_u32, v_lshl_add_u64, v_mul_lo / hi, v_add_u32, v_add_co / v_addc, shifts, and / or, min / max, compares ...
plus MFMA, LDS, vector-memory and scalar counts.  A block whose last branch targets itself or an earlier label is marked `loop<-`:
the body of a loop is the run of blocks from the target label to that branch (`--loops` sums those runs).
"""
import argparse
import collections
import re

TRANS = ("v_exp", "v_rcp", "v_log", "v_rsq", "v_sqrt", "v_sin", "v_cos")
MOVE = ("v_mov", "v_accvgpr", "v_readlane", "v_readfirstlane", "v_writelane", "v_swap")
ARITH = ("v_pk_", "v_fma", "v_mul_f", "v_add_f", "v_sub_f", "v_mac_f", "v_fmac", "v_cvt", "v_perm", "v_dot", "v_max_f", "v_min_f",
         "v_med3_f", "v_ldexp", "v_mul_legacy", "v_bfi", "v_and_or", "v_lshl_or", "v_pack")
CLASSES = ("trans", "arith", "select", "move", "addr", "mfma", "lds", "vmem", "salu")


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_"):
        return "salu"
    if not op.startswith("v_"):
        return None
    if op.startswith(TRANS):
        return "trans"
    if op.startswith("v_cndmask"):
        return "select"
    if op.startswith(MOVE):
        return "move"
    if op.startswith(ARITH):
        return "arith"
    return "addr"


def blocks_of(path, needle):
    name, cur, out, order = None, None, collections.OrderedDict(), {}
    for line in open(path):
        s = line.strip()
        if name is None:
            m = re.match(r"^(_Z\w+):", s)
            if m and needle in m.group(1):
                name, cur = m.group(1), "entry"
                out[cur] = []
            continue
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if not s or s.startswith((";", ".", "//")):
            continue
        out[cur].append(s.split(";")[0].split())
    for i, k in enumerate(out):
        order[k] = i
    return name, out, order


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernel", help="substring of the mangled kernel name")
    ap.add_argument("--loops", action="store_true", help="print only the summed loop bodies")
    ap.add_argument("--dump", metavar="LABEL", help="print the VALU opcodes of one block")
    a = ap.parse_args()
    name, blocks, order = blocks_of(a.asm, a.kernel)
    if name is None:
        raise SystemExit("no kernel matching %r" % a.kernel)
    print(name)
    counts, loops = {}, []
    for lab, ins in blocks.items():
        c = collections.Counter()
        back = None
        for t in ins:
            k = classify(t[0])
            if k:
                c[k] += 1
            if t[0].startswith(("s_cbranch", "s_branch")) and t[-1] in order and order[t[-1]] <= order[lab]:
                back = t[-1]
        counts[lab] = c
        if back:
            loops.append((back, lab))
        if not a.loops:
            valu = sum(c[k] for k in ("trans", "arith", "select", "move", "addr"))
            print("%-12s valu %4d | %s%s" % (lab, valu, " ".join("%s %d" % (k, c[k]) for k in CLASSES if c[k]), ("  loop<- " + back) if back else ""))
        if a.dump == lab:
            print("   " + " ".join(t[0] for t in ins if t[0].startswith("v_") and classify(t[0]) != "mfma"))
    for head, tail in loops:
        c = collections.Counter()
        for lab in list(blocks)[order[head]:order[tail] + 1]:
            c.update(counts[lab])
        valu = sum(c[k] for k in ("trans", "arith", "select", "move", "addr"))
        print("loop %s..%s: valu %d | %s" % (head, tail, valu, " ".join("%s %d" % (k, c[k]) for k in CLASSES if c[k])))


if __name__ == "__main__":
    main()
