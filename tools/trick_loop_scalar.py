#!/usr/bin/env python3
"""Diagnostic: the scalar side of the trick-aligned STD card loop of k_play_wide<false> (play_role, tricks(true_type)).

    python tools/trick_loop_scalar.py [file.s]

Sibling of tools/trick_loop_isa.py (same loop, same way of finding it, same compile when no file is given).  Printed, for
each of the four cards of the fall-through path (header to back edge, split at the end of each card's pick) and for every
run of blocks of the loop that the fall-through walk does not enter (ring drain, lineless lane / deal in place, ...):
every scalar ALU instruction, s_nop, s_waitcnt, branch and v_readlane / v_writelane, with what it serves:

    addr    row / pointer arithmetic for the stores         exec    save / restore of exec around a divergent region
    mask    lane-mask bookkeeping of a per-lane bool        test    a wave-uniform test (compare, vote, its branch)
    pad     hazard padding (s_nop)                          loop    loop control (counter, compare, back edge)
    spill   v_readlane / v_writelane in the loop            wait    s_waitcnt
    const   a literal put into an SGPR for a vector op      ring    wave-uniform bookkeeping of the finished-games ring

and for every branch on the fall-through path whether that path takes it.  Then the totals per class, the vector side of
the store addressing (v_lshl_add_u64, v_add of the row offset) and the kernel's registers.  It counts classes of
instructions for profiles/*_isa.txt; it is not a test."""
import collections
import re
import sys

import trick_loop_isa as T

MASK_OPS = ("s_and_b64", "s_or_b64", "s_andn2_b64", "s_orn2_b64", "s_xor_b64", "s_not_b64", "s_mov_b64", "s_cselect_b64")
ADDR_OPS = ("s_add_u32", "s_addc_u32", "s_lshl_b64", "s_mul_i32", "s_mul_hi_u32", "s_lshl_b32", "s_sub_u32", "s_subb_u32", "s_ashr_i32")


def classify(ins, head, counter):
    f = ins.replace(",", " ").split()
    op, args = f[0], f[1:]
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "spill"
    if op == "s_nop":
        return "pad"
    if op == "s_waitcnt":
        return "wait"
    if op.startswith(("s_cbranch", "s_branch")):
        if args[0] == head:
            return "loop"
        return "exec" if "exec" in op else "test"
    if "saveexec" in op or "exec" in args[:1]:
        return "exec"
    if counter and args and args[0] == counter and op in ("s_add_i32", "s_cmp_lt_i32", "s_cmp_ge_i32", "s_cmp_lt_u32", "s_cmp_ge_u32"):
        return "loop"
    if op in MASK_OPS:
        return "mask"
    if op.startswith("s_cmp"):
        return "test"
    if op in ("s_movk_i32", "s_mov_b32"):
        return "const"
    if op in ADDR_OPS:
        return "addr"
    return "ring"


def main():
    lines = open(sys.argv[1]).read().split("\n") if len(sys.argv) > 1 else T.assembly()
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z11k_play_wideILb0EE"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    labels = {m.group(1): i for i in range(start, end) for m in [re.match(r"^(\.LBB\d+_\d+):", lines[i])] if m}
    heads = [i for i in range(start, end) if "=>This Loop Header: Depth=1" in lines[i]]
    found = None
    for k, h in enumerate(heads):
        stop = heads[k + 1] if k + 1 < len(heads) else end
        body = [lines[i].split()[0] for i in range(h, stop) if T.is_ins(lines[i])]
        if body.count("global_store_short") == 0 and body.count("global_store_byte") >= 8 and body.count("global_store_dwordx2") >= 4:
            found = h
            break
    if found is None:
        sys.exit("trick-aligned STD loop not found")
    head = re.match(r"^(\.LBB\d+_\d+):", lines[found]).group(1)
    tag = head[2:]                                   # BBn_m as the block comments spell it
    # the blocks of the loop: every block whose comment names this header (as its loop or as the parent of its loop)
    member, cur = set(), False
    for i in range(found, end):
        l = lines[i]
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
            j, text = i, l
            while j + 1 < end and re.match(r"^\s+;", lines[j + 1]):
                j += 1
                text += lines[j]
            cur = i == found or ("Header=%s " % tag) in text + " " or ("Parent Loop %s " % tag) in text + " "
        if cur and T.is_ins(l) and not l.split()[0].startswith(";;#"):
            member.add(i)
    # the fall-through walk of trick_loop_isa.py, keeping line numbers
    path, i = [], found + 1
    while True:
        l = lines[i]
        if T.is_ins(l) and not l.split()[0].startswith(";;#"):
            f = l.split()
            path.append(i)
            if f[0].startswith(("s_cbranch", "s_branch")) and f[1] == head:
                break
            if f[0] == "s_branch":
                i = labels[f[1]]
                continue
        i += 1
    back = lines[path[-1]].split()
    cmp_ = next((lines[p].replace(",", " ").split() for p in reversed(path[:-1]) if lines[p].split()[0].startswith("s_cmp")), None)
    counter = cmp_[1] if cmp_ and back[0].startswith("s_cbranch_scc") else None
    on_path = set(path)
    cuts = [k for k, p in enumerate(path) if re.match(r"\s*v_and_or_b32 v\d+, v\d+, 32, v\d+", lines[p])][:4]
    bounds = [0] + [c + 1 for c in cuts[:3]] + [len(path)]
    regions = [("card %d%s" % (c, " (first-card fetch region inside)" if c == 0 else
                               " (pick, trick end, finish / renewal region, next lead's mask, stores)" if c == 3 else ""),
                path[bounds[c]:bounds[c + 1]], True) for c in range(4)]
    off = sorted(member - on_path)
    # the blocks off the path, split where a branch of the path enters them (in layout order: ring drain, lineless lane)
    entries = sorted((labels[lines[q].split()[1]], lines[q].strip()) for q in path[:-1]
                     if lines[q].split()[0].startswith("s_cbranch") and labels[lines[q].split()[1]] not in on_path and
                     not any(labels[lines[q].split()[1]] < p2 <= labels[lines[q].split()[1]] + 2 for p2 in on_path))
    for k, (at, how) in enumerate(entries):
        nxt = entries[k + 1][0] if k + 1 < len(entries) else end
        run = [p for p in off if at <= p < nxt]
        if run:
            regions.append(("off the fall-through path, %d instructions, entered by: %s" % (len(run), how), run, False))
    rest = [p for p in off if not entries or p < entries[0][0]]
    if rest:
        regions.append(("off the fall-through path, %d instructions, not entered from the path directly" % len(rest), rest, False))
    total = collections.Counter()
    print("loop header %s: %d instructions on the fall-through path, %d more in blocks of the loop off it" % (head, len(path), len(off)))
    for name, idx, usual in regions:
        print("\n-- %s --" % name)
        c = collections.Counter()
        for p in idx:
            ins = lines[p].strip()
            if not ins.startswith(("s_", "v_readlane", "v_writelane", "v_readfirstlane")):
                continue
            k = classify(ins, head, counter)
            c[k] += 1
            note = ""
            if ins.startswith(("s_cbranch", "s_branch")) and usual:
                note = "   <- TAKEN on the usual path" if ins.split()[1] == head else "   <- not taken on the usual path"
            print("  %-5s %s%s" % (k, ins.split(";")[0].strip(), note))
        valu = sum(1 for p in idx if lines[p].strip().startswith("v_") and not lines[p].strip().startswith(("v_readlane", "v_writelane", "v_readfirstlane")))
        print("  = " + ", ".join("%s %d" % kv for kv in sorted(c.items())) + "; vector ALU %d, all %d" % (valu, len(idx)))
        if usual:
            total.update(c)
    is_br = lambda p: lines[p].split()[0].startswith(("s_cbranch", "s_branch"))
    salu = sum(1 for p in path if lines[p].split()[0].startswith("s_") and not is_br(p) and lines[p].split()[0] not in ("s_waitcnt", "s_nop"))
    br = sum(1 for p in path if is_br(p))
    # taken on this walk: the unconditional ones it followed and whatever goes back to the header
    taken = sum(1 for p in path if is_br(p) and (lines[p].split()[0] == "s_branch" or lines[p].split()[1] == head))
    print("\nfall-through path by class (the exec and test classes include their branches): " + ", ".join("%s %d" % kv for kv in sorted(total.items())))
    print("fall-through path: scalar ALU %d, branches %d (%d taken), s_waitcnt %d, s_nop %d" % (salu, br, taken, total["wait"], total["pad"]))
    ops = collections.Counter(lines[p].split()[0] for p in path)
    print("fall-through path, store addressing on the vector side: v_lshl_add_u64 %d; stores: %s" % (
        ops["v_lshl_add_u64"], ", ".join("%s %d" % (k, v) for k, v in sorted(ops.items()) if "store" in k)))
    for inst in ("_Z11k_play_wideILb0EE", "_Z11k_play_wideILb1EE"):
        s = next(i for i, l in enumerate(lines) if l.startswith(inst))
        e = next(i for i in range(s, len(lines)) if lines[i].startswith(".Lfunc_end"))
        meta = {k: next((re.search(r"(\d+)", lines[i].split(":")[1]).group(1) for i in range(e, min(e + 80, len(lines))) if lines[i].startswith("; " + k + ":")), "?")
                for k in ("NumVgprs", "Occupancy", "ScratchSize")}
        ins = [lines[i].split()[0] for i in range(s, e) if T.is_ins(lines[i])]
        print("%s: NumVgprs %s, Occupancy %s, ScratchSize %s, scratch instructions %d, v_readlane / v_writelane %d / %d" % (
            "k_play_wide<%s>" % ("false" if "Lb0" in inst else "true"), meta["NumVgprs"], meta["Occupancy"], meta["ScratchSize"],
            sum(1 for o in ins if "scratch_" in o), sum(1 for o in ins if o.startswith("v_readlane")), sum(1 for o in ins if o.startswith("v_writelane"))))


if __name__ == "__main__":
    main()
