#!/usr/bin/env python3
"""Diagnostic: instruction count of the trick-aligned STD card loop of k_play_wide<false> (play_role, tricks(true_type)).

    python tools/trick_loop_isa.py [file.s]

Without an argument the library's source is compiled to gfx950 assembly with the library's own flags (hipcc -S).
The loop is the depth-1 loop of the kernel that stores eight bytes (action + done of four cards) and no 16-bit trick
row.  Counted: every instruction from the loop header along the FALL-THROUGH side of each conditional branch
(unconditional branches are followed) up to the branch back to the header — the path of a trick in which a game of
the wave ends and every finishing lane holds its next line.  The split is by the end of each card's pick (the
v_and_or ..., 32, ... that closes kth_bit / kth_bit_word): the compiler interleaves neighbouring cards, so the
per-card figures are where the scheduler put the instructions, their sum is exact."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assembly():
    with tempfile.TemporaryDirectory() as t:
        out = os.path.join(t, "tarok_env.s")
        sys.path.insert(0, ROOT)
        from tarok_amd import _native           # the library's own compiler and flags: the count is of the shipped build
        subprocess.check_call([_native.hipcc_path()] + _native.COMPILE_FLAGS + ["-S", "--cuda-device-only", "-o", out, _native.SRC],
                              stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


def is_ins(l):
    s = l.strip()
    return l.startswith("\t") and s and not s.startswith((".", ";"))


def main():
    lines = open(sys.argv[1]).read().split("\n") if len(sys.argv) > 1 else assembly()
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z11k_play_wideILb0EE"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    labels = {m.group(1): i for i in range(start, end) for m in [re.match(r"^(\.LBB\d+_\d+):", lines[i])] if m}
    heads = [i for i in range(start, end) if "=>This Loop Header: Depth=1" in lines[i]]
    found = None
    for k, h in enumerate(heads):
        stop = heads[k + 1] if k + 1 < len(heads) else end
        body = [lines[i].split()[0] for i in range(h, stop) if is_ins(lines[i])]
        if body.count("global_store_short") == 0 and body.count("global_store_byte") >= 8 and body.count("global_store_dwordx2") >= 4:
            found = h
            break
    if found is None:
        sys.exit("trick-aligned STD loop not found")
    head = re.match(r"^(\.LBB\d+_\d+):", lines[found]).group(1)
    path, i, seen = [], found + 1, set()
    while True:
        l = lines[i]
        if is_ins(l):
            f = l.split()
            if f[0] == ";;#ASMSTART" or f[0] == ";;#ASMEND":
                i += 1
                continue
            path.append(l.strip())
            if f[0].startswith(("s_cbranch", "s_branch")) and f[1] == head:
                break
            if f[0] == "s_branch":
                if f[1] in seen:
                    sys.exit("fall-through path loops without reaching the header")
                seen.add(f[1])
                i = labels[f[1]]
                continue
        i += 1
        if i >= end:
            sys.exit("back edge not found on the fall-through path")
    print("loop header %s: %d instructions on the fall-through path, header to back edge" % (head, len(path)))
    cuts = [k for k, p in enumerate(path) if re.match(r"v_and_or_b32 v\d+, v\d+, 32, v\d+", p)]
    prev = 0
    for c, k in enumerate(cuts[:4]):
        print("  up to the end of card %d's pick: %d" % (c, k + 1 - prev))
        prev = k + 1
    print("  after card 3's pick (4th card: trick end, finish, renewal, next lead's mask, stores): %d" % (len(path) - prev))
    c = collections.Counter(p.split()[0] for p in path)
    print("  by opcode:", ", ".join("%s %d" % kv for kv in sorted(c.items(), key=lambda kv: -kv[1])[:24]))
    print("  scratch instructions in the kernel:", sum(1 for i in range(start, end) if is_ins(lines[i]) and "scratch_" in lines[i].split()[0]))


if __name__ == "__main__":
    main()
