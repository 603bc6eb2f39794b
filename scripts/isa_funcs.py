#!/usr/bin/env python3
"""Do two device-ISA listings of the engine hold the same functions?  scripts/isa_funcs.py <a.s> <b.s>
When scripts/isa_hash.sh differs only because templates were instantiated in another order (the functions are emitted in that order, and
the local labels carry the function's number), the multiset of (name, body) with those numbers taken out is still identical — and so is
everything outside the functions (kernel descriptors, metadata), compared as sorted lines.  A listing:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S -o a.s nanosim_amd/csrc/nanosim_amd.hip"""
import collections, hashlib, re, sys

NUMBERED = re.compile(r"(\.L)?(BB|func_end|func_begin|tmp|JTI|CPI)\d+")       # .LBB469_3, "Header=BB469_14" in a comment, .Lfunc_end469


def read(path):
    funcs, rest, cur, name = collections.Counter(), [], None, None
    for ln in open(path):
        if "__hip_cuid_" in ln:
            continue
        ln = re.sub(r"[ \t]+;", " ;", NUMBERED.sub(r"\2", ln))      # (the comment column moves with the width of the label's number)
        m = re.search(r"; -- Begin function (\S+)", ln)
        if m and cur is None:
            name, cur = m.group(1), []
        if cur is None:
            rest.append(ln)
            continue
        cur.append(ln)
        if "; -- End function" in ln:
            funcs[(name, hashlib.md5("".join(cur).encode()).hexdigest())] += 1
            cur = None
    return funcs, sorted(rest)


(fa, ra), (fb, rb) = read(sys.argv[1]), read(sys.argv[2])
for name, _ in fa - fb: print("differs or only in", sys.argv[1], name)
for name, _ in fb - fa: print("differs or only in", sys.argv[2], name)
same = fa == fb and ra == rb
print("%d / %d functions, %s" % (sum(fa.values()), sum(fb.values()),
                                 "identical bodies and metadata" if same else "DIFFERENT" + ("" if ra == rb else " (also outside the functions)")))
sys.exit(0 if same else 1)
