#!/usr/bin/env python3
"""Static view of one kernel's ISA: instructions per basic block by class (VALU / SALU / DS / VMEM / SMEM / branch), so that the tile loop
of a record kernel can be read without a GPU.  scripts/isa_blocks.py <file.s> <mangled-name-substring> [--dump LABEL | --path PATH]
Next to the classes every block lists the vector instructions that do no work on data: lane = v_readlane / v_writelane / v_readfirstlane
(wave-uniform values and SGPR spills), mov = v_mov, and the s_nop that follow them.  --path sums ONE path through the function, e.g. the
blocks a tile without rare input runs through: PATH = block numbers separated by commas (113 = .LBB<f>_113); "135>140" counts block 135 up
to and including its branch to .LBB<f>_140, a plain number the whole block."""
import re, sys
src, pat = sys.argv[1], sys.argv[2]
dump = sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--dump" else None
path = sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--path" else None
lines = open(src).read().split("\n")
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(pat) + r"\S*:", l))
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
blocks, cur = [], ["entry", []]
for l in lines[start + 1:end]:
    m = re.match(r"^(\.LBB\S+):", l)
    if m:
        blocks.append(cur); cur = [m.group(1), []]
        continue
    t = l.strip()
    if not t or t.startswith(";") or t.startswith("."): continue
    cur[1].append(t)
blocks.append(cur)
def cls(op):
    if op.startswith("v_"): return "VALU"
    if op.startswith("ds_"): return "DS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")): return "VMEM"
    if op.startswith(("s_load", "s_buffer_load", "s_store")): return "SMEM"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")): return "BR"
    if op.startswith(("s_waitcnt", "s_nop")): return "WAIT"
    return "SALU"
def sub(op):
    """the vector instructions that do no work on data: lane traffic of wave-uniform values / SGPR spills, and register moves"""
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")): return "lane"
    if op.startswith(("v_mov_b32", "v_mov_b64", "v_accvgpr")): return "mov"
    if op.startswith("s_nop"): return "nop"
    return None
def count(ins, c):
    for t in ins:
        for k in (cls(t.split()[0]), sub(t.split()[0])):
            if k: c[k] = c.get(k, 0) + 1
if path is not None:
    by_no = {name.rsplit("_", 1)[-1]: ins for name, ins in blocks}
    c, n = {}, 0
    for el in path.split(","):
        no, _, to = el.partition(">")
        ins = by_no[no]
        if to:
            cut = next(i for i, t in enumerate(ins) if t.startswith(("s_cbranch", "s_branch")) and t.split()[-1].rsplit("_", 1)[-1] == to)
            ins = ins[:cut + 1]
        count(ins, c); n += len(ins)
    print("PATH %d blocks %d instructions  %s" % (len(path.split(",")), n, " ".join("%s=%d" % kv for kv in sorted(c.items()))))
    sys.exit(0)
tot = {}
for name, ins in blocks:
    c = {}
    for t in ins:
        k = cls(t.split()[0]); c[k] = c.get(k, 0) + 1; tot[k] = tot.get(k, 0) + 1
        k = sub(t.split()[0])
        if k: c[k] = c.get(k, 0) + 1; tot[k] = tot.get(k, 0) + 1
    tgt = [t.split()[-1] for t in ins if t.startswith(("s_cbranch", "s_branch"))]
    if dump is None:
        print("%-14s %4d  %s  -> %s" % (name, len(ins), " ".join("%s=%d" % kv for kv in sorted(c.items())), ",".join(tgt)))
    elif name == dump:
        print("\n".join(ins))
if dump is None: print("TOTAL", tot)
