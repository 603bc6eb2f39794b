#!/usr/bin/env python3
"""Mutation audit of the training side's walk headers and of the event chains' packer and look-ups ("What the
mutation audit leaves"), on the CPU host build.

The GPU tests of the training calls compare the device with the host build of the SAME header, so a mistake in the shared walk is wrong
on both sides at once; what pins the walk is the reference fixtures, the oracle and the hand cases.  This tool measures how tightly:
it changes ONE operator of a header in a scratch copy of the tree, runs that header's `-m "not gpu"` tests against the copy, and lists
the mutants the tests did not notice.

    python scripts/mutation_audit.py nanosim_amd/csrc/ns_em.h tests/test_quantify.py
    python scripts/mutation_audit.py --all [--classes rel,lit,logic] [--jobs N] [--timeout S] [--log FILE]
    python scripts/mutation_audit.py --chain            ns_pack.h and the thread-per-read part of ns_chain.h, on tests/chain_host.hip
    python scripts/mutation_audit.py --chain-wave       the wave-per-read part of ns_chain.h, on tests/chain_wave_host.hip (64 host threads
                                                        per mutant: --jobs 2)
    python scripts/mutation_audit.py --gz               ns_gz.h (the code builder and the block walk of the compressed output) on
                                                        tests/gz_wave_host.cpp, 64 host threads per mutant like --chain-wave

Mutation classes: rel   `<` <-> `<=`, `>` <-> `>=`                                   (the default)
                  lit   an integer literal inside a condition or an index expression, +1 and -1
                  logic `&&` <-> `||`
Per header it prints the number of mutants, how many were killed, and one line per survivor: `file:line col op | source line`.
A mutant that runs into its time limit counts as killed (a flipped loop bound need not terminate).  A mutant the host compiler rejects
is no mutant (a `<` of a template argument list, say) and is left out.  Text the host build never compiles — the true branch of an
`#if` on __HIP_DEVICE_COMPILE__, or on __HIPCC__ where the header's unit is built by g++, and, under --chain, the wave-per-read functions
of ns_chain.h (tests/chain_host.hip leaves them out) — is listed apart as "device-only, not auditable on the host", and is not counted.
--chain-wave audits exactly that part of ns_chain.h, from the DEVICE_ONLY_FROM marker to the end of the file, on the build that runs
it on a lock-step wavefront of 64 host threads (tests/chain_wave_host.hip); a mutant whose lanes diverge ends with the wave's message
and counts as killed, like one that runs into its time limit.

Mutants run on the CPU host build only: a mutant is by construction code that may read or loop out of bounds.  Nothing here compiles
for a GPU, imports an engine or runs a test marked gpu.  The working tree is never touched: every worker mutates its own copy."""
import argparse
import concurrent.futures
import os
import re
import shutil
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "nanosim_amd/csrc/"
# header -> (the host translation unit that includes it, the CPU test files that run its walk).  tests/mixfit_host.cpp is compiled as the
# tests compile it: HIP source for the host alone (hipcc --cuda-host-only: no code object for any GPU is made)
TRAINING = {
    CSRC + "ns_chimeric.h": ("tests/chimeric_host.cpp", ["tests/test_chimeric_train.py"]),
    CSRC + "ns_cs_hist.h": ("tests/cs_hist_host.cpp", ["tests/test_characterize.py", "tests/test_basequal.py"]),
    # (the two headers written against an abstract wavefront: the one-lane build first, then 64 lanes in lock step, tests/wave64_host.h —
    # 64 host threads per mutant, so few --jobs; a mutant whose lanes diverge ends with the wave's message, one that loops at its time limit)
    CSRC + "ns_bam.h": ("tests/bam_host.cpp", ["tests/test_bam.py", "tests/test_bam_wave64.py"]),
    CSRC + "ns_calmd.h": ("tests/calmd_host.cpp", ["tests/test_calmd.py", "tests/test_calmd_wave64.py"]),
    CSRC + "ns_em.h": ("tests/em_host.cpp", ["tests/test_quantify.py"]),
    CSRC + "ns_hp_hist.h": ("tests/hp_train_host.cpp", ["tests/test_hp_train.py"]),
    CSRC + "ns_ir_train.h": ("tests/ir_train_host.cpp", ["tests/test_ir_train.py"]),
    CSRC + "ns_maf_best.h": ("tests/maf_best_host.cpp", ["tests/test_besthit.py"]),
    CSRC + "ns_qual_hist.h": ("tests/qual_hist_host.cpp", ["tests/test_basequal.py"]),
    CSRC + "ns_read_len.h": ("tests/read_len_host.cpp", ["tests/test_read_lengths.py", "tests/test_chimeric_train.py"]),
    CSRC + "ns_sam_pairs.h": ("tests/sam_pairs_host.cpp", ["tests/test_sam_pairs.py", "tests/test_read_lengths.py", "tests/test_chimeric_train.py"]),
    CSRC + "ns_mixfit.h": ("tests/mixfit_host.cpp", ["tests/test_mixfit.py"]),
    # (the ranking of k_sam_sep_count / k_sam_sep_write in ns_train.h has no host build: DESIGN section 9 lists its conditions by hand)
    CSRC + "ns_sam_index.h": ("tests/sam_index_host.cpp", ["tests/test_sam_index.py"]),
}
# the event chains: the packer of the chain tables and the thread-per-read chains with their look-ups, compiled for the host by
# tests/chain_host.hip (hipcc --cuda-host-only -DNS_HOST_TEST); the tests that decide AT the thresholds first (a mutant dies at the first failure)
CHAIN_TESTS = ["tests/test_lookup_probe.py", "tests/test_chain_edges.py", "tests/test_chain_host.py", "tests/test_chain_guide.py"]
CHAIN = {
    CSRC + "ns_pack.h": ("tests/chain_host.hip", CHAIN_TESTS + ["tests/test_qual_probe.py"]),      # (+ the base-quality tables of the same header)
    CSRC + "ns_chain.h": ("tests/chain_host.hip", CHAIN_TESTS),
}
# the wave-per-read chains (ns_chain.h from the DEVICE_ONLY_FROM marker on) on the lock-step wavefront of tests/wave64_host.h; the test file
# has its edge tests first
CHAIN_WAVE = {CSRC + "ns_chain.h": ("tests/chain_wave_host.hip", ["tests/test_chain_wave64.py"])}
# the compressed output: the code builder and the block walk of ns_gz.h in the g++ program of tests/gz_wave_host.cpp (the kernels behind
# `#if defined(__HIPCC__)` are listed apart); the builder's file first: it is the cheaper one and decides most mutants
GZ = {CSRC + "ns_gz.h": ("tests/gz_wave_host.cpp", ["tests/test_gz_code_fuzz.py", "tests/test_gz_wave64.py"])}
UNITS = {**TRAINING, **CHAIN, **GZ}
# header -> the text from the first line that holds this marker to the end of the file is `__device__` only
DEVICE_ONLY_FROM = {CSRC + "ns_chain.h": "// ---- cooperative unaligned_error_list"}
SKIP_DIRS = {".git", "__pycache__", "_tmp", ".pytest_cache"}
DEVICE_MACROS = ("__HIP_DEVICE_COMPILE__", "__HIPCC__")


def host_defines(unit: str):
    """which of DEVICE_MACROS the host pass over `unit` defines: g++ none, hipcc --cuda-host-only __HIPCC__ (see syntax_check)"""
    return ("__HIPCC__",) if unit.endswith(("mixfit_host.cpp", ".hip")) else ()


def blank_comments(text: str) -> str:
    """the text with comments, string and character literals replaced by blanks, every other byte in its place"""
    out, i, n = list(text), 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            a, b = i, text.find("\n", i)
            b = n if b < 0 else b
            i = b
        elif text.startswith("/*", i):
            a, b = i, text.find("*/", i + 2)
            b = n if b < 0 else b + 2
            i = b
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c and text[j] != "\n":
                j += 2 if text[j] == "\\" else 1
            a, b = i + 1, min(j, n)                           # (the quotes stay: a literal remains a token)
            i = b + 1
        else:
            i += 1
            continue
        for k in range(a, b):
            if out[k] != "\n":
                out[k] = " "
    return "".join(out)


def device_only_lines(text: str, defined=(), from_marker=None) -> set:
    """the (0-based) lines the host pass leaves out: the true branch of an `#if` on a device macro that pass does not define (or the
    else branch of its negation), and the other branch for a macro it does define; with from_marker, every line from the first one that
    holds it"""
    dev, stack = set(), []                                    # stack of [is_left_out, tests_a_device_macro]
    tail = False
    for ln, line in enumerate(text.split("\n")):
        s = line.strip()
        tail = tail or (from_marker is not None and from_marker in line)
        if tail:
            dev.add(ln)
            continue
        if s.startswith("#if"):
            m = any(k in s for k in DEVICE_MACROS)
            neg = m and ("!defined" in s.replace(" ", "") or s.startswith("#ifndef"))
            neg = neg != (m and any(k in s for k in defined))  # a macro the pass defines: the branches change places
            stack.append([m and not neg, m])
        elif s.startswith("#else") or s.startswith("#elif"):
            if stack:
                stack[-1][0] = stack[-1][1] and not stack[-1][0]
        elif s.startswith("#endif"):
            if stack:
                stack.pop()
        elif any(f[0] for f in stack):
            dev.add(ln)
    return dev


REL = re.compile(r"(?<![<>\-=!])(<=|>=|<|>)(?![<>=])")
LOGIC = re.compile(r"&&|\|\|")
INT = re.compile(r"(?<![\w.])(\d+)(u|ul|ull|ll|l)?(?![\w.])", re.I)
FLIP = {"<": "<=", "<=": "<", ">": ">=", ">=": ">", "&&": "||", "||": "&&"}


def condition_spans(code: str):
    """the spans of `code` that are conditions or index expressions: the parentheses behind if / while / for, brackets, and what stands
    in front of a `?`"""
    spans = []
    for m in re.finditer(r"\b(if|while|for)\s*\(", code):
        depth, j = 1, m.end()
        while j < len(code) and depth:
            depth += {"(": 1, ")": -1}.get(code[j], 0)
            j += 1
        spans.append((m.end(), j))
    for m in re.finditer(r"\[", code):
        depth, j = 1, m.end()
        while j < len(code) and depth:
            depth += {"[": 1, "]": -1}.get(code[j], 0)
            j += 1
        spans.append((m.end(), j))
    for m in re.finditer(r"\?", code):
        j = m.start()
        while j > 0 and code[j - 1] not in ";{}=,\n" or (j > 1 and code[j - 2:j] in ("==", "<=", ">=", "!=")):
            j -= 1
        spans.append((j, m.start()))
    return spans


def mutants_of(text: str, classes):
    """[(offset, old, new, class)] in file order"""
    code = blank_comments(text)
    # the angle brackets of a cast or a standard container are no operators (elsewhere the compile check sorts template brackets out;
    # in device-only text nothing is compiled, so these are taken out here)
    code = re.sub(r"\b(\w+_cast|vector|array|pair|numeric_limits)(\s*)<([^<>;()]*)>", lambda m: m.group(1) + m.group(2) + " " + m.group(3) + " ", code)
    out = []
    line_start = [0] + [m.end() for m in re.finditer("\n", code)]
    pre = set()
    for k, s in enumerate(line_start):
        if code[s:].lstrip(" \t").startswith("#") or code[s:].lstrip(" \t").startswith("template"):
            pre.add(k)
    line_of = lambda off: max(k for k, s in enumerate(line_start) if s <= off) if off < line_start[-1] else len(line_start) - 1
    if "rel" in classes:
        for m in REL.finditer(code):
            if line_of(m.start()) not in pre:
                out.append((m.start(), m.group(1), FLIP[m.group(1)], "rel"))
    if "logic" in classes:
        for m in LOGIC.finditer(code):
            if line_of(m.start()) not in pre:
                out.append((m.start(), m.group(0), FLIP[m.group(0)], "logic"))
    if "lit" in classes:
        spans = condition_spans(code)
        for m in INT.finditer(code):
            if line_of(m.start()) in pre or not any(a <= m.start() < b for a, b in spans):
                continue
            v = int(m.group(1))
            for w in (v + 1, v - 1):
                if w >= 0:
                    out.append((m.start(), m.group(1), str(w), "lit"))
    return sorted(out)


def syntax_check(unit: str):
    """the command that tells whether a mutant is still a program"""
    if unit.endswith(("mixfit_host.cpp", ".hip")):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        hipcc = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
        if not hipcc:
            raise SystemExit("%s needs hipcc for its host build" % unit)
        return [hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-fsyntax-only", "-w"] + (["-DNS_HOST_TEST"] if unit.endswith(".hip") else []) + [unit]
    return ["g++", "-std=c++17", "-fsyntax-only", "-w", unit]


def copy_tree(dst: str) -> None:
    def ignore(d, names):
        return [n for n in names if n in SKIP_DIRS or n.endswith((".pyc", ".o"))]
    shutil.copytree(ROOT, dst, ignore=ignore, symlinks=True)


def run(cmd, cwd, limit):
    """(exit status or None at the time limit, the tail of the output); the whole process group ends with the limit"""
    p = subprocess.Popen(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True,
                         env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    try:
        out, _ = p.communicate(timeout=limit)
        return p.returncode, out.decode(errors="replace")[-600:]
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        return None, "time limit"


class Worker:
    """one scratch copy of the tree"""
    def __init__(self, base: str, k: int):
        self.tree = os.path.join(base, "w%d" % k)
        copy_tree(self.tree)

    def judge(self, header, unit, tests, text, mut, limit):
        off, old, new, _ = mut
        path = os.path.join(self.tree, header)
        with open(path, "w") as f:
            f.write(text[:off] + new + text[off + len(old):])
        try:
            rc, _ = run(syntax_check(unit), self.tree, 120)
            if rc != 0:
                return "invalid"
            rc, _ = run([sys.executable, "-m", "pytest", "-m", "not gpu", "-x", "-q", "-p", "no:cacheprovider"] + list(tests), self.tree, limit)
            return "survived" if rc == 0 else "timeout" if rc is None else "killed"
        finally:
            with open(path, "w") as f:
                f.write(text)


def audit(header, unit, tests, classes, jobs, limit, base, emit, tail_only=False):
    """tail_only: the text from the header's DEVICE_ONLY_FROM marker to the end of the file, and nothing in front of it"""
    with open(os.path.join(ROOT, header)) as f:
        text = f.read()
    lines = text.split("\n")
    tail = device_only_lines(text, (), DEVICE_ONLY_FROM[header]) - device_only_lines(text, ()) if tail_only else None
    dev = device_only_lines(text, host_defines(unit), None if tail_only else DEVICE_ONLY_FROM.get(header))
    where = lambda off: (text.count("\n", 0, off), off - (text.rfind("\n", 0, off) + 1) + 1)
    todo, device = [], []
    for mut in mutants_of(text, classes):
        if tail_only and where(mut[0])[0] not in tail:
            continue
        (device if where(mut[0])[0] in dev else todo).append(mut)
    show = lambda mut: "%s:%d col %d %s -> %s | %s" % (header, where(mut[0])[0] + 1, where(mut[0])[1], mut[1], mut[2], lines[where(mut[0])[0]].strip()[:150])
    t0 = time.time()
    workers = [Worker(base, k) for k in range(min(jobs, max(1, len(todo))))]
    # the unmutated header has to pass, or every verdict below is noise
    t1 = time.time()
    rc, tail = run([sys.executable, "-m", "pytest", "-m", "not gpu", "-x", "-q", "-p", "no:cacheprovider"] + list(tests), workers[0].tree, limit)
    if rc != 0:
        raise SystemExit("%s: its tests do not pass on the unmutated tree:\n%s" % (header, tail))
    # a mutant that needs far longer than the unmutated run (alone; the mutants share the machine) does not terminate
    limit = min(limit, 30.0 + 4.0 * len(workers) * (time.time() - t1))
    free = list(workers)
    verdict = {}

    def one(mut):
        w = free.pop()
        try:
            return mut, w.judge(header, unit, tests, text, mut, limit)
        finally:
            free.append(w)
    with concurrent.futures.ThreadPoolExecutor(len(workers)) as pool:
        for mut, v in pool.map(one, todo):
            verdict[mut] = v
    for w in workers:
        shutil.rmtree(w.tree, ignore_errors=True)
    valid = [m for m in todo if verdict[m] != "invalid"]
    survived = [m for m in valid if verdict[m] == "survived"]
    timed = [m for m in valid if verdict[m] == "timeout"]
    emit("== %s  [%s]  tests: %s" % (header, ",".join(classes), " ".join(tests)))
    emit("   mutants %d, killed %d (of them %d at the time limit), survived %d, device-only and not audited %d, rejected by the compiler %d; %.0f s"
         % (len(valid), len(valid) - len(survived), len(timed), len(survived), len(device), len(todo) - len(valid), time.time() - t0))
    for m in survived:
        emit("   survivor  " + show(m))
    for m in device:
        emit("   device-only, not auditable on the host  " + show(m))
    return len(valid), len(valid) - len(survived), len(survived), len(device)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("header", nargs="?", help="the header to mutate, relative to the repository")
    ap.add_argument("tests", nargs="*", help="the test files to run against every mutant")
    ap.add_argument("--all", action="store_true", help="the training headers with their CPU test files")
    ap.add_argument("--chain", action="store_true", help="ns_pack.h and the thread-per-read part of ns_chain.h with the chain's CPU test files")
    ap.add_argument("--chain-wave", action="store_true", help="the wave-per-read part of ns_chain.h on the 64-lane host build, with tests/test_chain_wave64.py")
    ap.add_argument("--gz", action="store_true", help="ns_gz.h on the 64-lane host program, with tests/test_gz_code_fuzz.py and tests/test_gz_wave64.py")
    ap.add_argument("--classes", default="rel", help="comma-separated: rel, lit, logic (default rel)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per mutant, at most (the limit in use follows the unmutated run's time)")
    ap.add_argument("--log", help="also write the report to this file")
    a = ap.parse_args()
    classes = [c for c in a.classes.split(",") if c]
    if not classes or set(classes) - {"rel", "lit", "logic"}:
        ap.error("classes are rel, lit and logic")
    if (a.all or a.chain or a.chain_wave or a.gz) == bool(a.header):
        ap.error("give a header with its tests, or --all, or --chain, or --chain-wave, or --gz")
    if a.chain_wave and (a.all or a.chain):
        ap.error("--chain-wave audits the other part of a header --chain audits: run it on its own")
    if a.chain_wave:
        plan = [(h, u, t) for h, (u, t) in CHAIN_WAVE.items()]
    elif a.all or a.chain or a.gz:
        plan = [(h, u, t) for h, (u, t) in {**(TRAINING if a.all else {}), **(CHAIN if a.chain else {}), **(GZ if a.gz else {})}.items()]
    else:
        h = os.path.relpath(os.path.abspath(a.header), ROOT)
        if not a.tests:
            ap.error("no test file given")
        unit = UNITS[h][0] if h in UNITS else None
        if unit is None:
            ap.error("%s: no host translation unit known for it (TRAINING, CHAIN, GZ)" % h)
        plan = [(h, unit, [os.path.relpath(os.path.abspath(t), ROOT) for t in a.tests])]
    log = open(a.log, "w") if a.log else None

    def emit(s):
        print(s, flush=True)
        if log:
            log.write(s + "\n")
            log.flush()
    t0 = time.time()
    base = tempfile.mkdtemp(prefix="mutation_audit_")
    tot = [0, 0, 0, 0]
    try:
        for h, u, t in plan:
            for k, v in enumerate(audit(h, u, t, classes, a.jobs, a.timeout, base, emit, tail_only=a.chain_wave)):
                tot[k] += v
    finally:
        shutil.rmtree(base, ignore_errors=True)
    emit("== total: mutants %d, killed %d, survived %d, device-only %d; %.0f s with %d jobs" % (tot[0], tot[1], tot[2], tot[3], time.time() - t0, a.jobs))
    if log:
        log.close()


if __name__ == "__main__":
    main()
