#!/usr/bin/env python3
"""Golden fixture of the training side's quantification ("Quantification: the EM in the reference's order"): the REAL
reference's src/get_primary_sam.py is run, unmodified, in the build container, and what it computes and writes is committed as data:

  * EM_meta and EM_trans (G:44-142) directly, on made-up quant_dic dictionaries, with normalize True and False;
  * primary_and_unaligned_chimeric (G:220-478) with a metagenome list, and with {'tpm': 0} and q_mode=True;
  * primary_and_unaligned (G:145-217) with a metagenome list —
    the last three on the SAM text of make_chimeric_train_golden.py with reads added that map to several targets.

It reads alignments through pysam, which this image lacks: the stand-ins of make_read_len_golden.py and what
make_chimeric_train_golden.py puts on top of them are imported, not edited.  Doubles are stored as float.hex.  The number of
iterations is taken by a counting `min` in the module's globals (the EM calls it once per iteration), the dictionaries handed to
EM_meta / EM_trans by a recording wrapper around them, the `Iteration:` lines from the captured stdout.

main() asserts the conditions on the input listed in the test files' docstrings; where the reference's functions do not show a branch
(which of the two stop conditions ended the loop, how many contributions a target takes), it uses a restatement of the EM that is used
for nothing else and is itself checked against what the reference returned.

    python tests/golden/make_quantify_golden.py        -> tests/golden/reference_quantify.json.gz
"""
import contextlib
import gzip
import io
import json
import os
import shutil
import statistics
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_read_len_golden as RL                            # noqa: E402  (the pysam / joblib / sklearn stand-ins)
import make_chimeric_train_golden as CT                      # noqa: E402  (its input, and what its alignments need on top)

W = 64                                                       # NS_EM_CHUNK: the terms the accumulate kernel folds at a time
KINDS = {"meta": (100, 0.01), "trans": (1000, 0.001)}


def restate(read_list, all_t, kind, max_iter=None):
    """the EM restated for the asserts on the input: which condition ended it, and the contributions per target"""
    n_max, factor = KINDS[kind]
    n_max = n_max if max_iter is None else max_iter
    names = list(all_t)
    unique, multi, total = dict.fromkeys(names, 0), {}, 0
    for read, cand in read_list.items():
        w = read[1][1] - read[1][0] if kind == "meta" else 1
        total += w
        if len(cand) == 1:
            unique[cand[0]] += w
        else:
            multi[(read[0], w) if kind == "meta" else read[0]] = cand
    a = {t: 100 / len(names) for t in names}
    diff, branch, n_iter = 100 * len(names), None, 0
    for _ in range(n_max):
        n_iter += 1
        cnt = dict(unique)
        for key, cand in multi.items():
            tot = 0
            for c in cand:
                tot = tot + a[c]
            for c in cand:
                cnt[c] += (key[1] * (a[c] / tot)) if kind == "meta" else a[c] / tot
        new = {t: c * 100 / total for t, c in cnt.items()}
        d = 0
        for t in names:
            d = d + abs(new[t] - a[t])
        a = new
        th = min(a.values()) * factor
        if d <= th:
            branch = "le"
            break
        if diff - d < th:
            branch = "shrink"
            break
        diff = d
    per_target = dict.fromkeys(names, 0)
    for cand in multi.values():
        for c in cand:
            per_target[c] += 1
    return dict(a=a, cnt=cnt, n_iter=n_iter, branch=branch, multi=multi, unique=unique, total=total, per_target=per_target, thres0=min(a.values()) == 0)


class Counter:
    """stands in for `min` in the module's globals: the EM calls it once per iteration (G:81 / G:124), directly behind the `sum` of
    G:75 / G:118 — so the last value of the recording `sum` is that iteration's diff_tmp, and what `min` returns is min(abundance)"""
    def __init__(self):
        self.n = 0
        self.last_sum = None
        self.trace, self.mins = [], []

    def __call__(self, *a, **k):
        self.n += 1
        v = min(*a, **k)
        self.trace.append(self.last_sum)
        self.mins.append(v)
        return v

    def sum(self, *a, **k):
        self.last_sum = sum(*a, **k)
        return self.last_sum


def run_em(G, kind, read_list, all_t, normalize=None, max_iter=None, counter_out=None):
    """the reference's EM on copies of the input: (result, n_iter, Iteration lines).  max_iter: the EM's own `range(0, 100)` /
    `range(0, 1000)` ends there instead (a `range` in the module's globals; every other range is the builtin)"""
    G.min = counter = Counter()
    G.sum = counter.sum
    if max_iter is not None:
        G.range = lambda *a: range(0, max_iter) if a in ((0, 100), (0, 1000)) else range(*a)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            res = G.EM_meta(dict(read_list), dict(all_t)) if kind == "meta" else G.EM_trans(dict(read_list), dict(all_t), normalize)
    finally:
        del G.min, G.sum
        if max_iter is not None:
            del G.range
    lines = "".join(line + "\n" for line in buf.getvalue().splitlines() if line.startswith("Iteration:"))
    if counter_out is not None:
        counter_out.append(counter)
    return res, counter.n, lines


def edge_problems():
    """[(name, kind, quant_dic, all_species, max_iter)]: problems that land on the edges of the stop rule (G:80-84)"""
    out = []
    # no multi-mapping item and a target without a read: the threshold is 0, the second iteration changes nothing, diff_tmp is exactly
    # 0.0 and `diff_tmp <= diff_thres` holds with equality (with `<` the loop would run to its last iteration)
    out.append(("meta_zero_diff", "meta", {("u%d" % i, (i, i + 90 + 11 * i)): ["z%d" % (i % 2)] for i in range(9)}, {"z0": 0, "z1": 0, "z2": 0}, None))
    out.append(("trans_zero_diff", "trans", {("u%d" % i, (0, 50)): ["z%d" % (i % 2)] for i in range(7)}, {"z0": 700, "z1": 900, "z2": 400}, None))
    # the iteration limit below the natural count (main() asserts it is above 3): 1, 2 and 3
    q = {("x%d" % i, (0, 1000)): ["A", "B"] for i in range(90)}
    q.update({("ua%d" % i, (0, 1000)): ["A"] for i in range(7)})
    q.update({("ub%d" % i, (0, 1000)): ["B"] for i in range(3)})
    q[("uc", (0, 1))] = ["C"]
    for k in (1, 2, 3):
        out.append(("meta_max_iter_%d" % k, "meta", q, {"A": 0, "B": 0, "C": 0}, k))
    qt = {("x%d" % i, (0, 1000)): ["A", "B"] for i in range(40)}
    qt.update({("ua%d" % i, (0, 1000)): ["A"] for i in range(5)})
    qt.update({("ub%d" % i, (0, 1000)): ["B", "C", "C"] for i in range(3)})
    qt[("uc", (0, 1))] = ["C"]
    for k in (1, 2, 3):
        out.append(("trans_max_iter_%d" % k, "trans", qt, {"A": 1000, "B": 1500, "C": 700}, k))
    return out


def direct_problems():
    """[(name, kind, quant_dic, all_species)]"""
    out = []
    rng = np.random.default_rng(20261019)
    # ---- trans_300: 300 transcripts, ~4 000 reads; t5 and t77 have no read (threshold 0), t9 has unique reads only (its count is an int),
    # t100 .. t103 take exactly W - 1, W, W + 1 and 3 W + 9 contributions
    n = 300
    names = ["t%d" % i for i in range(n)]
    special = {100: W - 1, 101: W, 102: W + 1, 103: 3 * W + 9}
    kept_out = set(special) | {5, 77, 9}
    free = [i for i in range(n) if i not in kept_out]
    expr = rng.gamma(0.6, 1.0, size=len(free))
    expr /= expr.sum()
    q = {}
    k = 0

    def read_name():
        nonlocal k
        k += 1
        return "r%05d" % k
    for _ in range(2800):
        q[(read_name(), (0, int(rng.integers(200, 3000))))] = ["t%d" % free[int(rng.choice(len(free), p=expr))]]
    for _ in range(7):
        q[(read_name(), (0, 500))] = ["t9"]
    for i in range(1100):
        first = free[int(rng.choice(len(free), p=expr))]
        m = 2 + int(rng.integers(0, 3)) if i % 40 else 5 + int(rng.integers(0, 3))
        cand = [first] + [free[(free.index(first) + 1 + int(rng.integers(0, 6))) % len(free)] for _ in range(m - 1)]
        if i % 97 == 0:
            cand.append(cand[0])                             # a duplicate inside a list
        q[(read_name(), (0, int(rng.integers(200, 3000))))] = ["t%d" % c for c in cand]
    for t, cnt in special.items():
        for j in range(cnt):
            q[(read_name(), (0, 800))] = ["t%d" % t, "t%d" % free[(7 * t + j) % len(free)]]
        for j in range(3):
            q[(read_name(), (0, 800))] = ["t%d" % t]
    # key collisions of EM_trans: one read name, two intervals, both multi-mapping — the later list replaces the earlier one, in its place
    q[("twice", (0, 400))] = ["t1", "t2"]
    q[("between", (0, 400))] = ["t3", "t4"]
    q[("twice", (450, 900))] = ["t2", "t6", "t7"]
    out.append(("trans_300", "trans", q, {nm: 300 + 13 * i for i, nm in enumerate(names)}))
    # ---- one target: every list names it; [A, A] is a list with a duplicate
    out.append(("trans_one", "trans", {("a", (0, 10)): ["only"], ("b", (0, 10)): ["only", "only"], ("c", (5, 9)): ["only"]}, {"only": 1234}))
    out.append(("meta_one", "meta", {("a", (0, 100)): ["sp"], ("b", (0, 250)): ["sp", "sp"]}, {"sp": 0}))
    # ---- no multi-mapping item at all
    out.append(("meta_unique_only", "meta", {("u%d" % i, (i, i + 100 + 7 * i)): ["s%d" % (i % 3)] for i in range(40)}, {"s0": 0, "s1": 0, "s2": 0}))
    # ---- 63, 64, 65 targets
    for n in (63, 64, 65):
        names = ["g%d" % i for i in range(n)]
        q = {}
        for i in range(400):
            a = int(rng.integers(0, n - 1))
            ln = int(rng.integers(300, 9000))
            if i % 3 == 0:
                q[("m%d" % i, (10, 10 + ln))] = [names[a], names[(a + 1 + int(rng.integers(0, 4))) % (n - 1)]]
            else:
                q[("m%d" % i, (10, 10 + ln))] = [names[a]]
        # (the last target has no read: the threshold is 0 for n = 64; for the others it gets one)
        if n != 64:
            q[("last", (0, 50))] = [names[-1]]
        # EM_meta's key is (name, length): two items of one name and one length collide, whatever their intervals
        q[("same_len", (0, 700))] = [names[0], names[1]]
        q[("same_len", (40, 740))] = [names[2], names[3], names[4]]
        out.append(("meta_%d" % n, "meta", q, dict.fromkeys(names, 0)))
    # ---- a metagenome on which all 100 iterations run: two species told apart by few unique bases, a third with a tiny share
    q = {("x%d" % i, (0, 1000)): ["A", "B"] for i in range(900)}
    q.update({("ua%d" % i, (0, 1000)): ["A"] for i in range(66)})
    q.update({("ub%d" % i, (0, 1000)): ["B"] for i in range(34)})
    q[("uc", (0, 1))] = ["C"]
    out.append(("meta_100_iterations", "meta", q, {"A": 0, "B": 0, "C": 0}))
    return out


def hexes(v):
    return float(v).hex()


def pack_quant(qd):
    return [[k[0], k[1][0], k[1][1], list(v)] for k, v in qd.items()]


def extra_reads(m):
    """reads added to the chimeric input so that its quant_dic has multi-mapping items; -> ([Rec], {what: [names]})"""
    r = m.rng
    recs, tags = [], {}

    def rec(name, flag, rname, pos, cigar, nm=3):
        return CT.Rec((name, flag, rname, pos, cigar, "*"), {"NM": nm})

    def add(what, name, rows):
        tags.setdefault(what, []).append(name)
        recs.extend(rows)
    others = {"spA_1": "spB_1", "spA_2": "spB_1", "spB_1": "spA_1"}
    for i in range(120):
        ref = CT.REFS[int(r.integers(0, 3))][0]
        a, clip, tail = int(r.integers(200, 1500)), int(r.integers(0, 60)), int(r.integers(0, 30))
        cigar = ("%dS" % clip if clip else "") + m.body(a) + ("%dS" % tail if tail else "")
        name = "multi%03d" % i
        rows = [rec(name, 0, ref, 700 + i, cigar)]
        n_sec = 1 if i % 15 else 4                           # lists of 2 and of 5 candidates
        for j in range(n_sec):
            rows.append(rec(name, 256 | (16 if j % 2 else 0), others[ref] if j % 2 == 0 else ref, 900 + 3 * i + j, cigar))
        add("multi5" if n_sec == 4 else "multi2", name, rows)
    # a primary with HARD clips: pysam's interval starts at 0, cigar_parser's at the clip — the copy of its own CIGAR does not match
    for i in range(3):
        name = "hardclip%d" % i
        add("hardclip", name, [rec(name, 0, "spA_1", 3000 + i, "30H500M20H"), rec(name, 256, "spB_1", 1200 + i, "30H500M20H")])
    # ... and `=` / X ops, which pysam counts and cigar_parser does not
    add("eqx_primary", "eqxprimary", [rec("eqxprimary", 0, "spA_2", 4000, "5S100M50=3X40M"), rec("eqxprimary", 256, "spB_1", 800, "5S100M50=3X40M")])
    # a key that is assigned again restarts its list: the second primary of this name and interval drops what was appended
    add("restart", "restart", [rec("restart", 0, "spA_1", 5000, "10S400M"), rec("restart", 256, "spB_1", 1500, "10S400M")])
    recs.append(rec("filler_between", 0, "spA_2", 6000, "300M"))
    add("restart_again", "restart", [rec("restart", 16, "spB_1", 2000, "10S400M")])
    # a later record with an equal key appends, whichever read it follows: this one stands behind ANOTHER read's primary
    add("late_append", "late", [rec("late", 0, "spA_1", 7000, "350M"), rec("filler_late", 0, "spA_2", 7100, "200M"), rec("late", 2048, "spB_1", 2500, "350M5S")])
    # EM_meta's key (name, length): two primaries of one name with intervals of one length, both multi-mapping
    add("same_len", "samelen", [rec("samelen", 0, "spA_1", 8000, "600M"), rec("samelen", 256, "spB_1", 2600, "600M"),
                                rec("samelen", 0, "spA_2", 8100, "25S600M"), rec("samelen", 256, "spB_1", 2700, "25S600M"), rec("samelen", 256, "spA_1", 8200, "25H600M")])
    return recs, tags


def main():
    sys.dont_write_bytecode = True
    files, written = {}, {}
    dumped, KernelDensity, joblib = RL.install_standins(files, written)
    CT.extend_standin()
    if CT.REF_SRC not in sys.path:
        sys.path.insert(0, CT.REF_SRC)
    import get_primary_sam as G

    # ---- EM_meta / EM_trans directly ------------------------------------------------------------------------------------------------------
    direct = []
    seen_branches, sizes = set(), set()
    for name, kind, q, all_t, max_iter in [p + (None,) for p in direct_problems()] + edge_problems():
        R = restate(q, all_t, kind, max_iter)
        sizes.add(len(all_t))
        for normalize in ((True, False) if kind == "trans" else (None,)):
            seen_counter = []
            res, n_iter, lines = run_em(G, kind, q, all_t, normalize, max_iter, seen_counter)
            assert n_iter == R["n_iter"], (name, n_iter, R["n_iter"])
            trace, mins = seen_counter[0].trace, seen_counter[0].mins
            assert len(trace) == len(mins) == n_iter and lines.startswith("Iteration: 0, Diff: " + str(trace[0]) + "\n")
            if max_iter is not None:
                assert n_iter == max_iter and R["branch"] is None and restate(q, all_t, kind)["n_iter"] > 3, name
            if name.endswith("_zero_diff"):
                assert n_iter == 2 and trace[1] == 0.0 and mins[1] == 0 and R["branch"] == "le" and not R["multi"] and R["thres0"], name
            if kind == "meta":
                assert list(res) == list(all_t) and all(res[t].hex() == R["a"][t].hex() for t in res), name
                result = [[t, hexes(v)] for t, v in res.items()]
            else:
                assert all(float(res[t][0]).hex() == float(R["cnt"][t]).hex() and type(res[t][0]) is type(R["cnt"][t]) for t in res), name
                result = [[t, repr(c), hexes(c), hexes(tpm)] for t, (c, tpm) in res.items()]
            assert lines.count("\n") == (n_iter + (9 if kind == "meta" else 49)) // (10 if kind == "meta" else 50)
            direct.append(dict(name=name, kind=kind, normalize=normalize, items=pack_quant(q), targets=[[t, v] for t, v in all_t.items()], result=result,
                               n_iter=n_iter, lines=lines, branch=R["branch"], max_iter=max_iter, trace=[hexes(v) for v in trace],
                               mins=[hexes(v) for v in mins], multi_keys=[list(k) if kind == "meta" else k for k in R["multi"]],
                               unique=[R["unique"][t] for t in all_t], total=R["total"], per_target=[R["per_target"][t] for t in all_t]))
        seen_branches.add(R["branch"])
        if name == "trans_300":
            pt = R["per_target"]
            assert R["thres0"] and R["n_iter"] < 1000 and R["branch"] is not None, (R["n_iter"], R["branch"])
            assert [pt["t%d" % t] for t in (100, 101, 102, 103)] == [W - 1, W, W + 1, 3 * W + 9]
            assert pt["t9"] == 0 and type(R["cnt"]["t9"]) is int and R["cnt"]["t9"] == 7 and R["unique"]["t5"] == 0 and pt["t5"] == 0
            assert list(R["multi"]).index("twice") < list(R["multi"]).index("between") and R["multi"]["twice"] == ["t2", "t6", "t7"]
            assert any(len(c) == 2 for c in R["multi"].values()) and any(len(c) >= 5 for c in R["multi"].values())
            assert any(len(set(c)) < len(c) for c in R["multi"].values())
            assert len(q) <= 5000 and R["total"] == len(q)
        if name == "meta_100_iterations":
            assert R["n_iter"] == 100 and R["branch"] is None
        if name == "meta_unique_only":
            assert not R["multi"]
        if name.startswith("meta_6"):
            assert R["multi"][("same_len", 700)] == [t for t in list(all_t)[2:5]]
    assert seen_branches >= {"le", "shrink", None} and sizes >= {1, 63, 64, 65, 300}, (seen_branches, sizes)

    # ---- the three end-to-end runs ----------------------------------------------------------------------------------------------------------
    reads, everything, tags = CT.build_input()
    m = CT.Maker(77)
    more, more_tags = extra_reads(m)
    everything = everything[:-1] + more + everything[-1:]
    files["training.sam"] = (CT.REFS, everything)
    seen = {}
    em_meta, em_trans = G.EM_meta, G.EM_trans

    def rec_meta(qd, sp):
        seen["quant"], seen["targets"] = pack_quant(qd), [[t, v] for t, v in sp.items()]
        return em_meta(qd, sp)

    def rec_trans(qd, sp, normalize):
        seen["quant"], seen["targets"] = pack_quant(qd), [[t, v] for t, v in sp.items()]
        return em_trans(qd, sp, normalize)
    G.EM_meta, G.EM_trans = rec_meta, rec_trans
    expected = {"spA": 60.0, "spB": 40.0}
    e2e = {}
    work = tempfile.mkdtemp(prefix="nsq_")
    cwd = os.getcwd()
    try:
        os.chdir(work)
        for key in ("chimeric_meta", "chimeric_trans_q", "primary_meta"):
            seen.clear()
            G.min = counter = Counter()
            buf = io.StringIO()
            meta_list = {"tpm": 0} if key == "chimeric_trans_q" else {s: {"expected": v} for s, v in expected.items()}
            with contextlib.redirect_stdout(buf):
                if key == "chimeric_meta":
                    G.primary_and_unaligned_chimeric("training.sam", "training", meta_list)
                elif key == "chimeric_trans_q":
                    G.primary_and_unaligned_chimeric("training.sam", "training", meta_list, q_mode=True)
                else:
                    G.primary_and_unaligned("training.sam", "training", meta_list)
            del G.min
            with open("training_quantification.tsv") as f:
                tsv = f.read()
            os.remove("training_quantification.tsv")
            lines = "".join(line + "\n" for line in buf.getvalue().splitlines() if line.startswith("Iteration:"))
            R = restate({(q[0], (q[1], q[2])): q[3] for q in seen["quant"]}, dict((t, v) for t, v in seen["targets"]), "trans" if key == "chimeric_trans_q" else "meta")
            d = e2e[key] = dict(quant=seen["quant"], targets=seen["targets"], tsv=tsv, lines=lines, n_iter=R["n_iter"],
                                multi_keys=[list(k) if isinstance(k, tuple) else k for k in R["multi"]])
            if key != "chimeric_trans_q":
                assert counter.n == R["n_iter"] + 1                      # (+ min(variations))
                var = [meta_list[s]["variation"] for s in meta_list]
                d["variation"] = [hexes(min(var)), hexes(max(var)), hexes(statistics.median([abs(v) for v in var]))]
                d["abundance"] = [[s, hexes(meta_list[s]["real"])] for s in meta_list]
                assert tsv == "Species\tAbundance\n" + "".join(s + "\t" + str(R["a"][s]) + "\n" for s in R["a"])
            else:
                assert counter.n == R["n_iter"]
                assert not os.path.exists("training_chimeric_info")
            if key == "chimeric_meta":
                with open("training_chimeric_info") as f:
                    d["chimeric_info"] = f.read()
                os.remove("training_chimeric_info")
                assert "Shrinkage rate (beta):\t" in d["chimeric_info"]
            lens = [len(q[3]) for q in seen["quant"]]
            assert 2 in lens and max(lens) >= 5 and any(len(set(q[3])) < len(q[3]) for q in seen["quant"]), key
            qd = {(q[0], (q[1], q[2])): q[3] for q in seen["quant"]}
            name_of = (lambda n: n) if key == "chimeric_trans_q" else (lambda n: "_".join(n.split("_")[:-1]))
            assert qd[("restart", (10, 410))] == [name_of("spB_1")]                                       # restarted
            assert qd[("late", (0, 350))] == [name_of("spA_1"), name_of("spB_1")]                         # appended behind another read
            assert all(qd[("hardclip%d" % i, (0, 500))] == [name_of("spA_1")] for i in range(3))          # the hard-clipped copy does not match
            assert qd[("eqxprimary", (5, 198))] == [name_of("spA_2")]
            assert qd[("samelen", (0, 600))] == [name_of("spA_1"), name_of("spB_1")] and len(qd[("samelen", (25, 625))]) == 3
            if key == "chimeric_trans_q":
                assert R["multi"]["samelen"] == ["spA_2", "spB_1", "spA_1"]
            else:
                assert R["multi"][("samelen", 600)] == ["spA", "spB", "spA"]
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
        G.EM_meta, G.EM_trans = em_meta, em_trans
    fixture = dict(W=W, refs=[list(r) for r in CT.REFS], sam=CT.sam_text(CT.REFS, everything), expected=expected, direct=direct, e2e=e2e, tags=more_tags)
    out = os.path.join(HERE, "reference_quantify.json.gz")
    with gzip.GzipFile(out, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(fixture).encode())
    print("written", out, os.path.getsize(out), "bytes;", [(d["name"], d["normalize"], d["n_iter"], d["branch"]) for d in direct],
          {k: (v["n_iter"], len(v["quant"]), len(v["multi_keys"])) for k, v in e2e.items()})


if __name__ == "__main__":
    main()
