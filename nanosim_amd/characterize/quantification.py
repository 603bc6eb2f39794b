"""Quantification (``EM_meta`` and ``EM_trans`` of src/get_primary_sam.py, G:44-142; ``read_analysis.py quantify`` and ``-q``) is the eighth
piece: the EM over multi-mapping reads that gives the abundance of every species of a metagenome, or count and TPM of every transcript,
``<prefix>_quantification.tsv``.  The reference's loop ends where its ``diff`` stops shrinking, which is in rounding noise, so its result
depends on its summation order; the iterations run on the GPU in exactly that order (``ns_em_quantify``, csrc/ns_em.h) and give the
reference's doubles and its iteration count bit for bit.  This module builds the reference's ``quant_dic`` and ``multi_mapping_list``
with Python dicts, as the reference does, so that its key collisions are kept, computes TPM and writes the file:

    abundance, variation = characterize.quantify("training", "training.sam", eng, "meta", expected={"spA": 60.0, "spB": 40.0})
    characterize.chimeric("training", "training.sam", eng, quantify="meta")     # _chimeric_info with its own shrinkage rate

Deviations: a species of the header that ``expected`` lacks, a species or transcript of an alignment that the header lacks, a total of
2^53 / 100 bases or more and an abundance that is not finite raise ValueError; the sums are CPython's up to 3.11 (from 3.12 on ``sum``
compensates, and the reference's own result changes with it)."""
import ctypes as C
import re
import statistics

import numpy as np

from ._abi import write_text
from .chim_select import CHIM_ALONE, chimeric_records, sa_entries, select_chimeric, species_of_reference
from .sam_text import _CIGAR_TOKEN


class NsEmProblem(C.Structure):
    """mirror of ns_em_problem (include/nanosim_amd.h)"""
    _fields_ = [("n_targets", C.c_uint32), ("n_multi", C.c_uint32), ("multi_off", C.c_void_p), ("target", C.c_void_p), ("weight", C.c_void_p),
                ("unique", C.c_void_p), ("total", C.c_double), ("factor", C.c_double), ("max_iter", C.c_uint32), ("group", C.c_uint32)]


class NsEmResult(C.Structure):
    """mirror of ns_em_result (include/nanosim_amd.h)"""
    _fields_ = [("abundance", C.c_void_p), ("count", C.c_void_p), ("diff_trace", C.c_void_p), ("n_iter", C.c_uint32), ("reserved", C.c_uint32),
                ("n_nonfinite", C.c_uint64), ("ms_kernel", C.c_double)]


EM_KINDS = {"meta": (100, 0.01, 10), "trans": (1000, 0.001, 50)}       # iterations, threshold factor, print cadence (G:63, 81, 76; G:107, 124, 119)


def _parser_interval(cigar: str):
    """(qstart, qend) of cigar_parser (G:16-31) — csrc/ns_chimeric.h, CHIM_PARSER, says what its regular expression sees"""
    items = re.findall(r'(\d+)(\w)', cigar)
    if not items:
        raise ValueError("CIGAR %.60s is not one" % cigar)
    qstart = int(items[0][0]) if items[0][1] in "SH" else 0
    return qstart, qstart + sum(int(n) for n, op in items if op in "MI")


def _pysam_interval(cigar: str):
    """(query_alignment_start, query_alignment_end) as pysam states them: the S ops among the leading clips; start + M + I + `=` + X"""
    ops = _CIGAR_TOKEN.findall(cigar)
    if not ops or "".join(n + o for n, o in ops) != cigar:
        raise ValueError("CIGAR %.60s is not one" % cigar)
    qstart = 0
    for n, op in ops:
        if op == "S":
            qstart += int(n)
        elif op != "H":
            break
    return qstart, qstart + sum(int(n) for n, op in ops if op in "MI=X")


def _alone_winner(ent, ref_ids, nms) -> int:
    """the entry of a read's winning list when that list is one piece that is not the primary (CHIM_ALONE: the device reports the primary
    record for such a read, G:331 needs the piece's interval): the grouping of csrc/ns_chimeric.h restated for these few reads"""
    q = [(int(e["qstart"]), int(e["qend"])) for e in ent]
    r = [(s, s + int(e["rlen"])) for (_, s), e in zip(ref_ids, ent)]
    over = lambda a, b: a[0] < b[1] - 10 and a[1] - 10 > b[0]
    lists = [[0]]
    for e in range(1, len(q)):
        added = False
        for members in lists:
            if not any(over(q[e], q[m]) for m in members) and not any(over(r[e], r[m]) and ref_ids[e][0] == ref_ids[m][0] for m in members):
                members.append(e)
                added = True
        if not added:
            lists.append([e])
    scores = [sum(int(ent[m]["qlen"]) - nms[m] for m in members) for members in lists]
    return lists[scores.index(max(scores))][0]


def quant_items(records, sel, refs, species=None) -> dict:
    """the reference's quant_dic of the chimeric path, {(qname, (qstart, qend)): [target, ...]}, from what select_chimeric returned for
    `records`.  species: {reference name: species} (meta), or None: the reference name itself (trans, G:330 / 354 / 392 / 404).
    A Python dict on purpose — the reference's corners are its dict's:
      * a key that is assigned again restarts its list (G:331 / 355 / 393 are assignments): a later read of the same name and interval,
        or two pieces of one read with one interval, drop what was appended before;
      * a later supplementary or secondary record with equal (qname, (qstart, qend)) appends its target, whatever it is and whichever
        read it follows (G:403-405) — the record a piece was matched to included, so a chosen piece has its own target twice;
      * the primary's interval is pysam's (S clips only, `=` / X counted) while the other records' is cigar_parser's (G:398): a
        hard-clipped copy of the primary's CIGAR does not match."""
    name_of = (lambda n: n) if species is None else (lambda n: species[n])
    ent, ent_off, pieces = sel["ent"], sel["ent_off"], sel["pieces"]
    quant = {}
    at = 0                                                   # the next of sel["others"]
    others, spans, primaries = sel["others"], sel["spans"], sel["primaries"]
    for k, i in enumerate(primaries + [len(records)]):       # (the last round: the records behind the last primary)
        while at < len(others) and others[at] < i:           # the records in front of this primary, in file order (G:397-405)
            o = records[others[at]]
            key = (o.qname, (int(spans["qstart"][at]), int(spans["qend"][at])))
            if key in quant:
                quant[key].append(name_of(o.rname))
            at += 1
        if k == len(primaries):
            break
        r = records[i]
        e0, e1 = int(ent_off[k]), int(ent_off[k + 1])
        sa = sa_entries(r.sa, r.qname) if r.sa is not None else []
        rnames = [r.rname] + [e[0] for e in sa]
        if sel["flags"][k] & CHIM_ALONE:                     # G:325-334: the piece's interval, the PRIMARY's reference
            starts = [(r.rname, r.pos - 1)] + [(e[0], e[1]) for e in sa]
            w = _alone_winner(ent[e0:e1], starts, [r.nm] + [e[4] for e in sa])
            quant[(r.qname, (int(ent["qstart"][e0 + w]), int(ent["qend"][e0 + w])))] = [name_of(r.rname)]
            continue
        for p in pieces[e0:e0 + int(sel["n_pieces"][k])]:    # G:353-355 (G:391-393 without an SA tag: the one piece is the primary)
            e = int(p["entry"])
            quant[(r.qname, (int(ent["qstart"][e0 + e]), int(ent["qend"][e0 + e])))] = [name_of(rnames[e])]
    return quant


def quant_items_primary(records, refs) -> dict:
    """the quant_dic of the non-chimeric primary_and_unaligned (G:169-181), always by species: a primary record assigns
    [(qname, pysam's interval)] = [species], a later supplementary or secondary record with that name and cigar_parser's interval appends"""
    quant = {}
    for r in records:
        if r.flag & 0x4:
            continue
        if not r.flag & (0x100 | 0x800):
            quant[(r.qname, _pysam_interval(r.cigar))] = [species_of_reference(r.rname)]          # G:171: an assignment
        else:
            key = (r.qname, _parser_interval(r.cigar))
            if key in quant:
                quant[key].append(species_of_reference(r.rname))                                  # G:179-181
    return quant


def quant_targets(refs, kind: str, species=None) -> dict:
    """all_species (G:157-161, G:253-261): {species: LN of its last reference} for meta, {reference name: LN} for trans, in @SQ order"""
    if kind == "trans":
        return {name: ln for name, ln in refs}
    return {(species[name] if species is not None else species_of_reference(name)): ln for name, ln in refs}


def em_problem(items: dict, targets, kind: str) -> dict:
    """What EM_meta (G:50-62) / EM_trans (G:95-106) set up from quant_dic: "names" (the targets in order), "unique" (float64),
    "total" (int: every item counts), "keys" (multi_mapping_list's, in its order), "multi_off", "target", "weight".
    multi_mapping_list is keyed by (qname, length) for meta (G:59) and by qname alone for trans (G:103): a later item with the same key
    replaces the candidates and keeps the first one's place — a Python dict does exactly that."""
    if kind not in EM_KINDS:
        raise ValueError("kind must be 'meta' or 'trans'")
    names = list(dict.fromkeys(targets))
    if not names:
        raise ValueError("no target")
    index = {n: i for i, n in enumerate(names)}
    unique = [0] * len(names)
    multi = {}
    total = 0
    for read, cand in items.items():
        for c in cand:
            if c not in index:
                raise ValueError("read %s lies on %s, which is not among the targets" % (read[0], c))
        length = read[1][1] - read[1][0] if kind == "meta" else 1
        total += length
        if len(cand) == 1:
            unique[index[cand[0]]] += length
        else:
            multi[(read[0], length) if kind == "meta" else read[0]] = cand
    if total <= 0:
        raise ValueError("nothing to quantify: total is %d" % total)
    if total * 100 >= 2 ** 53:
        raise ValueError("total of %d: its hundredfold is no exact double" % total)
    multi_off = np.zeros(len(multi) + 1, dtype=np.uint64)
    np.cumsum([len(c) for c in multi.values()], out=multi_off[1:])
    return dict(kind=kind, names=names, unique=np.array(unique, dtype=np.float64), unique_int=unique, total=total, keys=list(multi),
                multi_off=multi_off, target=np.array([index[c] for cand in multi.values() for c in cand], dtype=np.uint32),
                weight=np.array([k[1] if kind == "meta" else 1.0 for k in multi], dtype=np.float64))


def em_call(eng, prob: dict) -> dict:
    """ns_em_quantify on an em_problem: abundance, count (float64 per target), diff_trace, n_iter, n_nonfinite, ms_kernel"""
    max_iter, factor, group = EM_KINDS[prob["kind"]]
    n = len(prob["names"])
    abundance, count, trace = np.zeros(n), np.zeros(n), np.zeros(max_iter)
    P, R = NsEmProblem(), NsEmResult()
    P.n_targets, P.n_multi = n, len(prob["keys"])
    P.multi_off, P.target, P.weight = prob["multi_off"].ctypes.data, prob["target"].ctypes.data, prob["weight"].ctypes.data
    P.unique, P.total, P.factor, P.max_iter, P.group = prob["unique"].ctypes.data, float(prob["total"]), factor, max_iter, group
    R.abundance, R.count, R.diff_trace = abundance.ctypes.data, count.ctypes.data, trace.ctypes.data
    eng._check(eng.L.ns_em_quantify(eng.ctx, C.addressof(P), C.addressof(R)))
    return dict(abundance=abundance, count=count, diff_trace=trace, n_iter=int(R.n_iter), n_nonfinite=int(R.n_nonfinite), ms_kernel=float(R.ms_kernel))


def iteration_lines(kind: str, diff_trace, n_iter: int) -> str:
    """the `Iteration: i, Diff: d` lines the reference prints (G:76-78, G:119-121), from the recorded trace"""
    step = EM_KINDS[kind][2]
    return "".join("Iteration: " + str(i) + ", Diff: " + str(float(diff_trace[i])) + "\n" for i in range(0, n_iter, step))


def em_quantify(eng, items: dict, targets, kind: str, normalize: bool = True) -> dict:
    """EM_meta(items, targets) / EM_trans(items, targets, normalize): "result" is {species: abundance} for meta and
    {transcript: (count, tpm)} for trans — targets is then {transcript: length} —, next to "n_iter", "diff_trace" and "ms_kernel".
    A transcript that stands in no multi-mapping list keeps a Python int as its count, as in the reference (it writes `3`, not `3.0`).
    TPM (G:129-140) is one ordered fold on the host, so that total_rpk is the reference's."""
    prob = em_problem(items, targets, kind)
    got = em_call(eng, prob)
    if got["n_nonfinite"]:
        raise ValueError("%d abundance(s) are not finite after %d iteration(s)" % (got["n_nonfinite"], got["n_iter"]))
    names = prob["names"]
    out = dict(n_iter=got["n_iter"], diff_trace=got["diff_trace"], ms_kernel=got["ms_kernel"])
    if kind == "meta":
        out["result"] = {n: float(v) for n, v in zip(names, got["abundance"])}
        return out
    touched = set(prob["target"].tolist())
    counts = [float(got["count"][t]) if t in touched else prob["unique_int"][t] for t in range(len(names))]
    rpk = [c / targets[n] * 1e3 if normalize else c for n, c in zip(names, counts)]
    total_rpk = 0
    for v in rpk:                                            # (the fold of sum() up to CPython 3.11)
        total_rpk = total_rpk + v
    out["result"] = {n: (c, v * 1e6 / total_rpk) for n, c, v in zip(names, counts, rpk)}
    return out


def format_quantification(kind: str, result: dict) -> str:
    """the text of <prefix>_quantification.tsv: G:418-420 (trans), G:426-430 (meta)"""
    if kind == "trans":
        return "ID\tcount\tTPM\n" + "".join(t + '\t' + str(info[0]) + '\t' + str(info[1]) + '\n' for t, info in result.items())
    return "Species\tAbundance\n" + "".join(k + '\t' + str(v) + '\n' for k, v in result.items())


def abundance_variation(abundance: dict, expected: dict):
    """(low, high, abs-median) of (real - expected) / expected over the species (G:199-212)"""
    for k in abundance:
        if k not in expected:
            raise ValueError("species %s of the header has no expected abundance" % k)          # (a KeyError at G:198 in the reference)
    var = [(v - expected[k]) / expected[k] for k, v in abundance.items()]
    return min(var), max(var), statistics.median([abs(v) for v in var])


def quantify(prefix: str, path: str, eng, kind: str, species=None, expected=None, normalize: bool = True):
    """the reference's quantification-only mode (q_mode of G:220-478; `read_analysis.py quantify`): writes <prefix>_quantification.tsv and
    nothing else.  kind "meta": species = {reference name: species} (default: species_of_reference), expected = {species: percent} gives
    the variation triple; kind "trans": count and TPM per transcript.  -> (result of em_quantify, variation or None)"""
    if kind not in EM_KINDS:
        raise ValueError("kind must be 'meta' or 'trans'")
    refs, records, _, _ = chimeric_records(path)
    if kind == "meta" and species is None:
        species = {name: species_of_reference(name) for name, _ in refs}
    targets = quant_targets(refs, kind, species)
    if kind == "meta" and expected is not None:
        for k in targets:
            if k not in expected:
                raise ValueError("species %s of the header has no expected abundance" % k)
    sel = select_chimeric(eng, refs, records, species if kind == "meta" else None)
    res = em_quantify(eng, quant_items(records, sel, refs, species if kind == "meta" else None), targets, kind, normalize)
    write_text(prefix + "_quantification.tsv", format_quantification(kind, res["result"]))
    variation = abundance_variation(res["result"], expected) if kind == "meta" and expected is not None else None
    return res["result"], variation
