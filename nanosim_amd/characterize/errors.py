"""Training side, the histogramming step of the characterisation stage (second half): a drop-in for
``hist(prefix, "bam")`` of src/besthit_to_histogram.py (B:148-486) from the cs strings of the primary alignments on.

The reference walks every alignment in Python (parse_cs B:41-69, then the loop B:316-365) and fills dictionaries; the tables it writes
afterwards (B:366-486) are what ``simulator.py`` reads back as the error model (``read_profile``, src/simulator.py:473-501).  Here the
walk runs on the GPU through the C-ABI (``ns_cs_histograms``: one alignment per thread, include/nanosim_amd.h) and this module does
what is left: getting the cs strings out of a SAM file and formatting the reference's files from the counts, text for text.

    from nanosim_amd import characterize, engine
    eng = engine.Engine(0)
    characterize.hist("training", characterize.cs_from_sam("training_primary.sam"), eng)

    characterize.hist("training", characterize.maf_pairs("training_besthit.maf"), eng, alnm_ftype="maf")      # hist(prefix, "maf"), B:188-315"""
import ctypes as C

import numpy as np

from ._abi import PackedPairs, _pack, _pack_pairs, write_text
from .sam_table import SamTable
from .sam_text import cs_of, sam_lines

DICT_MAX = 1000                      # add_dict ignores larger values (B:15-16)
ERR_ROWS = ("mis", "ins", "del", "mis0", "ins0", "del0")
ERR_COLS = ("mis", "ins", "del")


class NsCsHist(C.Structure):
    """mirror of ns_cs_hist (include/nanosim_amd.h)"""
    _fields_ = [("cap_match2d", C.c_uint32), ("_pad", C.c_uint32), ("match_list", C.c_void_p), ("dic", (C.c_uint64 * 1001) * 5),
                ("error_list", C.c_uint64 * 18), ("first_error", C.c_uint64 * 3), ("max_match", C.c_uint64),
                ("n_match2d_overflow", C.c_uint64), ("n_skip", C.c_uint64), ("ms_kernel", C.c_double)]


def cs_from_sam(path: str):
    """the cs string of every alignment of a SAM text file: the cs:Z tag, else from CIGAR + MD:Z (B:320-324)"""
    if isinstance(path, SamTable):
        return path.cs_from_sam()
    return [cs_of(fld) for fld in sam_lines(path, 11) if fld[5] != "*"]


def _count(call, cap: int) -> dict:
    """count and count_maf: `call(h)` makes the library's call on an NsCsHist; repeated with a larger match matrix while it overflows"""
    while True:
        h = NsCsHist()
        m2 = np.zeros((cap, cap), dtype=np.uint64)
        h.cap_match2d, h.match_list = cap, m2.ctypes.data
        call(h)
        if not h.n_match2d_overflow:
            break
        cap = 1 << int(h.max_match).bit_length()                       # the matrix has to hold index max_match
    return dict(dic=np.ctypeslib.as_array(h.dic).copy(), match_list=m2, error_list=np.ctypeslib.as_array(h.error_list).copy().reshape(6, 3),
                first_error=np.ctypeslib.as_array(h.first_error).copy(), max_match=int(h.max_match), ms_kernel=float(h.ms_kernel))


def count(eng, cs_list, cap: int = 2048) -> dict:
    """the counts of hist()'s loop for these alignments, from the GPU (ns_cs_histograms)"""
    data, off = _pack(cs_list)

    def call(h):
        eng._check(eng.L.ns_cs_histograms(eng.ctx, data.ctypes.data, int(off[-1]), off.ctypes.data, len(off) - 1, C.byref(h)))
        if h.n_skip:
            raise ValueError("long-form cs strings (`=` items) are not supported: the reference's parse_cs loses the pairing of its two "
                             "lists on them (src/besthit_to_histogram.py:49-65)")
    return _count(call, cap)


def s_line_pairs(path: str, sequences: bool = True):
    """the `s` lines of a MAF text file two by two, split at blanks; every other line is skipped.  ValueError: an `s` line without its
    partner (behind the last pair) and, with `sequences`, a pair without aligned sequences or whose reference sequence is the longer"""
    pend = None
    with open(path) as f:
        for line in f:
            if not line.startswith("s ") and not line.startswith("s\t"):
                continue
            r = line.split()
            if pend is None:
                pend = r
                continue
            r, q, pend = pend, r, None
            if sequences and (len(r) < 7 or len(q) < 7 or len(r[6]) > len(q[6])):
                raise ValueError("%s: not two `s` lines with an aligned sequence each (the reference would stop with an IndexError)" % path)
            yield r, q
    if pend is not None:
        raise ValueError("%s: an `s` line without its partner (odd number of `s` lines)" % path)


def maf_pairs(path: str):
    """[(reference line, query line)] of `<prefix>_besthit.maf` as hist(prefix, "maf") reads it (B:190-198): two `s` lines per alignment;
    field 7 of each is the aligned sequence (the upper-casing is done by the counting walk).  The file get_besthit_maf writes holds `s`
    lines only, and the reference assumes that; here everything else a MAF file may carry (`#` headers, `a score=` lines, blank
    separators) is skipped, and an `s` line without its partner is a ValueError."""
    return [(r[6], q[6][:len(r[6])]) for r, q in s_line_pairs(path)]                   # (the walk runs over len(ref), B:203)


def count_maf(eng, pairs, cap: int = 2048) -> dict:
    """the counts of hist()'s MAF loop for these alignments, from the GPU (ns_maf_histograms)"""
    ref, qry, off = _pack_pairs(pairs) if isinstance(pairs, PackedPairs) else _pack_pairs([a for a, _ in pairs], [b for _, b in pairs])
    return _count(lambda h: eng._check(eng.L.ns_maf_histograms(eng.ctx, ref.ctypes.data, qry.ctypes.data, int(off[-1]), off.ctypes.data,
                                                               len(off) - 1, C.byref(h))), cap)


def _dict_len(cnt, initial):
    nz = np.nonzero(cnt)[0]
    return max(initial, int(nz[-1]) + 1 if len(nz) else 0)


def format_tables(t: dict) -> dict:
    """{file suffix: text} exactly as hist() writes them (B:366-486) from the counts"""
    dic, m2 = t["dic"], t["match_list"]
    out = {}
    totals = {}
    for w, name, head, initial in ((0, "_match.hist", "Matches", 150), (2, "_mis.hist", "Mismatches", 30), (3, "_ins.hist", "Insertions", 30),
                                   (4, "_del.hist", "Deletions", 30)):
        n = _dict_len(dic[w], initial)
        lines = ["number of bases\t%s:\n" % head]
        tot = 0
        for key in range(n):
            lines.append(str(key) + "\t" + str(int(dic[w][key])) + "\n")
            tot += key * int(dic[w][key])
        out[name] = "".join(lines)
        totals[w] = tot
    total_match, total_mis, total_ins, total_del = totals[0], totals[2], totals[3], totals[4]
    den = total_mis + total_match + total_del
    out["_error_rate.tsv"] = ("Mismatch rate:\t" + str(total_mis * 1.0 / den) + '\n' + "Insertion rate:\t" + str(total_ins * 1.0 / den) + '\n' +
                              "Deletion rate:\t" + str(total_del * 1.0 / den) + '\n' +
                              "Total error rate:\t" + str((total_mis + total_ins + total_del) * 1.0 / den) + '\n')
    # error Markov model (B:404-422)
    err = t["error_list"]
    first = [int(x) for x in t["first_error"]]
    num_first = sum(first)
    s = "succedent \tmis\tins\tdel\n"
    s += "start\t" + str(first[0] * 1.0 / num_first) + "\t" + str(first[1] * 1.0 / num_first) + "\t" + str(first[2] * 1.0 / num_first)
    for r, x in enumerate(ERR_ROWS):
        s += "\n" + x
        pred = int(err[r].sum())
        for c in range(3):
            s += "\t" + ("0" if pred == 0 else str(int(err[r][c]) * 1.0 / pred))
    out["_error_markov_model"] = s
    # match Markov model (B:424-476).  The previous-match lengths are cut into <= 15 consecutive bins of about total / 15 pairs each:
    # a bin takes rows while it is below the target and stops in front of a row that would carry it further from the target than it is
    # (never in front of its first row); rows left over behind the 15th bin are added to its counts (its label keeps the old end)
    n = max(150, t["max_match"] + 1)
    pairs = np.zeros((n, n), dtype=np.int64)
    k = min(n, m2.shape[0])
    pairs[:k, :k] = m2[:k, :k]
    per_row = [int(x) for x in pairs.sum(axis=1)]
    target = sum(per_row) / 15
    edges, sizes = [], []                 # (first row, one past the last row) and the pairs of every bin
    row = 0
    while len(edges) < 15 and row < n:
        start, got = row, 0
        while got < target and row < n:
            if got != 0 and abs(got + per_row[row] - target) > abs(got - target):
                break
            got += per_row[row]
            row += 1
        edges.append((start, row))
        sizes.append(got)
    cols = [pairs[lo:hi].sum(axis=0) if hi > lo else np.zeros(n, dtype=np.int64) for lo, hi in edges]
    if row < n:
        cols[-1] = cols[-1] + pairs[row:n].sum(axis=0)
        sizes[-1] += sum(per_row[row:n])
    running = [0] * len(edges)
    lines = ["bins\t" + "\t".join("%s-%s" % e for e in edges) + '\n']
    for i in range(n):
        cells = [str(i) + "-" + str(i + 1)]
        for j in range(len(edges)):
            if sizes[j] == 0:
                cells.append("0")
            else:
                running[j] += int(cols[j][i]) * 1.0 / sizes[j]
                cells.append(str(running[j]))
        lines.append("\t".join(cells) + '\n')
    out["_match_markov_model"] = "".join(lines)
    # first match profile (B:478-486)
    nf = _dict_len(dic[1], 150)
    total_first = int(dic[1][:nf].sum())
    lines = ["bin\t0-50000\n"]
    cp = 0
    for i in range(nf):
        cp += int(dic[1][i]) * 1.0 / total_first
        lines.append(str(i) + "-" + str(i + 1) + "\t" + str(cp) + '\n')
    out["_first_match.hist"] = "".join(lines)
    return out


def hist(prefix: str, alignments, eng, alnm_ftype: str = "bam") -> dict:
    """writes <prefix>_match.hist, _mis.hist, _ins.hist, _del.hist, _error_rate.tsv, _error_markov_model, _match_markov_model and
    _first_match.hist like hist(prefix, alnm_ftype) (B:148-486; `prefix` may end in "_genome", B:150-151); returns the counts.
    alnm_ftype "bam" (or "sam"): alignments = cs strings (cs_from_sam); "maf": (reference line, query line) pairs (maf_pairs)"""
    if "_genome" in prefix:
        prefix = prefix[:-7]
    t = count_maf(eng, alignments) if alnm_ftype == "maf" else count(eng, alignments)
    for name, text in format_tables(t).items():
        write_text(prefix + name, text)
    return t
