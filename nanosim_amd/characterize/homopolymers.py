"""The homopolymer-length model (src/model_homopolymer_lengths.py, H:9-243) is the third piece: `-hp` reads
``<prefix>_hp_lengths_model_parameters.tsv``.  Per homopolymer of the reference line of every MAF alignment its length there and the
length the read shows (the reference's four regular expressions, restated as one pass in csrc/ns_hp_hist.h and counted on the GPU,
``ns_hp_histograms``), then the two fits per class (AT, CG) over the counts:

    recs = characterize.maf_records("training_besthit.maf")
    characterize.homopolymer_lengths("training", recs, eng, min_hp_len=5)   # -> training_hp_lengths_model_parameters.tsv, _hp_lengths.tsv

Deviation: the reference fits the mean read length with ``piecewise_regression.Fit(xx, yy, n_breakpoints=1)`` — Muggeo's iteration from
random starts with 100 bootstrap restarts, which the reference does not seed, so its text is not reproducible even by itself.  What is
written here is the least-squares optimum that iteration approximates, computed exactly (Hudson 1966).  The library is not installed
where this was developed, so nobody has compared the two fits.  ``min_hp_len < 1`` and input without any homopolymer raise ValueError
(the reference's `A{0,}` matches empty strings; it divides by zero)."""
import ctypes as C

import numpy as np

from ._abi import PackedPairs, _pack_pairs, write_text
from .errors import s_line_pairs


class NsHpHist(C.Structure):
    """mirror of ns_hp_hist (include/nanosim_amd.h)"""
    _fields_ = [("cap_ref", C.c_uint32), ("cap_read", C.c_uint32), ("table", C.c_void_p), ("records", C.c_void_p), ("cap_records", C.c_uint64),
                ("n_hp", C.c_uint64), ("columns", C.c_uint64 * 4), ("max_ref", C.c_uint64), ("max_read", C.c_uint64), ("n_overflow", C.c_uint64),
                ("ms_kernel", C.c_double)]


HP_CLASSES = ("AT", "CG")                                   # the rows of the reference's file (H:48, 116)
HP_COLUMNS = ("ins", "del", "mis", "match")                 # err_dict (H:15)
HP_RECORD_DTYPE = np.dtype([("aln", "<u4"), ("start", "<u4"), ("ref_len", "<u4"), ("read_base", "<u4")])      # ns_hp_record
HP_PW_KEYS = ("const", "beta1", "breakpoint1", "alpha1", "alpha2")      # get_results()["estimates"] of piecewise_regression, in its order
HP_NOT_CONVERGED = ("Piecewise regression for homopolymer characterization did not converge. Consider using more reads, a subsample, "
                    "turning off homopolymer compression, or using a pre-trained model.")                    # H:151-153


def maf_records(path: str):
    """[(reference name, reference start, reference line, query line)] of `<prefix>_besthit.maf`: maf_pairs plus fields 2 and 3 of the
    reference `s` line, which analyze_homopolymers puts into `<prefix>_hp_lengths.tsv` (H:55-57, 113)"""
    return [(r[1], int(r[2]), r[6], q[6][:len(r[6])]) for r, q in s_line_pairs(path)]


def _hp_count(call, nbytes_hint: int, min_hp_len: int, records: bool, cap_ref: int, cap_read: int, cap_records) -> dict:
    """count_homopolymers and count_homopolymers_sam: `call(h)` makes the library's call on an NsHpHist (false: it counted nothing);
    repeated with what it asks for while it reports an overflow"""
    if min_hp_len < 1:
        raise ValueError("min_hp_len must be at least 1 (the reference's `A{0,}` matches empty strings)")
    if cap_records is None:
        cap_records = nbytes_hint // (4 * min_hp_len) + 16
    while True:
        h = NsHpHist()
        table = np.zeros((2, cap_ref, cap_read), dtype=np.uint64)
        rec = np.zeros(max(int(cap_records), 1) if records else 0, dtype=HP_RECORD_DTYPE)
        h.cap_ref, h.cap_read, h.table = cap_ref, cap_read, table.ctypes.data
        if records:
            h.records, h.cap_records = rec.ctypes.data, len(rec)
        call(h)
        again = False
        if h.n_overflow:
            cap_ref = max(cap_ref, 1 << int(h.max_ref).bit_length())           # the table has to hold index max_ref
            cap_read = max(cap_read, 1 << int(h.max_read).bit_length())
            again = True
        if records and h.n_hp > len(rec):
            cap_records = int(h.n_hp)
            again = True
        if not again:
            break
    out = dict(table=table[:, :int(h.max_ref) + 1, :int(h.max_read) + 1].copy(), columns=np.ctypeslib.as_array(h.columns).copy(),
               n_hp=int(h.n_hp), ms_kernel=float(h.ms_kernel))
    if records:
        r = rec[:int(h.n_hp)]
        out["records"] = np.stack([r["aln"], r["start"], r["ref_len"], r["read_base"] >> 2,
                                   np.frombuffer(b"ACGT", dtype=np.uint8)[r["read_base"] & 3]], axis=1).astype(np.int64).reshape(-1, 5)
    return out


def count_homopolymers(eng, pairs, min_hp_len: int = 5, records: bool = False, cap_ref: int = 64, cap_read: int = 64, cap_records=None) -> dict:
    """what analyze_homopolymers (H:64-119) and calc_homopolymer_mis_rate (H:9-33) collect for these alignments, from the GPU
    (ns_hp_histograms).  pairs: (reference line, query line) tuples, maf_records' tuples (their last two entries are used), or a
    PackedPairs (used as it is: no join, no re-pack).
    {"table": uint64 (2, R, Q) — class AT / CG, reference length, read length; R, Q = the largest lengths met + 1 —, "columns": uint64 (4,)
    in the order HP_COLUMNS, "n_hp", "ms_kernel"} and, with records, "records": int64 (n_hp, 5) — alignment index, first letter in the
    dash-less reference line, reference length, read length, base (its character code) — in the order of the alignments.
    The caps are first sizes only: a call that reports an overflow is repeated with what it asks for."""
    if min_hp_len < 1:
        raise ValueError("min_hp_len must be at least 1 (the reference's `A{0,}` matches empty strings)")
    ref, qry, off = _pack_pairs(pairs) if isinstance(pairs, PackedPairs) else _pack_pairs([p[-2] for p in pairs], [p[-1] for p in pairs])
    return _hp_count(lambda h: eng._check(eng.L.ns_hp_histograms(eng.ctx, ref.ctypes.data, qry.ctypes.data, int(off[-1]), off.ctypes.data, len(off) - 1,
                                                                 int(min_hp_len), C.byref(h))),
                     int(off[-1]), min_hp_len, records, cap_ref, cap_read, cap_records)


def _piecewise_rss(x, y, const, alpha1, beta1, psi):
    r = y - (const + alpha1 * x + beta1 * np.maximum(x - psi, 0.0))
    return float(r @ r)


def fit_piecewise(x, y):
    """(const, beta1, breakpoint1, alpha1, alpha2): the least-squares continuous two-segment line through (x, y) — x distinct, ascending —
    with its breakpoint in [x[1], x[-2]], exactly (Hudson 1966): the optimum either joins the separate fits of the points left and right of
    a gap where they cross inside that gap, or has its breakpoint on a data point, where the fit is linear in the other three."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(x)
    if n < 4:
        raise ValueError(HP_NOT_CONVERGED)
    best = None

    def offer(const, alpha1, beta1, psi):
        nonlocal best
        rss = _piecewise_rss(x, y, const, alpha1, beta1, psi)
        if best is None or rss < best[0]:
            best = (rss, const, alpha1, beta1, psi)
    for i in range(1, n - 1):                                   # the breakpoint on a data point
        psi = x[i]
        sol = np.linalg.lstsq(np.stack([np.ones(n), x, np.maximum(x - psi, 0.0)], axis=1), y, rcond=None)[0]
        offer(float(sol[0]), float(sol[1]), float(sol[2]), float(psi))
    for j in range(2, n - 1):                                   # the gap between x[j - 1] and x[j]: at least two points on either side
        b1, a1 = np.polyfit(x[:j], y[:j], 1)
        b2, a2 = np.polyfit(x[j:], y[j:], 1)
        if b1 != b2:
            psi = (a1 - a2) / (b2 - b1)
            if x[j - 1] <= psi <= x[j]:
                offer(float(a1), float(b1), float(b2 - b1), float(psi))
    _, const, alpha1, beta1, psi = best
    return (const, beta1, psi, alpha1, alpha1 + beta1)


def fit_homopolymers(table, columns) -> dict:
    """{"mis_rate", "AT": {"pw": (const, beta1, breakpoint1, alpha1, alpha2), "lr": (intercept, slope)}, "CG": ...} from the counts:
    calc_homopolymer_mis_rate (H:33), fit_piecewise over the mean read length per reference length (H:142-163; see the module docstring
    for what stands in for piecewise_regression) and fit_lr over its population standard deviation (H:189-201:
    LinearRegression(fit_intercept=False) is slope = sum(x y) / sum(x x), intercept 0.0).  Both fits are unweighted over the distinct
    reference lengths present, as in the reference."""
    table = np.asarray(table)
    ins, dele, mis, match = (int(v) for v in columns)
    if not table.any() or dele + mis + match == 0:
        raise ValueError("no homopolymer in the alignments: no mismatch rate (the reference divides by zero)")
    out = {"mis_rate": mis / (dele + mis + match)}
    q = np.arange(table.shape[2], dtype=np.float64)
    for name, t in zip(HP_CLASSES, table):
        n = t.sum(axis=1)
        xs = np.nonzero(n)[0]
        if len(xs) < 4:
            raise ValueError(HP_NOT_CONVERGED)
        cnt = t[xs].astype(np.float64)
        mean = np.array([int((row.astype(np.int64) * np.arange(len(row), dtype=np.int64)).sum()) / int(tot) for row, tot in zip(t[xs], n[xs])], dtype=np.float64)
        sd = np.sqrt((cnt * (q[None, :] - mean[:, None]) ** 2).sum(axis=1) / n[xs].astype(np.float64))
        x = xs.astype(np.float64)
        out[name] = {"pw": fit_piecewise(x, mean), "lr": (0.0, float((x * sd).sum() / (x * x).sum()))}
    return out


def format_hp_model(fit: dict) -> str:
    """the text of <prefix>_hp_lengths_model_parameters.tsv as model_homopolymer_lengths writes it (H:236-243)"""
    s = "#Homopolymer mismatch rate: " + str(fit["mis_rate"]) + "\n" + "base\t" + "\t".join(HP_PW_KEYS) + "\t" + "intercept\tslope" + "\n"
    for name in HP_CLASSES:
        s += name + "\t" + "\t".join(str(float(v)) for v in fit[name]["pw"]) + "\t" + "\t".join(str(float(v)) for v in fit[name]["lr"]) + "\n"
    return s


def format_hp_lengths(maf_recs, records) -> str:
    """the text of <prefix>_hp_lengths.tsv (H:126-138): one row per distinct (position, base, reference length, read length) with its
    count, in the order np.unique(..., axis=0) gives the reference's rows of strings — lexicographic on the strings"""
    s = "Chrom:Ref pos\tType\tRef length\tRead length\tCount\n"
    if not len(records):
        return s
    if isinstance(maf_recs, PackedPairs):
        maf_recs = maf_recs.heads()
    names = sorted(set(r[0] for r in maf_recs))
    name_id = {n: i for i, n in enumerate(names)}
    aln = records[:, 0]
    key = np.stack([np.array([name_id[maf_recs[a][0]] for a in aln], dtype=np.int64),
                    np.array([maf_recs[a][1] for a in aln], dtype=np.int64) + records[:, 1], records[:, 2], records[:, 3], records[:, 4]], axis=1)
    uniq, counts = np.unique(key, axis=0, return_counts=True)
    rows = [(names[u[0]] + ":" + str(u[1] + 1) + "-" + str(u[1] + u[2] + 1), chr(u[4]), str(u[2]), str(u[3]), str(c))
            for u, c in zip(uniq.tolist(), counts.tolist())]
    rows.sort(key=lambda r: r[:4])
    return s + "".join("\t".join(r) + "\n" for r in rows)


def write_hp_files(prefix: str, t: dict, recs, lengths_file: bool) -> None:
    """<prefix>_hp_lengths.tsv (with lengths_file; recs: maf_records' tuples or a PackedPairs) and _hp_lengths_model_parameters.tsv"""
    if lengths_file:
        write_text(prefix + "_hp_lengths.tsv", format_hp_lengths(recs, t["records"]))
    write_text(prefix + "_hp_lengths_model_parameters.tsv", format_hp_model(fit_homopolymers(t["table"], t["columns"])))


def homopolymer_lengths(prefix: str, records_or_pairs, eng, min_hp_len: int = 5, lengths_file: bool = True) -> dict:
    """writes <prefix>_hp_lengths_model_parameters.tsv like model_homopolymer_lengths (H:212-243) and, with lengths_file,
    <prefix>_hp_lengths.tsv like analyze_homopolymers (H:126-138; it needs maf_records' tuples: the reference name and start);
    returns the counts"""
    if lengths_file and any(len(r) < 4 for r in records_or_pairs):
        raise ValueError("<prefix>_hp_lengths.tsv needs the reference name and start of every alignment (maf_records)")
    t = count_homopolymers(eng, records_or_pairs, min_hp_len, records=lengths_file)
    write_hp_files(prefix, t, records_or_pairs, lengths_file)
    return t
