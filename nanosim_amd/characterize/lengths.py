"""The read-length models (src/head_align_tail_dist.py, A:58-281; the non-chimeric ``primary_and_unaligned`` of src/get_primary_sam.py,
G:145-217; src/read_analysis.py R:833-851) are the sixth piece, and the last one between a SAM file and a genome-mode model that
``model.load_model`` opens: ``_aligned_region.pkl``, ``_aligned_reads.pkl``, ``_ht_length.pkl``, ``_ht_ratio.pkl``,
``_unaligned_length.pkl``, ``_aligned_region_2d.pkl`` (transcriptome mode), ``_strandness_rate`` and ``_reads_alignment_rate``.  The
reference walks every primary alignment through pysam; here the CIGAR walk, the segment rule and the reduction per read run on the GPU
(``ns_read_lengths``, csrc/ns_read_len.h), and this module transforms the lengths and writes the files:

    refs, recs, unaligned_len, strandness = characterize.primary_and_unaligned("training.sam")
    characterize.read_lengths("training", refs, recs, eng, unaligned_len, strandness)

The KDEs always go to ``<prefix>_kde.npz`` (what ``model.load_model`` reads first) and, when scikit-learn and joblib are installed, also
to the reference's pickles.  Deviations: a record whose CIGAR is not one, or that covers no reference base, raises ValueError (the
reference silently drops the read that such a record ends, A:172); the seven debugging ``.txt`` files of A:81-87 are not written."""
import ctypes as C
import os

import numpy as np

from ._abi import _pack, arr, check_bad, ptr, write_text
from .errors import s_line_pairs
from .sam_table import SamTable
from .sam_text import no_sq_line, sam_lines


class NsLenResult(C.Structure):
    """mirror of ns_len_result (include/nanosim_amd.h)"""
    _fields_ = [("aln", C.c_void_p), ("reads", C.c_void_p), ("segments", C.c_void_p), ("n_segments", C.c_uint64), ("n_bad", C.c_uint64),
                ("first_bad", C.c_uint64), ("ms_kernel", C.c_double)]


LEN_ALN_DTYPE = np.dtype([("head", "<u4"), ("tail", "<u4"), ("read_len", "<u4"), ("ref_len", "<u4"), ("query_aln_len", "<u4"), ("edge", "<u4")])   # ns_len_aln
LEN_READ_DTYPE = np.dtype([("read_len", "<u4"), ("head", "<u4"), ("tail", "<u4"), ("n_segments", "<u4")])                                      # ns_len_read
LEN_GENOME, LEN_TRANSCRIPTOME = 0, 1                        # NS_LEN_*
LEN_NONE = 0xffffffff
LEN_MODES = {"genome": LEN_GENOME, "transcriptome": LEN_TRANSCRIPTOME}
KDE_NAMES = ("aligned_region", "aligned_reads", "ht_length", "ht_ratio", "unaligned_length", "aligned_region_2d")


def length_records(path: str):
    """(refs, records) of a SAM text file: refs = [(SN, LN)] of its @SQ lines, records = [(qname, flag, rname, pos, cigar)] of every
    record whose CIGAR is not `*`, in file order — the reference's `<prefix>_primary` file (A:127-134) as SAM text.  A record on a
    reference without an @SQ line raises ValueError (the reference stops with a KeyError, A:138, 156)."""
    if isinstance(path, SamTable):
        return path.length_records()
    refs, records = [], []
    for fld in sam_lines(path, 6, refs):
        if fld[5] != "*":
            records.append((fld[0], int(fld[1]), fld[2], int(fld[3]), fld[5]))
    known = set(n for n, _ in refs)
    for r in records:
        if r[2] not in known:
            raise no_sq_line(r[0], r[2])
    return refs, records


def primary_and_unaligned(path: str):
    """(refs, records, unaligned_len, strandness) of a whole SAM text file, as primary_and_unaligned does without a metagenome list
    (G:163-187): refs and records as length_records gives them, of the primary records (FLAG without 0x4, 0x100 and 0x800);
    unaligned_len: int64 array of len(SEQ), 0 for `*`, of the 0x4 records (query_length); strandness = records whose FLAG is 0 over the
    primary records.  No primary record raises ValueError (the reference divides by zero)."""
    if isinstance(path, SamTable):
        return path.primary_and_unaligned()
    refs, records, unaligned, pos_strand = [], [], [], 0
    for fld in sam_lines(path, 11, refs):
        flag = int(fld[1])
        if not flag & (0x4 | 0x100 | 0x800):
            records.append((fld[0], flag, fld[2], int(fld[3]), fld[5]))
            if flag == 0:
                pos_strand += 1
        elif flag & 0x4:
            unaligned.append(0 if fld[9] == "*" else len(fld[9]))
    if not records:
        raise ValueError("%s holds no primary alignment" % path)
    return refs, records, np.array(unaligned, dtype=np.int64), float(pos_strand) / len(records)


def _len_call(eng, refs, records, read_off, mode: int, extra=None):
    """ns_read_lengths: (figures per record, per read, the segments, ms_kernel); bad records raise ValueError naming the first"""
    n, n_reads = len(records), len(read_off) - 1
    ref_index = {name: i for i, (name, _) in reversed(list(enumerate(refs)))}            # (of equal names the first)
    ref_id = np.zeros(n, dtype=np.uint32)
    ref_start = np.zeros(n, dtype=np.uint64)
    for i, r in enumerate(records):
        if r[2] not in ref_index:
            raise no_sq_line(r[0], r[2])
        if r[3] < 1:
            raise ValueError("alignment %s has POS %d" % (r[0], r[3]))
        ref_id[i], ref_start[i] = ref_index[r[2]], r[3] - 1
    cg, cg_off = _pack([r[4] for r in records])
    reverse = np.array([1 if r[1] & 0x10 else 0 for r in records], dtype=np.uint8)
    ref_total = np.array([ln for _, ln in refs], dtype=np.uint64)
    read_off = arr(read_off, np.uint64)
    aln = np.zeros(n, dtype=LEN_ALN_DTYPE)
    reads = np.zeros(n_reads, dtype=LEN_READ_DTYPE)
    segments = np.zeros(n, dtype=np.uint64)
    out = NsLenResult()
    out.aln, out.reads, out.segments = ptr(aln), ptr(reads), ptr(segments)
    eh, et = (None, None) if extra is None else (arr(extra[0], np.uint32), arr(extra[1], np.uint32))        # (one per read: NULL without reads)
    eng._check(eng.L.ns_read_lengths(eng.ctx, cg.ctypes.data, cg_off.ctypes.data, reverse.ctypes.data, ref_id.ctypes.data, ref_start.ctypes.data,
                                     ref_total.ctypes.data, len(refs), read_off.ctypes.data, n_reads, n, mode, ptr(eh), ptr(et), C.byref(out)))
    check_bad(out.n_bad, out.first_bad, "SAM record(s) whose CIGAR is not one or covers no reference base",
              lambda i: "record %d (%s): CIGAR %.60s" % (i, records[i][0], records[i][4]))
    return aln, reads, segments[:int(out.n_segments)], float(out.ms_kernel)


def count_read_lengths(eng, refs, records, mode: str = "genome", genome_records=None) -> dict:
    """what head_align_tail's loop (A:134-229) collects for the records of length_records, from the GPU (ns_read_lengths).  Reads are
    runs of equal consecutive qname.  genome_records (transcriptome mode): the records of `<prefix>_genome_primary` — their heads and
    tails, from a call of their own and reduced by name, bound the heads and tails of the reads they share (dict_genome_alnm_info,
    A:64-73, 145-153, 203-207).
    int64 arrays: "aligned_ref_length" (the aligned segments), "total_length", "ht_length", "head", "tail" (per read), in transcriptome
    mode "total_ref_length" (LN per record); float64 "head_vs_ht_ratio" = head / ht with the reference's two conditions — every read but
    the last contributes when its head != 0 (A:180), the last when its ht != 0 (A:219); "aln": the figures per record (LEN_ALN_DTYPE),
    "n_segments" per read, "ms_kernel"."""
    if mode not in LEN_MODES:
        raise ValueError("mode must be 'genome' or 'transcriptome'")
    n = len(records)
    starts = [i for i in range(n) if i == 0 or records[i][0] != records[i - 1][0]]
    read_off = np.array(starts + [n], dtype=np.uint64)
    extra, ms = None, 0.0
    if genome_records is not None:
        g_aln, _, _, ms = _len_call(eng, [("", 0)], [(r[0], r[1], "", 1, r[4]) for r in genome_records],
                                    np.arange(len(genome_records) + 1, dtype=np.uint64), LEN_TRANSCRIPTOME)
        info = {}
        for r, h, t in zip(genome_records, g_aln["head"].tolist(), g_aln["tail"].tolist()):
            old = info.get(r[0])
            info[r[0]] = (h, t) if old is None else (min(h, old[0]), min(t, old[1]))
        extra = (np.array([info.get(records[i][0], (LEN_NONE, LEN_NONE))[0] for i in starts], dtype=np.uint32),
                 np.array([info.get(records[i][0], (LEN_NONE, LEN_NONE))[1] for i in starts], dtype=np.uint32))
    aln, reads, segments, ms2 = _len_call(eng, refs, records, read_off, LEN_MODES[mode], extra)
    head, tail = reads["head"].astype(np.int64), reads["tail"].astype(np.int64)
    ht = head + tail
    take = head != 0
    if len(take):
        take[-1] = ht[-1] != 0
    out = dict(aligned_ref_length=segments.astype(np.int64), total_length=reads["read_len"].astype(np.int64), ht_length=ht, head=head, tail=tail,
               head_vs_ht_ratio=head[take].astype(np.float64) / ht[take].astype(np.float64), aln=aln, n_segments=reads["n_segments"].astype(np.int64),
               ms_kernel=ms + ms2)
    if mode == "transcriptome":
        ln = dict((name, l) for name, l in reversed(refs))
        out["total_ref_length"] = np.array([ln[r[2]] for r in records], dtype=np.int64)
    return out


def length_figures_maf(path: str, mode: str = "genome") -> dict:
    """count_read_lengths' dict for `<prefix>_besthit.maf` (A:91-110): per pair of `s` lines the aligned reference length, the read's
    length, head and ht = length - aligned part, the ratio when ht != 0, and the reference's size in transcriptome mode.  Host only:
    the numbers stand in the lines."""
    if mode not in LEN_MODES:
        raise ValueError("mode must be 'genome' or 'transcriptome'")
    rows = [(int(r[3]), int(r[5]), int(q[2]), int(q[5]), int(q[5]) - int(q[3])) for r, q in s_line_pairs(path, sequences=False)]
    return maf_figures(*np.array(rows, dtype=np.int64).reshape(-1, 5).T, mode)


def maf_figures(aligned_ref, ref_total, head, total, ht, mode: str) -> dict:
    """count_read_lengths' dict from the five figures of every pair of `s` lines (A:91-110)"""
    if mode not in LEN_MODES:
        raise ValueError("mode must be 'genome' or 'transcriptome'")
    head, ht = head.astype(np.int64), ht.astype(np.int64)
    take = ht != 0
    out = dict(aligned_ref_length=aligned_ref.astype(np.int64), total_length=total.astype(np.int64), ht_length=ht, head=head, tail=ht - head,
               head_vs_ht_ratio=head[take].astype(np.float64) / ht[take].astype(np.float64), ms_kernel=0.0)
    if mode == "transcriptome":
        out["total_ref_length"] = ref_total.astype(np.int64)
    return out


def kde_models(figures: dict, unaligned_len=None) -> dict:
    """{name: (data float64, bandwidth)} — what the reference hands to KernelDensity(bandwidth).fit (A:243-278, R:845-846):
    aligned_region and aligned_reads the raw lengths, 10; ht_length log10(ht + 1), 0.01; ht_ratio, 0.01; unaligned_length, 10, only with
    unaligned reads; aligned_region_2d, in transcriptome mode, the rows (total_ref, aligned_ref) with Silverman's bandwidth (A:13-22)"""
    m = {"aligned_region": (np.asarray(figures["aligned_ref_length"]).astype(np.float64), 10),
         "aligned_reads": (np.asarray(figures["total_length"]).astype(np.float64), 10),
         "ht_length": (np.log10(np.asarray(figures["ht_length"]) + 1).astype(np.float64), 0.01),
         "ht_ratio": (np.asarray(figures["head_vs_ht_ratio"], dtype=np.float64), 0.01)}
    if unaligned_len is not None and len(unaligned_len):
        m["unaligned_length"] = (np.asarray(unaligned_len).astype(np.float64), 10)
    if "total_ref_length" in figures:
        xy = np.vstack([np.asarray(figures["total_ref_length"]), np.asarray(figures["aligned_ref_length"])])
        d, n = xy.shape
        m["aligned_region_2d"] = (np.ascontiguousarray(xy.T, dtype=np.float64), (n * (d + 2) / 4.) ** (-1. / (d + 4)))
    return m


def write_kde(prefix: str, models: dict, pickles=None, merge: bool = False) -> None:
    """<prefix>_kde.npz with the keys <name>_data / <name>_bw that model.load_model reads; and <prefix>_<name>.pkl like the reference
    (KernelDensity(bandwidth).fit, joblib.dump) — pickles=None: when scikit-learn and joblib import, True: they have to, False: never.
    merge: the keys an existing <prefix>_kde.npz holds for other names are kept (without it the file holds `models` alone)"""
    arrays = {}
    if merge and os.path.exists(prefix + "_kde.npz"):
        with np.load(prefix + "_kde.npz") as old:
            arrays.update((k, old[k]) for k in old.files)
    for name, (data, bw) in models.items():
        arrays[name + "_data"] = np.asarray(data, dtype=np.float64)
        arrays[name + "_bw"] = np.float64(bw)
    np.savez(prefix + "_kde.npz", **arrays)
    if pickles is False:
        return
    try:
        import joblib                                       # (local: scikit-learn stays optional)
        from sklearn.neighbors import KernelDensity
    except ImportError:
        if pickles:
            raise
        return
    for name, (data, bw) in models.items():
        data = np.asarray(data, dtype=np.float64)
        joblib.dump(KernelDensity(bandwidth=bw).fit(data if data.ndim == 2 else data[:, np.newaxis]), prefix + "_" + name + ".pkl")


def format_strandness(strandness: float) -> str:
    """the text of <prefix>_strandness_rate (R:833-835): no newline"""
    return "strandness:\t" + str(round(strandness, 3))


def format_alignment_rate(num_aligned: int, num_unaligned: int) -> str:
    """the text of <prefix>_reads_alignment_rate (R:842-849)"""
    if num_unaligned != 0:
        return "Aligned / Unaligned ratio:" + "\t" + str(num_aligned * 1.0 / num_unaligned) + '\n'
    return "Aligned / Unaligned ratio:\t100%\n"


def read_lengths(prefix: str, refs, records, eng, unaligned_len, strandness: float, mode: str = "genome", genome_records=None, pickles=None,
                 merge: bool = False) -> dict:
    """writes the KDE files (write_kde), <prefix>_strandness_rate and <prefix>_reads_alignment_rate like head_align_tail (A:239-281) and
    read_analysis.py (R:833-851) — num_aligned is the number of READS of the length figures, as at R:830 — and returns the figures.
    The seven debugging files of A:81-87 (<prefix>_total.txt, _middle.txt, _head.txt, _middle_ref.txt, _ht.txt, _ratio.txt, _tail.txt)
    are not written."""
    return write_length_files(prefix, count_read_lengths(eng, refs, records, mode, genome_records), unaligned_len, strandness, pickles, merge)


def write_length_files(prefix: str, figures: dict, unaligned_len, strandness: float, pickles=None, merge: bool = False) -> dict:
    """the KDE files, <prefix>_strandness_rate and <prefix>_reads_alignment_rate from the length figures; returns the figures"""
    write_kde(prefix, kde_models(figures, unaligned_len), pickles, merge)        # (merge: the keys of other models, gap_length of chimeric(), stay)
    write_text(prefix + "_strandness_rate", format_strandness(strandness))
    write_text(prefix + "_reads_alignment_rate", format_alignment_rate(len(figures["total_length"]), 0 if unaligned_len is None else len(unaligned_len)))
    return figures


read_lengths_from_maf = write_length_files            # its name for figures that are there already (besthit's, length_figures_maf's)
