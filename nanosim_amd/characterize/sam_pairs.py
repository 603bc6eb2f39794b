"""SAM input of that model is the fourth piece.  The reference's default aligner writes SAM, and the reference turns it into MAF line pairs
first: ``samtools view | sam2pairwise``, then src/pairwise2maf.py (P:38-82; src/read_analysis.py:200-204).  Here the two aligned lines of
every record are built on the GPU from its CIGAR, MD:Z and SEQ (``ns_sam_pairs_build``, csrc/ns_sam_pairs.h) and stay packed — and, for
the model, stay on the device (``ns_hp_histograms_sam``):

    recs = characterize.sam_records("training_primary.sam")                 # FLAG 0 / 16, as pairwise2maf keeps them
    characterize.homopolymer_lengths_from_sam("training", recs, eng, min_hp_len=5, maf_file=True)   # + training_processed.maf
    packed = characterize.pairs_from_sam(eng, recs)                         # a PackedPairs: count_maf / count_homopolymers take it as it is

Deviations: a record pairwise2maf would stop on (`H` in the CIGAR: its int() fails; a trailing clip behind an op other than M) or whose
CIGAR, MD and SEQ contradict each other raises ValueError; `N` / `P` ops are not handled."""
import ctypes as C

import numpy as np

from ._abi import PackedPairs, _pack, check_bad, ptr, write_text
from .homopolymers import _hp_count, write_hp_files
from .sam_table import SamTable
from .sam_text import sam_lines, sam_tag


class NsSamPairs(C.Structure):
    """mirror of ns_sam_pairs (include/nanosim_amd.h)"""
    _fields_ = [("ref_lines", C.c_void_p), ("query_lines", C.c_void_p), ("cap_bytes", C.c_uint64), ("aln_off", C.c_void_p), ("aln", C.c_void_p),
                ("n_bytes", C.c_uint64), ("n_bad", C.c_uint64), ("first_bad", C.c_uint64), ("ms_kernel", C.c_double)]


SAM_ALN_DTYPE = np.dtype([("head", "<u4"), ("tail", "<u4"), ("ref_len", "<u4"), ("query_len", "<u4")])      # ns_sam_aln


def sam_records(path: str):
    """[(qname, flag, rname, pos, cigar, md, seq)] of a SAM text file: the records pairwise2maf keeps — FLAG exactly 0 or 16 (P:46-51) —
    in file order.  A kept record without MD:Z, or with `H` in its CIGAR (the reference's int() stops there, P:59-67), raises ValueError."""
    if isinstance(path, SamTable):
        return path.sam_records()
    out = []
    for fld in sam_lines(path, 11):
        if fld[1] not in ("0", "16"):
            continue
        md = sam_tag(fld, "MD:Z:")
        if md is None:
            raise ValueError("alignment %s has no MD tag" % fld[0])
        if "H" in fld[5]:
            raise ValueError("alignment %s has a hard clip in its CIGAR (src/pairwise2maf.py:59-67 stops on it)" % fld[0])
        out.append((fld[0], int(fld[1]), fld[2], int(fld[3]), fld[5], md, fld[9]))
    return out


def _pack_sam(sam_recs):
    """the six string arguments of the SAM calls and what keeps them alive"""
    cg, cg_off = _pack([r[4] for r in sam_recs])
    md, md_off = _pack([r[5] for r in sam_recs])
    sq, sq_off = _pack([r[6] for r in sam_recs])
    return (cg.ctypes.data, cg_off.ctypes.data, md.ctypes.data, md_off.ctypes.data, sq.ctypes.data, sq_off.ctypes.data), (cg, cg_off, md, md_off, sq, sq_off)


def _sam_out(sam_recs, keep, lines: bool):
    """an NsSamPairs with its buffers: the lines sized by what no record can exceed (a column per SEQ byte and per MD byte), so that
    one call is enough"""
    n = len(sam_recs)
    cap = int(keep[3][-1]) + int(keep[5][-1]) if lines else 0
    p = NsSamPairs()
    bufs = dict(off=np.zeros(n + 1, dtype=np.uint64), aln=np.zeros(n, dtype=SAM_ALN_DTYPE),
                ref=np.zeros(cap + 1 if lines else 0, dtype=np.uint8), qry=np.zeros(cap + 1 if lines else 0, dtype=np.uint8))
    p.aln_off, p.aln = bufs["off"].ctypes.data, ptr(bufs["aln"])
    if lines:
        p.ref_lines, p.query_lines, p.cap_bytes = bufs["ref"].ctypes.data, bufs["qry"].ctypes.data, cap
    return p, bufs


def _sam_packed(sam_recs, p, bufs) -> PackedPairs:
    check_bad(p.n_bad, p.first_bad, "SAM record(s) whose CIGAR, MD and SEQ do not describe an alignment",
              lambda i: "record %d (%s): CIGAR %.60s, MD %.60s, %d bases" % (i, sam_recs[i][0], sam_recs[i][4], sam_recs[i][5], len(sam_recs[i][6])))
    n = int(p.n_bytes)
    if not len(bufs["ref"]):
        return PackedPairs(None, None, bufs["off"], bufs["aln"], sam_recs)
    bufs["ref"][n] = bufs["qry"][n] = 0
    return PackedPairs(bufs["ref"][:n + 1], bufs["qry"][:n + 1], bufs["off"], bufs["aln"], sam_recs)


def pairs_from_sam(eng, sam_recs) -> PackedPairs:
    """the aligned line pairs of these sam_records, built on the GPU (ns_sam_pairs_build); bad records raise ValueError naming the first"""
    args, keep = _pack_sam(sam_recs)
    p, bufs = _sam_out(sam_recs, keep, True)
    eng._check(eng.L.ns_sam_pairs_build(eng.ctx, *args, len(sam_recs), C.byref(p)))
    out = _sam_packed(sam_recs, p, bufs)
    out.ms_kernel = float(p.ms_kernel)
    return out


def format_maf(sam_recs, packed) -> str:
    """the text pairwise2maf writes for these records (P:80-82): two `s` lines per record"""
    out = []
    for i, (r, a) in enumerate(zip(sam_recs, packed.aln)):
        lo, hi = int(packed.off[i]), int(packed.off[i + 1])
        qlen, head, tail = int(a["query_len"]), int(a["head"]), int(a["tail"])
        out.append("s " + r[2] + " " + str(r[3] - 1) + " " + str(int(a["ref_len"])) + " + * " + packed.ref[lo:hi].tobytes().decode() + "\n")
        out.append("s " + r[0] + " " + str(head) + " " + str(qlen) + " " + ("+" if r[1] == 0 else "-") + " " + str(qlen + head + tail) + " " +
                   packed.qry[lo:hi].tobytes().decode() + "\n")
    return "".join(out)


def write_maf(path: str, sam_recs, packed) -> None:
    write_text(path, format_maf(sam_recs, packed))


def count_homopolymers_sam(eng, sam_recs, min_hp_len: int = 5, records: bool = False, lines: bool = False, cap_ref: int = 64, cap_read: int = 64,
                           cap_records=None) -> dict:
    """count_homopolymers for sam_records in one call (ns_hp_histograms_sam): the lines are built and counted on the device and come
    back only with `lines` ("pairs": a PackedPairs; without `lines` its ref / qry are None)"""
    args, keep = _pack_sam(sam_recs)
    state = {}

    def call(h):
        p, bufs = _sam_out(sam_recs, keep, lines)
        eng._check(eng.L.ns_hp_histograms_sam(eng.ctx, *args, len(sam_recs), int(min_hp_len), C.byref(p), C.byref(h)))
        state["pairs"] = _sam_packed(sam_recs, p, bufs)
        state["ms_pairs"] = float(p.ms_kernel)
    out = _hp_count(call, int(keep[5][-1]), min_hp_len, records, cap_ref, cap_read, cap_records)
    out["pairs"], out["ms_kernel_pairs"] = state["pairs"], state["ms_pairs"]
    return out


def homopolymer_lengths_from_sam(prefix: str, sam_recs, eng, min_hp_len: int = 5, lengths_file: bool = True, maf_file: bool = False) -> dict:
    """homopolymer_lengths for sam_records: the same two files, through ns_hp_histograms_sam; with maf_file also <prefix>_processed.maf
    (what read_analysis.py:200-204 leaves behind); returns the counts"""
    t = count_homopolymers_sam(eng, sam_recs, min_hp_len, records=lengths_file, lines=maf_file)
    if maf_file:
        write_maf(prefix + "_processed.maf", sam_recs, t["pairs"])
    write_hp_files(prefix, t, t["pairs"], lengths_file)
    return t
