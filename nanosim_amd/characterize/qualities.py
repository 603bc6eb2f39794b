"""The base-quality model (src/model_base_qualities.py, M:23-117) is the second piece: for every query base of every primary alignment its
class (mismatch / insertion / match from the cs string, head-tail for the soft clips, unmapped) and its quality, counted on the GPU
(``ns_qual_histograms``) into a 5 x 94 histogram, of which the log-normal fit the reference runs (``lognorm.fit(quals, floc=0)``, M:93)
is a closed form:

    aligned, unmapped = characterize.quals_from_sam("training.sam")
    characterize.base_qualities("training", aligned, unmapped, eng)     # -> training_base_qualities_model_parameters.tsv

Deviations: the fit uses every value (the reference subsamples classes above 500 000 values with np.random.choice, M:86-89: the same
estimator on fewer data); a class without values or with a quality of 0, an alignment whose cs string covers fewer bases than its
aligned part, and an aligned record without QUAL raise ValueError where the reference stops inside scipy / with an IndexError."""
import ctypes as C
import re

import numpy as np

from ._abi import _pack, write_text
from .sam_table import SamTable
from .sam_text import cs_of, sam_lines


class NsQualAln(C.Structure):
    """mirror of ns_qual_aln (include/nanosim_amd.h)"""
    _fields_ = [("head", C.c_uint32), ("tail", C.c_uint32), ("unmapped", C.c_uint32), ("reserved", C.c_uint32)]


class NsQualHist(C.Structure):
    """mirror of ns_qual_hist (include/nanosim_amd.h)"""
    _fields_ = [("hist", (C.c_uint64 * 128) * 5), ("n_short", C.c_uint64), ("n_bad_qual", C.c_uint64), ("ms_kernel", C.c_double)]


QUAL_TYPES = ("mis", "ins", "match", "ht", "unmapped")      # the rows of the reference's file, in its order (M:62, 85)
QUAL_VALUES = 94                                            # Phred 0 .. 93 ('!' .. '~')
QUAL_ALN_DTYPE = np.dtype([("head", "<u4"), ("tail", "<u4"), ("unmapped", "<u4"), ("reserved", "<u4")])

_CLIP_HEAD = re.compile(r'^(?:\d+H)?(\d+)S')
_CLIP_TAIL = re.compile(r'(\d+)S(?:\d+H)?$')


def quals_from_sam(path: str, primary_only: bool = True):
    """(aligned, unmapped) of a SAM text file.  aligned: [(cs, QUAL, head, tail)] of the records without flag 0x4 and 0x100 (and, with
    primary_only, without 0x800: what get_primary_sam keeps) — the cs:Z tag, else from CIGAR + MD:Z; head / tail: the leading / trailing
    soft clip (query_alignment_start, len - query_alignment_end; hard clips are not in QUAL).  unmapped: the QUAL strings of the flag 0x4
    records (src/get_primary_sam.py:172-175; a missing QUAL is skipped there, and is a ValueError on an aligned record)."""
    if isinstance(path, SamTable):
        return path.quals_from_sam(primary_only)
    aligned, unmapped = [], []
    drop = 0x100 | 0x800 if primary_only else 0x100
    for fld in sam_lines(path, 11):
        flag = int(fld[1])
        if flag & 0x4:
            if fld[10] != "*":
                unmapped.append(fld[10])
        elif not flag & drop:
            if fld[10] == "*":
                raise ValueError("alignment %s has no QUAL" % fld[0])
            cs = cs_of(fld)
            h, t = _CLIP_HEAD.match(fld[5]), _CLIP_TAIL.search(fld[5])
            aligned.append((cs, fld[10], int(h.group(1)) if h else 0, int(t.group(1)) if t else 0))
    return aligned, unmapped


def _qual_call(eng, entries) -> NsQualHist:
    """ns_qual_histograms on [(cs, QUAL, head, tail, unmapped)], in this order"""
    cs_data, cs_off = _pack([e[0] for e in entries])
    q_data, q_off = _pack([e[1] for e in entries])
    aln = np.array([(e[2], e[3], 1 if e[4] else 0, 0) for e in entries], dtype=QUAL_ALN_DTYPE)
    h = NsQualHist()
    eng._check(eng.L.ns_qual_histograms(eng.ctx, cs_data.ctypes.data, int(cs_off[-1]), cs_off.ctypes.data, q_data.ctypes.data, int(q_off[-1]),
                                        q_off.ctypes.data, aln.ctypes.data, len(entries), C.byref(h)))
    return h


def count_qualities(eng, aligned, unmapped=()) -> dict:
    """{"hist": uint64 (5, 94) — rows QUAL_TYPES, columns Phred 0 .. 93 —, "ms_kernel"}: what analyze_aligned_base_qualities (M:55-79)
    collects for `aligned` = [(cs, QUAL, head, tail)] plus the qualities of the `unmapped` QUAL strings, as counts, from the GPU"""
    h = _qual_call(eng, [(c, q, hd, tl, 0) for c, q, hd, tl in aligned] + [("", q, 0, 0, 1) for q in unmapped])
    if h.n_short:
        raise ValueError("%d alignment(s) whose cs string covers fewer query bases than the aligned part of QUAL (the reference stops with "
                         "an IndexError, src/model_base_qualities.py:74)" % h.n_short)
    if h.n_bad_qual:
        raise ValueError("%d QUAL byte(s) outside '!' .. '~'" % h.n_bad_qual)
    return dict(hist=np.ctypeslib.as_array(h.hist)[:, :QUAL_VALUES].copy(), ms_kernel=float(h.ms_kernel))


def fit_qualities(hist) -> dict:
    """{type: (sd, loc, mu)} of fit_lognorm (M:82-96) from the counts.  With floc = 0 scipy's lognorm.fit is the closed form
    mu = mean(ln q), sd = sqrt(mean((ln q - mu)^2)), loc = 0, evaluated here over the histogram (every value, no subsample).
    (A class whose values are all equal gives sd = 0; scipy falls back to a numeric fit there.)"""
    hist = np.asarray(hist)
    lnq = np.log(np.arange(1, hist.shape[1], dtype=np.float64))
    out = {}
    for name, row in zip(QUAL_TYPES, hist):
        n = int(row.sum())
        if n == 0:
            raise ValueError("no base qualities of type %r: a log-normal cannot be fitted" % name)
        if row[0]:
            raise ValueError("base qualities of type %r hold the value 0 (ln 0): a log-normal with loc = 0 cannot be fitted" % name)
        w = row[1:].astype(np.float64)
        mu = float((w * lnq).sum() / n)
        sd = float(np.sqrt((w * (lnq - mu) ** 2).sum() / n))
        out[name] = (sd, 0, mu)
    return out


def format_base_qualities(params: dict) -> str:
    """the text of <prefix>_base_qualities_model_parameters.tsv as fit_lognorm writes it (M:83-96)"""
    return "type\tsd\tloc\tmu\n" + "".join(name + "\t" + str(params[name][0]) + "\t" + str(params[name][1]) + "\t" + str(params[name][2]) + "\n"
                                           for name in QUAL_TYPES)


def base_qualities(prefix: str, aligned, unmapped, eng) -> dict:
    """writes <prefix>_base_qualities_model_parameters.tsv like model_base_qualities (M:99-117); returns the counts"""
    t = count_qualities(eng, aligned, unmapped)
    write_text(prefix + "_base_qualities_model_parameters.tsv", format_base_qualities(fit_qualities(t["hist"])))
    return t
