"""Training side, the histogramming step of the characterisation stage (second half): a drop-in for
``hist(prefix, "bam")`` of src/besthit_to_histogram.py (B:148-486) from the cs strings of the primary alignments on.

The reference walks every alignment in Python (parse_cs B:41-69, then the loop B:316-365) and fills dictionaries; the tables it writes
afterwards (B:366-486) are what ``simulator.py`` reads back as the error model (``read_profile``, src/simulator.py:473-501).  Here the
walk runs on the GPU through the C-ABI (``ns_cs_histograms``: one alignment per thread, include/nanosim_amd.h) and this module does
what is left: getting the cs strings out of a SAM file and formatting the reference's files from the counts, text for text.

    from nanosim_amd import characterize, engine
    eng = engine.Engine(0)
    characterize.hist("training", characterize.cs_from_sam("training_primary.sam"), eng)

    characterize.hist("training", characterize.maf_pairs("training_besthit.maf"), eng, alnm_ftype="maf")      # hist(prefix, "maf"), B:188-315

The base-quality model (src/model_base_qualities.py, M:23-117) is the second piece: for every query base of every primary alignment its
class (mismatch / insertion / match from the cs string, head-tail for the soft clips, unmapped) and its quality, counted on the GPU
(``ns_qual_histograms``) into a 5 x 94 histogram, of which the log-normal fit the reference runs (``lognorm.fit(quals, floc=0)``, M:93)
is a closed form:

    aligned, unmapped = characterize.quals_from_sam("training.sam")
    characterize.base_qualities("training", aligned, unmapped, eng)     # -> training_base_qualities_model_parameters.tsv

Deviations: the fit uses every value (the reference subsamples classes above 500 000 values with np.random.choice, M:86-89: the same
estimator on fewer data); a class without values or with a quality of 0, an alignment whose cs string covers fewer bases than its
aligned part, and an aligned record without QUAL raise ValueError where the reference stops inside scipy / with an IndexError.

The homopolymer-length model (src/model_homopolymer_lengths.py, H:9-243) is the third piece: `-hp` reads
``<prefix>_hp_lengths_model_parameters.tsv``.  Per homopolymer of the reference line of every MAF alignment its length there and the
length the read shows (the reference's four regular expressions, restated as one pass in csrc/ns_hp_hist.h and counted on the GPU,
``ns_hp_histograms``), then the two fits per class (AT, CG) over the counts:

    recs = characterize.maf_records("training_besthit.maf")
    characterize.homopolymer_lengths("training", recs, eng, min_hp_len=5)   # -> training_hp_lengths_model_parameters.tsv, _hp_lengths.tsv

Deviation: the reference fits the mean read length with ``piecewise_regression.Fit(xx, yy, n_breakpoints=1)`` — Muggeo's iteration from
random starts with 100 bootstrap restarts, which the reference does not seed, so its text is not reproducible even by itself.  What is
written here is the least-squares optimum that iteration approximates, computed exactly (Hudson 1966).  The library is not installed
where this was developed, so nobody has compared the two fits.  ``min_hp_len < 1`` and input without any homopolymer raise ValueError
(the reference's `A{0,}` matches empty strings; it divides by zero).

SAM input of that model is the fourth piece.  The reference's default aligner writes SAM, and the reference turns it into MAF line pairs
first: ``samtools view | sam2pairwise``, then src/pairwise2maf.py (P:38-82; src/read_analysis.py:200-204).  Here the two aligned lines of
every record are built on the GPU from its CIGAR, MD:Z and SEQ (``ns_sam_pairs_build``, csrc/ns_sam_pairs.h) and stay packed — and, for
the model, stay on the device (``ns_hp_histograms_sam``):

    recs = characterize.sam_records("training_primary.sam")                 # FLAG 0 / 16, as pairwise2maf keeps them
    characterize.homopolymer_lengths_from_sam("training", recs, eng, min_hp_len=5, maf_file=True)   # + training_processed.maf
    packed = characterize.pairs_from_sam(eng, recs)                         # a PackedPairs: count_maf / count_homopolymers take it as it is

Deviations: a record pairwise2maf would stop on (`H` in the CIGAR: its int() fails; a trailing clip behind an op other than M) or whose
CIGAR, MD and SEQ contradict each other raises ValueError; `N` / `P` ops are not handled.

The error-length mixtures (src/model_fitting.py, F:27-217) are the fifth piece: the simulator does not start without
``<prefix>_model_profile``, which the reference fits to the three histograms ``hist()`` wrote — 512 + 9 216 + 9 216 Nelder-Mead searches
through scipy.  Here every search is one wavefront of one kernel (``ns_mixture_fit``; objective, evaluation order and search are written
down in csrc/ns_mixfit.h), three calls in all, and this module selects and writes as the reference does:

    characterize.model_fitting("training", eng)                             # reads training_{mis,ins,del}.hist -> training_model_profile

Deviations: a search whose residual is NaN never wins (the reference sorts its results with NaN among them, which leaves their order
undefined); a histogram that leaves no bin, or a type without a valid search, raises ValueError.

The read-length models (src/head_align_tail_dist.py, A:58-281; the non-chimeric ``primary_and_unaligned`` of src/get_primary_sam.py,
G:145-217; src/read_analysis.py R:833-851) are the sixth piece, and the last one between a SAM file and a genome-mode model that
``model.load_model`` opens: ``_aligned_region.pkl``, ``_aligned_reads.pkl``, ``_ht_length.pkl``, ``_ht_ratio.pkl``,
``_unaligned_length.pkl``, ``_aligned_region_2d.pkl`` (transcriptome mode), ``_strandness_rate`` and ``_reads_alignment_rate``.  The
reference walks every primary alignment through pysam; here the CIGAR walk, the segment rule and the reduction per read run on the GPU
(``ns_read_lengths``, csrc/ns_read_len.h), and this module transforms the lengths and writes the files:

    refs, recs, unaligned_len, strandness = characterize.primary_and_unaligned("training.sam")
    characterize.read_lengths("training", refs, recs, eng, unaligned_len, strandness)

The KDEs always go to ``<prefix>_kde.npz`` (what ``model.load_model`` reads first) and, when scikit-learn and joblib are installed, also
to the reference's pickles.  Deviations: a record whose CIGAR is not one, or that covers no reference base, raises ValueError (the
reference silently drops the read that such a record ends, A:172); the seven debugging ``.txt`` files of A:81-87 are not written.

Chimeric training (``primary_and_unaligned_chimeric`` of src/get_primary_sam.py, G:220-478) is the seventh piece: what ``--chimeric``
and metagenome mode need next to the files above — ``<prefix>_chimeric_info`` and the ``gap_length`` KDE — and the choice of the records
every later training step reads (``<prefix>_primary.bam`` there, ``<prefix>_primary.sam`` here).  For every primary alignment with an
``SA:Z`` tag the reference parses the CIGAR of every entry, sorts the entries into lists of compatible pieces, keeps the best list and
records the gaps between its pieces; here the CIGAR walks and the choice run on the GPU (``ns_cigar_spans``, ``ns_chimeric_select``;
csrc/ns_chimeric.h names every corner of the reference that is kept), and this module matches the chosen pieces to SAM records and
writes the files:

    refs, recs, unaligned_len, strandness = characterize.chimeric("training", "training.sam", eng)
    characterize.read_lengths("training", refs, recs, eng, unaligned_len, strandness, merge=True)

``read_lengths`` writes ``<prefix>_kde.npz`` anew and ``chimeric`` merges into it: ``read_lengths(..., merge=True)`` keeps ``gap_length``.
Deviations: SAM text instead of BAM; a primary record without ``NM``, an SA entry without six fields, a reference name without an
``@SQ`` line, a supplementary or secondary record in front of the first primary, a chosen piece that no record matches (the reference
hands ``None`` to pysam) and a file without a primary record raise ValueError where the reference stops with another exception; the
abundances behind the shrinkage rate come from the caller unless ``quantify="meta"`` is given.

Quantification (``EM_meta`` and ``EM_trans`` of src/get_primary_sam.py, G:44-142; ``read_analysis.py quantify`` and ``-q``) is the eighth
piece: the EM over multi-mapping reads that gives the abundance of every species of a metagenome, or count and TPM of every transcript,
``<prefix>_quantification.tsv``.  The reference's loop ends where its ``diff`` stops shrinking, which is in rounding noise, so its result
depends on its summation order; the iterations run on the GPU in exactly that order (``ns_em_quantify``, csrc/ns_em.h) and give the
reference's doubles and its iteration count bit for bit.  This module builds the reference's ``quant_dic`` and ``multi_mapping_list``
with Python dicts, as the reference does, so that its key collisions are kept, computes TPM and writes the file:

    abundance, variation = characterize.quantify("training", "training.sam", eng, "meta", expected={"spA": 60.0, "spB": 40.0})
    characterize.chimeric("training", "training.sam", eng, quantify="meta")     # _chimeric_info with its own shrinkage rate

Deviations: a species of the header that ``expected`` lacks, a species or transcript of an alignment that the header lacks, a total of
2^53 / 100 bases or more and an abundance that is not finite raise ValueError; the sums are CPython's up to 3.11 (from 3.12 on ``sum``
compensates, and the reference's own result changes with it).

The intron-retention model (``intron_retention`` of src/model_intron_retention.py, M:35-219) is the ninth piece, and the last file of
a transcriptome prefix: ``<prefix>_IR_markov_model`` with ``<prefix>_IR_info``.  The reference walks the aligned blocks of every read
that has a genome and a transcriptome alignment through HTSeq's interval array; here the walk over a read's CIGAR and the introns of
its transcript, the six Markov counts and the retained introns come from the GPU (``ns_ir_train``; csrc/ns_ir_train.h names every
corner of the reference that is kept), and this module reads the annotation and the two SAM files and writes the files:

    characterize.add_introns("annotation.gff3", "training_added_intron_final.gff3")       # in place of GenomeTools
    characterize.intron_retention("training", "training_added_intron_final.gff3", "genome.sam", "transcriptome.sam", eng)

Deviations: SAM text instead of BAM; a CIGAR that is not one (`*` among them) and a start beyond 32 bits raise ValueError;
``add_introns`` is not pinned against GenomeTools' output.

LAST's MAF as alignment input (``besthit_and_unaligned`` of src/get_besthit_maf.py, G:8-56; ``-a LAST`` / ``-ga x.maf``) is the tenth
piece: of the alignments of every read the one with the largest size, the first of several, written to ``<prefix>_besthit.maf``, which
the MAF branches above read.  The `s` lines are found, parsed and chosen on the GPU from the bytes of the file (``ns_maf_besthit``,
csrc/ns_maf_best.h); this module walks the reads file and writes the files:

    unaligned_len, strandness = characterize.besthit_and_unaligned("training", "last.maf", "reads.fasta", eng)
    characterize.train_genome_from_maf("training", "last.maf", "reads.fasta", eng)      # what `read_analysis.py genome -ga last.maf` leaves

Deviations: a line whose start, size or srcSize is not made of decimal digits below 2^32 raises ValueError (Python's int() takes more);
a file without any alignment raises ValueError (the reference divides by zero); the reads file is FASTA.

Not covered: BAM input (pysam is not a dependency here: convert with ``samtools view -h``).
"""
from __future__ import annotations

import collections
import ctypes as C
import math
import os
import re
import statistics

import numpy as np

DICT_MAX = 1000                      # add_dict ignores larger values (B:15-16)
ERR_ROWS = ("mis", "ins", "del", "mis0", "ins0", "del0")
ERR_COLS = ("mis", "ins", "del")


class NsCsHist(C.Structure):
    """mirror of ns_cs_hist (include/nanosim_amd.h)"""
    _fields_ = [("cap_match2d", C.c_uint32), ("_pad", C.c_uint32), ("match_list", C.c_void_p), ("dic", (C.c_uint64 * 1001) * 5),
                ("error_list", C.c_uint64 * 18), ("first_error", C.c_uint64 * 3), ("max_match", C.c_uint64),
                ("n_match2d_overflow", C.c_uint64), ("n_skip", C.c_uint64), ("ms_kernel", C.c_double)]


class NsQualAln(C.Structure):
    """mirror of ns_qual_aln (include/nanosim_amd.h)"""
    _fields_ = [("head", C.c_uint32), ("tail", C.c_uint32), ("unmapped", C.c_uint32), ("reserved", C.c_uint32)]


class NsQualHist(C.Structure):
    """mirror of ns_qual_hist (include/nanosim_amd.h)"""
    _fields_ = [("hist", (C.c_uint64 * 128) * 5), ("n_short", C.c_uint64), ("n_bad_qual", C.c_uint64), ("ms_kernel", C.c_double)]


QUAL_TYPES = ("mis", "ins", "match", "ht", "unmapped")      # the rows of the reference's file, in its order (M:62, 85)
QUAL_VALUES = 94                                            # Phred 0 .. 93 ('!' .. '~')
QUAL_ALN_DTYPE = np.dtype([("head", "<u4"), ("tail", "<u4"), ("unmapped", "<u4"), ("reserved", "<u4")])

_MD_TOKEN = re.compile(r'(\d+)|(\^[A-Za-z]+)|([A-Za-z])')
_CIGAR_TOKEN = re.compile(r'(\d+)([MIDSHX=])')          # (no N: introns are not looked for, as in the reference)


def get_cs(cigar_str: str, md_str: str) -> str:
    """The cs string the reference derives for an alignment that carries only CIGAR + MD (B:76-132).  It models indels and mismatches,
    not bases: a mismatch is always `*ab`, an inserted base `I`.  Written as a walk of the MD items over a cursor into the CIGAR; the
    reference's corner behaviour is kept because its histograms depend on it: an MD item that ends exactly where an M block ends closes
    the block as a MATCH of the remaining length (so a mismatch in the last column of a block counts as `:1`, and an item that starts at
    a block end leaves a `:0`), and the items behind an insertion start with whatever is left of the MD count."""
    blocks = [(int(n), op) for n, op in _CIGAR_TOKEN.findall(cigar_str)]
    out = []
    at = 0              # cursor into `blocks`
    block_end = 0       # query-side end of the blocks consumed so far (M, I and S advance it)
    md_pos = 0          # how far the MD items have come on the same axis
    for count, deleted, base in _MD_TOKEN.findall(md_str):
        if deleted:
            out.append("-" + deleted[1:])
            at += 1                                         # the D block that carries it
            continue
        left = int(count) if count else 1
        while at < len(blocks) and blocks[at][1] != 'D':
            size, op = blocks[at]
            if op == 'I':
                out.append("+" + "I" * size)
            elif op == 'M':
                if md_pos + left < block_end + size:        # the item ends inside this block
                    if left > 0:
                        out.append("*ab" if base else ":%d" % left)
                    md_pos += left
                    break
                rest = block_end + size - md_pos            # ... or runs to its end: the rest of the block is a match
                out.append(":%d" % rest)
                md_pos += rest
                left -= rest
                block_end += size
                at += 1
                continue
            elif op != 'S':                                 # (H, X, = : the reference never advances on these; minimap2 -a writes M/I/D/S)
                raise ValueError("CIGAR operation %r is not handled by get_cs (src/besthit_to_histogram.py:100-129)" % op)
            block_end += size
            md_pos += size
            at += 1
    return "".join(out)


def cs_from_sam(path: str):
    """the cs string of every alignment of a SAM text file: the cs:Z tag, else from CIGAR + MD:Z (B:320-324)"""
    out = []
    with open(path) as f:
        for line in f:
            if line.startswith("@"):
                continue
            fld = line.rstrip("\n").split("\t")
            if len(fld) < 11 or fld[5] == "*":
                continue
            cs = md = None
            for t in fld[11:]:
                if t.startswith("cs:Z:"):
                    cs = t[5:]
                elif t.startswith("MD:Z:"):
                    md = t[5:]
            if cs is None:
                if md is None:
                    raise ValueError("alignment %s has neither a cs nor an MD tag" % fld[0])
                cs = get_cs(fld[5], md)
            out.append(cs)
    return out


def _pack(strings):
    """(the bytes of these str / bytes one behind the other plus a NUL as a uint8 array, their len + 1 offsets as uint64)"""
    blobs = [x.encode() if isinstance(x, str) else bytes(x) for x in strings]
    off = np.zeros(len(blobs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in blobs], out=off[1:])
    return np.frombuffer(b"".join(blobs) + b"\0", dtype=np.uint8), off


class PackedPairs:
    """Aligned line pairs that are packed already (pairs_from_sam): `ref`, `qry`, `off` as _pack_pairs returns them (a NUL byte behind
    the lines), `aln` = the ns_sam_aln figures (SAM_ALN_DTYPE) and the records they come from.  _pack_pairs, count_maf and
    count_homopolymers take it as it is; indexing or iterating gives maf_records' tuples (rname, pos - 1, reference line, query line)."""

    def __init__(self, ref, qry, off, aln, sam_recs):
        self.ref, self.qry, self.off, self.aln, self.sam_recs = ref, qry, off, aln, sam_recs

    def __len__(self):
        return len(self.off) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        lo, hi = int(self.off[i]), int(self.off[i + 1])
        return (self.sam_recs[i][2], self.sam_recs[i][3] - 1, self.ref[lo:hi].tobytes().decode(), self.qry[lo:hi].tobytes().decode())

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def heads(self):
        """[(rname, pos - 1)]: what <prefix>_hp_lengths.tsv needs of every alignment, without its lines"""
        return [(r[2], r[3] - 1) for r in self.sam_recs]


def _pack_pairs(ref_lines, query_lines=None):
    """_pack of the two lines of every alignment: (reference bytes, query bytes, the offsets of both); a PackedPairs as it is"""
    if isinstance(ref_lines, PackedPairs):
        return ref_lines.ref, ref_lines.qry, ref_lines.off
    ref, off = _pack(ref_lines)
    qry, q_off = _pack(query_lines)
    if not np.array_equal(off, q_off):
        raise ValueError("the two lines of an alignment differ in length")
    return ref, qry, off


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


def maf_pairs(path: str):
    """[(reference line, query line)] of `<prefix>_besthit.maf` as hist(prefix, "maf") reads it (B:190-198): two `s` lines per alignment;
    field 7 of each is the aligned sequence (the upper-casing is done by the counting walk).  The file get_besthit_maf writes holds `s`
    lines only, and the reference assumes that; here everything else a MAF file may carry (`#` headers, `a score=` lines, blank
    separators) is skipped, and an `s` line without its partner is a ValueError."""
    out, pend = [], None
    with open(path) as f:
        for line in f:
            if not line.startswith("s ") and not line.startswith("s\t"):
                continue
            r = line.split()
            if pend is None:
                pend = r
                continue
            r, q, pend = pend, r, None
            if len(r) < 7 or len(q) < 7 or len(r[6]) > len(q[6]):
                raise ValueError("%s: not two `s` lines with an aligned sequence each (the reference would stop with an IndexError)" % path)
            out.append((r[6], q[6][:len(r[6])]))                   # (the walk runs over len(ref), B:203)
    if pend is not None:
        raise ValueError("%s: an `s` line without its partner (odd number of `s` lines)" % path)
    return out


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
        with open(prefix + name, "w") as f:
            f.write(text)
    return t


# ---- the base-quality model (src/model_base_qualities.py) ------------------------------------------------------------------------------
_CLIP_HEAD = re.compile(r'^(?:\d+H)?(\d+)S')
_CLIP_TAIL = re.compile(r'(\d+)S(?:\d+H)?$')


def quals_from_sam(path: str, primary_only: bool = True):
    """(aligned, unmapped) of a SAM text file.  aligned: [(cs, QUAL, head, tail)] of the records without flag 0x4 and 0x100 (and, with
    primary_only, without 0x800: what get_primary_sam keeps) — the cs:Z tag, else from CIGAR + MD:Z; head / tail: the leading / trailing
    soft clip (query_alignment_start, len - query_alignment_end; hard clips are not in QUAL).  unmapped: the QUAL strings of the flag 0x4
    records (src/get_primary_sam.py:172-175; a missing QUAL is skipped there, and is a ValueError on an aligned record)."""
    aligned, unmapped = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("@"):
                continue
            fld = line.rstrip("\n").split("\t")
            if len(fld) < 11:
                continue
            flag = int(fld[1])
            if flag & 0x4:
                if fld[10] != "*":
                    unmapped.append(fld[10])
                continue
            if flag & 0x100 or (primary_only and flag & 0x800):
                continue
            if fld[10] == "*":
                raise ValueError("alignment %s has no QUAL" % fld[0])
            cs = md = None
            for t in fld[11:]:
                if t.startswith("cs:Z:"):
                    cs = t[5:]
                elif t.startswith("MD:Z:"):
                    md = t[5:]
            if cs is None:
                if md is None:
                    raise ValueError("alignment %s has neither a cs nor an MD tag" % fld[0])
                cs = get_cs(fld[5], md)
            h, t = _CLIP_HEAD.match(fld[5]), _CLIP_TAIL.search(fld[5])
            aligned.append((cs, fld[10], int(h.group(1)) if h else 0, int(t.group(1)) if t else 0))
    return aligned, unmapped


def _qual_call(eng, entries) -> NsQualHist:
    """ns_qual_histograms on [(cs, QUAL, head, tail, unmapped)], in this order"""
    cs_data, cs_off = _pack([e[0] for e in entries])
    q_data, q_off = _pack([e[1] for e in entries])
    aln = np.zeros(len(entries), dtype=QUAL_ALN_DTYPE)
    for i, e in enumerate(entries):
        aln[i] = (e[2], e[3], 1 if e[4] else 0, 0)
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
    with open(prefix + "_base_qualities_model_parameters.tsv", "w") as f:
        f.write(format_base_qualities(fit_qualities(t["hist"])))
    return t


# ---- the homopolymer-length model (src/model_homopolymer_lengths.py) -------------------------------------------------------------------
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
    out, pend = [], None
    with open(path) as f:
        for line in f:
            if not line.startswith("s ") and not line.startswith("s\t"):
                continue
            r = line.split()
            if pend is None:
                pend = r
                continue
            r, q, pend = pend, r, None
            if len(r) < 7 or len(q) < 7 or len(r[6]) > len(q[6]):
                raise ValueError("%s: not two `s` lines with an aligned sequence each (the reference would stop with an IndexError)" % path)
            out.append((r[1], int(r[2]), r[6], q[6][:len(r[6])]))
    if pend is not None:
        raise ValueError("%s: an `s` line without its partner (odd number of `s` lines)" % path)
    return out


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


def homopolymer_lengths(prefix: str, records_or_pairs, eng, min_hp_len: int = 5, lengths_file: bool = True) -> dict:
    """writes <prefix>_hp_lengths_model_parameters.tsv like model_homopolymer_lengths (H:212-243) and, with lengths_file,
    <prefix>_hp_lengths.tsv like analyze_homopolymers (H:126-138; it needs maf_records' tuples: the reference name and start);
    returns the counts"""
    if lengths_file and any(len(r) < 4 for r in records_or_pairs):
        raise ValueError("<prefix>_hp_lengths.tsv needs the reference name and start of every alignment (maf_records)")
    t = count_homopolymers(eng, records_or_pairs, min_hp_len, records=lengths_file)
    if lengths_file:
        with open(prefix + "_hp_lengths.tsv", "w") as f:
            f.write(format_hp_lengths(records_or_pairs, t["records"]))
    with open(prefix + "_hp_lengths_model_parameters.tsv", "w") as f:
        f.write(format_hp_model(fit_homopolymers(t["table"], t["columns"])))
    return t


# ---- SAM input: the line pairs (samtools view | sam2pairwise, then src/pairwise2maf.py) -------------------------------------------------
class NsSamPairs(C.Structure):
    """mirror of ns_sam_pairs (include/nanosim_amd.h)"""
    _fields_ = [("ref_lines", C.c_void_p), ("query_lines", C.c_void_p), ("cap_bytes", C.c_uint64), ("aln_off", C.c_void_p), ("aln", C.c_void_p),
                ("n_bytes", C.c_uint64), ("n_bad", C.c_uint64), ("first_bad", C.c_uint64), ("ms_kernel", C.c_double)]


SAM_ALN_DTYPE = np.dtype([("head", "<u4"), ("tail", "<u4"), ("ref_len", "<u4"), ("query_len", "<u4")])      # ns_sam_aln


def sam_records(path: str):
    """[(qname, flag, rname, pos, cigar, md, seq)] of a SAM text file: the records pairwise2maf keeps — FLAG exactly 0 or 16 (P:46-51) —
    in file order.  A kept record without MD:Z, or with `H` in its CIGAR (the reference's int() stops there, P:59-67), raises ValueError."""
    out = []
    with open(path) as f:
        for line in f:
            if line.startswith("@"):
                continue
            fld = line.rstrip("\n").split("\t")
            if len(fld) < 11 or fld[1] not in ("0", "16"):
                continue
            md = None
            for t in fld[11:]:
                if t.startswith("MD:Z:"):
                    md = t[5:]
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
    p.aln_off, p.aln = bufs["off"].ctypes.data, bufs["aln"].ctypes.data if n else None
    if lines:
        p.ref_lines, p.query_lines, p.cap_bytes = bufs["ref"].ctypes.data, bufs["qry"].ctypes.data, cap
    return p, bufs


def _sam_packed(sam_recs, p, bufs) -> PackedPairs:
    if p.n_bad:
        r = sam_recs[int(p.first_bad)]
        raise ValueError("%d SAM record(s) whose CIGAR, MD and SEQ do not describe an alignment; the first is record %d (%s): CIGAR %.60s, MD %.60s, %d bases"
                         % (p.n_bad, p.first_bad, r[0], r[4], r[5], len(r[6])))
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
    with open(path, "w") as f:
        f.write(format_maf(sam_recs, packed))


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
    if lengths_file:
        with open(prefix + "_hp_lengths.tsv", "w") as f:
            f.write(format_hp_lengths(t["pairs"], t["records"]))
    with open(prefix + "_hp_lengths_model_parameters.tsv", "w") as f:
        f.write(format_hp_model(fit_homopolymers(t["table"], t["columns"])))
    return t


# ---- the error-length mixtures (src/model_fitting.py) ----------------------------------------------------------------------------------
class NsMixfitFit(C.Structure):
    """mirror of ns_mixfit_fit (include/nanosim_amd.h)"""
    _fields_ = [("x", C.c_double * 4), ("fun", C.c_double), ("residual", C.c_double), ("nfev", C.c_uint32), ("nit", C.c_uint32),
                ("status", C.c_int32), ("reserved", C.c_uint32)]


class NsMixfitResult(C.Structure):
    """mirror of ns_mixfit_result (include/nanosim_amd.h)"""
    _fields_ = [("fits", C.c_void_p), ("ms_kernel", C.c_double)]


MIXFIT_DTYPE = np.dtype([("x", "<f8", (4,)), ("fun", "<f8"), ("residual", "<f8"), ("nfev", "<u4"), ("nit", "<u4"), ("status", "<i4"),
                         ("reserved", "<u4")])
MIXFIT_MISMATCH, MIXFIT_INDEL = 0, 1                        # NS_MIXFIT_*
MIXFIT_FIT, MIXFIT_EVALUATE = 0, 1
MIXFIT_TYPES = (("mis", "mismatch", "_mis.hist"), ("ins", "insertion", "_ins.hist"), ("del", "deletion", "_del.hist"))   # F:112-114, 136, 169, 203


def read_length_hist(path: str) -> dict:
    """{length: count} of a `_mis.hist` / `_ins.hist` / `_del.hist` file (F:28-33)"""
    h = {}
    with open(path) as f:
        f.readline()
        for line in f:
            info = line.strip().split()
            h[int(info[0])] = int(info[1])
    return h


def empirical_cdf(hist: dict, error: str):
    """(cdf, number of observations) as read_histogram (F:34-45) returns them for a {length: count} dict, without the list of
    observations: error "mis" — lengths shifted by one, max bins — or "indel" — max - 1 bins, so the last bin takes the two largest
    lengths.  np.histogram(density=True) divides by the bin width, which is 1 only when the smallest length present is the domain's
    first: kept.  A histogram that leaves no bin raises ValueError (numpy does in the reference)."""
    if error not in ("mis", "indel"):
        raise ValueError("error must be 'mis' or 'indel'")
    shift = 1 if error == "mis" else 0
    vals = sorted(k - shift for k, v in hist.items() if v > 0)
    if not vals:
        raise ValueError("empty histogram")
    bins = vals[-1] if error == "mis" else vals[-1] - 1
    if bins < 1:
        raise ValueError("the histogram leaves no bin (largest length %d)" % (vals[-1] + shift))
    w = np.array([hist[v + shift] for v in vals], dtype=np.float64)
    pmf, _ = np.histogram(np.array(vals, dtype=np.int64), bins=bins, weights=w, density=True)
    return np.cumsum(pmf), int(w.sum())


def fit_starts(error: str) -> np.ndarray:
    """the reference's grid of starts in its order: (512, 3) for "mis" (F:120-121), (9216, 4) for "indel" (F:153-154, 186-187) — whose
    tuples are built as (l, p, k, w) and read as (l, k, p, w) by ins_ll: kept, so column 1 runs over 0.1 .. 1.2 and column 2 over 0.1 .. 0.8"""
    a = np.arange
    if error == "mis":
        g = [(l, p, w) for l in a(0.1, 0.9, 0.1) for p in a(0.1, 0.9, 0.1) for w in a(0.1, 0.9, 0.1)]
    elif error == "indel":
        g = [(l, p, k, w) for l in a(0.1, 1.3, 0.1) for p in a(0.1, 1.3, 0.1) for k in a(0.1, 0.9, 0.1) for w in a(0.1, 0.9, 0.1)]
    else:
        raise ValueError("error must be 'mis' or 'indel'")
    return np.array(g, dtype=np.float64)


def mixture_fit(eng, error: str, cdf, starts, evaluate: bool = False) -> dict:
    """ns_mixture_fit: one Nelder-Mead search per start (or, with evaluate, the objective at each point).
    {"x": (n, 3 or 4), "fun", "residual", "nfev", "nit", "status": (n,), "ms_kernel"}"""
    dim = 3 if error == "mis" else 4
    cdf = np.ascontiguousarray(cdf, dtype=np.float64)
    starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, dim)
    fits = np.zeros(len(starts), dtype=MIXFIT_DTYPE)
    r = NsMixfitResult()
    r.fits = fits.ctypes.data
    eng._check(eng.L.ns_mixture_fit(eng.ctx, MIXFIT_MISMATCH if error == "mis" else MIXFIT_INDEL, cdf.ctypes.data, len(cdf), starts.ctypes.data,
                                    len(starts), MIXFIT_EVALUATE if evaluate else MIXFIT_FIT, C.byref(r)))
    out = {k: fits[k].copy() for k in ("fun", "residual", "nfev", "nit", "status")}
    out["x"] = fits["x"][:, :dim].copy()
    out["ms_kernel"] = float(r.ms_kernel)
    return out


def select_fit(error: str, x, residual):
    """the index the reference's loop ends on (F:126-146, 160-179): the smallest residual whose parameters pass the validity test of
    F:131 / F:164, the earlier start on a tie (list.sort is stable); a NaN residual never wins.  None when no start qualifies."""
    x, residual = np.asarray(x), np.asarray(residual)
    if error == "mis":
        ok = (x[:, 0] > 0) & (x[:, 1] > 0) & (x[:, 1] < 1) & (x[:, 2] > 0) & (x[:, 2] < 1)
    else:
        ok = (x[:, 0] > 0) & (x[:, 1] > 0) & (x[:, 2] > 0) & (x[:, 2] < 1) & (x[:, 3] > 0) & (x[:, 3] < 1)
    ok &= ~np.isnan(residual)
    if not ok.any():
        return None
    r = np.where(ok, residual, np.inf)
    return int(np.argmin(r))                                # (the first of equal minima)


def fit_mixtures(eng, hists: dict) -> dict:
    """hists: {"mis" | "ins" | "del": {length: count}}.  Three calls of ns_mixture_fit over the reference's grids; per type
    {"params", "residual", "precision" = 1.36 / sqrt(n) (F:128), "warning": residual > precision (the reference's WARNING line), "start",
    "n_obs", "ms_kernel"}"""
    out = {}
    for t, _, _ in MIXFIT_TYPES:
        error = "mis" if t == "mis" else "indel"
        cdf, n_obs = empirical_cdf(hists[t], error)
        res = mixture_fit(eng, error, cdf, fit_starts(error))
        i = select_fit(error, res["x"], res["residual"])
        if i is None:
            raise ValueError("no search of the %s grid ended on valid parameters" % t)
        precision = 1.36 / math.sqrt(n_obs)
        out[t] = dict(params=[float(v) for v in res["x"][i]], residual=float(res["residual"][i]), precision=precision,
                      warning=bool(res["residual"][i] > precision), start=i, n_obs=n_obs, ms_kernel=res["ms_kernel"])
    return out


def format_model_profile(fit: dict) -> str:
    """the text of <prefix>_model_profile (F:110, 136, 169, 203): the mismatch row carries a literal 0 in the k column"""
    m, i, d = fit["mis"]["params"], fit["ins"]["params"], fit["del"]["params"]
    s = "Type\tlambda\tk\tprob\tweight\n"
    s += "mismatch\t" + str(m[0]) + '\t0\t' + str(m[1]) + '\t' + str(m[2]) + '\n'
    s += "insertion\t" + str(i[0]) + '\t' + str(i[1]) + '\t' + str(i[2]) + '\t' + str(i[3]) + '\n'
    s += "deletion\t" + str(d[0]) + '\t' + str(d[1]) + '\t' + str(d[2]) + '\t' + str(d[3]) + '\n'
    return s


def model_fitting(prefix: str, eng) -> dict:
    """model_fitting(prefix, threads) (F:108-217): reads <prefix>_mis.hist, _ins.hist and _del.hist as hist() wrote them and writes
    <prefix>_model_profile; returns fit_mixtures' dict"""
    fit = fit_mixtures(eng, {t: read_length_hist(prefix + suffix) for t, _, suffix in MIXFIT_TYPES})
    with open(prefix + "_model_profile", "w") as f:
        f.write(format_model_profile(fit))
    return fit


# ---- the read-length models (src/head_align_tail_dist.py, src/get_primary_sam.py:145-217) ----------------------------------------------
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


def _sam_refs(fld, refs):
    """an @SQ line's (SN, LN) behind `refs`"""
    tags = dict(t.split(":", 1) for t in fld[1:] if ":" in t)
    if "SN" in tags and "LN" in tags:
        refs.append((tags["SN"], int(tags["LN"])))


def length_records(path: str):
    """(refs, records) of a SAM text file: refs = [(SN, LN)] of its @SQ lines, records = [(qname, flag, rname, pos, cigar)] of every
    record whose CIGAR is not `*`, in file order — the reference's `<prefix>_primary` file (A:127-134) as SAM text.  A record on a
    reference without an @SQ line raises ValueError (the reference stops with a KeyError, A:138, 156)."""
    refs, records = [], []
    with open(path) as f:
        for line in f:
            fld = line.rstrip("\n").split("\t")
            if line.startswith("@"):
                if fld[0] == "@SQ":
                    _sam_refs(fld, refs)
                continue
            if len(fld) < 6 or fld[5] == "*":
                continue
            records.append((fld[0], int(fld[1]), fld[2], int(fld[3]), fld[5]))
    known = set(n for n, _ in refs)
    for r in records:
        if r[2] not in known:
            raise ValueError("alignment %s lies on %s, which has no @SQ line" % (r[0], r[2]))
    return refs, records


def primary_and_unaligned(path: str):
    """(refs, records, unaligned_len, strandness) of a whole SAM text file, as primary_and_unaligned does without a metagenome list
    (G:163-187): refs and records as length_records gives them, of the primary records (FLAG without 0x4, 0x100 and 0x800);
    unaligned_len: int64 array of len(SEQ), 0 for `*`, of the 0x4 records (query_length); strandness = records whose FLAG is 0 over the
    primary records.  No primary record raises ValueError (the reference divides by zero)."""
    refs, records, unaligned = [], [], []
    pos_strand = 0
    with open(path) as f:
        for line in f:
            fld = line.rstrip("\n").split("\t")
            if line.startswith("@"):
                if fld[0] == "@SQ":
                    _sam_refs(fld, refs)
                continue
            if len(fld) < 11:
                continue
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
    ref_index = {}
    for i, (name, _) in enumerate(refs):
        ref_index.setdefault(name, i)
    ref_id = np.zeros(n, dtype=np.uint32)
    ref_start = np.zeros(n, dtype=np.uint64)
    for i, r in enumerate(records):
        if r[2] not in ref_index:
            raise ValueError("alignment %s lies on %s, which has no @SQ line" % (r[0], r[2]))
        if r[3] < 1:
            raise ValueError("alignment %s has POS %d" % (r[0], r[3]))
        ref_id[i], ref_start[i] = ref_index[r[2]], r[3] - 1
    cg, cg_off = _pack([r[4] for r in records])
    reverse = np.array([1 if r[1] & 0x10 else 0 for r in records], dtype=np.uint8)
    ref_total = np.array([ln for _, ln in refs], dtype=np.uint64)
    read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
    aln = np.zeros(n, dtype=LEN_ALN_DTYPE)
    reads = np.zeros(n_reads, dtype=LEN_READ_DTYPE)
    segments = np.zeros(n, dtype=np.uint64)
    out = NsLenResult()
    out.aln, out.reads, out.segments = (aln.ctypes.data if n else None), (reads.ctypes.data if n_reads else None), (segments.ctypes.data if n else None)
    eh = et = None
    if extra is not None:
        eh, et = np.ascontiguousarray(extra[0], dtype=np.uint32), np.ascontiguousarray(extra[1], dtype=np.uint32)
    eng._check(eng.L.ns_read_lengths(eng.ctx, cg.ctypes.data, cg_off.ctypes.data, reverse.ctypes.data, ref_id.ctypes.data, ref_start.ctypes.data,
                                     ref_total.ctypes.data, len(refs), read_off.ctypes.data, n_reads, n, mode,
                                     eh.ctypes.data if eh is not None else None, et.ctypes.data if et is not None else None, C.byref(out)))
    if out.n_bad:
        r = records[int(out.first_bad)]
        raise ValueError("%d SAM record(s) whose CIGAR is not one or covers no reference base; the first is record %d (%s): CIGAR %.60s"
                         % (out.n_bad, out.first_bad, r[0], r[4]))
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
    aligned, total_ref, total, heads, hts = [], [], [], [], []
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
            aligned.append(int(r[3]))
            total_ref.append(int(r[5]))
            heads.append(int(q[2]))
            total.append(int(q[5]))
            hts.append(int(q[5]) - int(q[3]))
    if pend is not None:
        raise ValueError("%s: an `s` line without its partner (odd number of `s` lines)" % path)
    head, ht = np.array(heads, dtype=np.int64), np.array(hts, dtype=np.int64)
    take = ht != 0
    out = dict(aligned_ref_length=np.array(aligned, dtype=np.int64), total_length=np.array(total, dtype=np.int64), ht_length=ht, head=head, tail=ht - head,
               head_vs_ht_ratio=head[take].astype(np.float64) / ht[take].astype(np.float64), ms_kernel=0.0)
    if mode == "transcriptome":
        out["total_ref_length"] = np.array(total_ref, dtype=np.int64)
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
    figures = count_read_lengths(eng, refs, records, mode, genome_records)
    write_kde(prefix, kde_models(figures, unaligned_len), pickles, merge)        # (merge: the keys of other models, gap_length of chimeric(), stay)
    with open(prefix + "_strandness_rate", "w") as f:
        f.write(format_strandness(strandness))
    with open(prefix + "_reads_alignment_rate", "w") as f:
        f.write(format_alignment_rate(len(figures["total_length"]), 0 if unaligned_len is None else len(unaligned_len)))
    return figures


# ---- chimeric reads: the split-alignment choice (src/get_primary_sam.py:220-478) --------------------------------------------------------------
class NsChimResult(C.Structure):
    """mirror of ns_chim_result (include/nanosim_amd.h)"""
    _fields_ = [("ent", C.c_void_p), ("pieces", C.c_void_p), ("reads", C.c_void_p), ("species_count", C.c_void_p), ("n_gaps", C.c_uint64),
                ("pos_strand", C.c_uint64), ("n_bad", C.c_uint64), ("first_bad", C.c_uint64), ("ms_kernel", C.c_double), ("ms_scan", C.c_double)]


CHIM_ENT_DTYPE = np.dtype([("qstart", "<u4"), ("qend", "<u4"), ("qlen", "<u4"), ("rlen", "<u4")])          # ns_chim_ent
CHIM_PIECE_DTYPE = np.dtype([("entry", "<u4"), ("is_primary", "<u4"), ("gap", "<i8")])                     # ns_chim_piece
CHIM_READ_DTYPE = np.dtype([("n_pieces", "<u4"), ("flags", "<u4")])                                        # ns_chim_read
CHIM_NO_GAP = -1                                            # NS_CHIM_NO_GAP
CHIM_POS_STRAND, CHIM_ALONE, CHIM_HAS_SA = 1, 2, 4          # NS_CHIM_*: ns_chim_read.flags

# a record of chimeric_records; [:5] is a record of length_records.  nm: int or None; sa: the SA:Z text or None; seq_len: len(SEQ), 0 for `*`
ChimRecord = collections.namedtuple("ChimRecord", "qname flag rname pos cigar nm sa seq_len line")


def species_of_reference(name: str) -> str:
    """the species of a metagenome reference `<species>_<chromosome>` (G:260)"""
    return "_".join(name.split("_")[:-1])


def sa_entries(sa: str, qname: str = "?"):
    """[(rname, ref_start 0-based, reverse, cigar, nm)] of an SA:Z text as the reference takes it apart (G:290, 297-300): split at `;`,
    the LAST part dropped (the empty one behind the closing `;` — an entry without it is lost, as there), six fields each"""
    out = []
    for part in sa.split(";")[:-1]:
        fld = part.split(",")
        if len(fld) != 6:
            raise ValueError("read %s: an SA entry does not have six comma-separated fields: %.60s" % (qname, part))
        try:
            pos, nm = int(fld[1]), int(fld[5])
        except ValueError:
            raise ValueError("read %s: position or NM of an SA entry is no number: %.60s" % (qname, part)) from None
        if pos < 1 or nm < 0:
            raise ValueError("read %s: position or NM of an SA entry is out of range: %.60s" % (qname, part))
        out.append((fld[0], pos - 1, fld[2] != "+", fld[3], nm))
    return out


def chimeric_records(path: str):
    """(refs, records, unaligned_len, header) of a whole SAM text file, one pass: refs = [(SN, LN)] of the @SQ lines, records = a
    ChimRecord for every record that is not unmapped, in file order, unaligned_len = int64 array of len(SEQ) of the 0x4 records (0 for
    `*`), header = the `@` lines as they stand.  ValueError where the reference stops or misbehaves: a primary record without NM:i (its
    get_tag raises outside the try, G:279), an SA entry without six fields (G:298), a reference name — of a record or of an SA entry —
    without an @SQ line, a supplementary or secondary record in front of the first primary (a NameError at G:400), no primary at all."""
    refs, records, unaligned, header = [], [], [], []
    seen_primary = False
    with open(path) as f:
        for line in f:
            if line.startswith("@"):
                header.append(line)
                fld = line.rstrip("\n").split("\t")
                if fld[0] == "@SQ":
                    _sam_refs(fld, refs)
                continue
            fld = line.rstrip("\n").split("\t")
            if len(fld) < 11:
                continue
            flag = int(fld[1])
            seq_len = 0 if fld[9] == "*" else len(fld[9])
            if flag & 0x4:
                unaligned.append(seq_len)
                continue
            nm = sa = None
            for t in fld[11:]:
                if t.startswith("NM:i:"):
                    nm = int(t[5:])
                elif t.startswith("SA:Z:"):
                    sa = t[5:]
            if not flag & (0x100 | 0x800):
                seen_primary = True
                if nm is None:
                    raise ValueError("primary alignment of read %s has no NM:i tag" % fld[0])
                if nm < 0:
                    raise ValueError("primary alignment of read %s has a negative NM" % fld[0])
            elif not seen_primary:
                raise ValueError("record of read %s (FLAG %d) stands in front of the first primary alignment" % (fld[0], flag))
            records.append(ChimRecord(fld[0], flag, fld[2], int(fld[3]), fld[5], nm, sa, seq_len, line))
    if not seen_primary:
        raise ValueError("%s holds no primary alignment" % path)
    known = set(n for n, _ in refs)
    for r in records:
        if r.rname not in known:
            raise ValueError("alignment %s lies on %s, which has no @SQ line" % (r.qname, r.rname))
        if r.sa is not None and not r.flag & (0x100 | 0x800):
            for e in sa_entries(r.sa, r.qname):
                if e[0] not in known:
                    raise ValueError("an SA entry of read %s lies on %s, which has no @SQ line" % (r.qname, e[0]))
    return refs, records, np.array(unaligned, dtype=np.int64), header


def cigar_spans(eng, cigars):
    """ns_cigar_spans: (cigar_parser's figures per CIGAR (CHIM_ENT_DTYPE), n_bad, first_bad, ms_kernel)"""
    n = len(cigars)
    cg, cg_off = _pack(cigars)
    out = np.zeros(n, dtype=CHIM_ENT_DTYPE)
    n_bad, first_bad, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
    eng._check(eng.L.ns_cigar_spans(eng.ctx, cg.ctypes.data, cg_off.ctypes.data, n, out.ctypes.data if n else None, C.addressof(n_bad),
                                    C.addressof(first_bad), C.addressof(ms)))
    return out, int(n_bad.value), int(first_bad.value), float(ms.value)


def chimeric_call(eng, reads, ref_total, species, n_species: int):
    """ns_chimeric_select on reads = [[(cigar, ref_id, ref_start, nm, reverse), ...]] (entry 0 of each the primary):
    (the NsChimResult, ent, pieces, per read, species_count[n_species][2], ent_off); nothing is raised for bad CIGARs"""
    ent_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=ent_off[1:])
    flat = [e for r in reads for e in r]
    n = len(flat)
    cg, cg_off = _pack([e[0] for e in flat])
    ref_id = np.array([e[1] for e in flat], dtype=np.uint32)
    ref_start = np.array([e[2] for e in flat], dtype=np.uint64)
    nm = np.array([e[3] for e in flat], dtype=np.uint32)
    reverse = np.array([1 if e[4] else 0 for e in flat], dtype=np.uint8)
    ref_total = np.ascontiguousarray(ref_total, dtype=np.uint64)
    species = np.ascontiguousarray(species, dtype=np.uint32)
    ent, pieces = np.zeros(n, dtype=CHIM_ENT_DTYPE), np.zeros(n, dtype=CHIM_PIECE_DTYPE)
    per_read = np.zeros(len(reads), dtype=CHIM_READ_DTYPE)
    count = np.zeros((n_species, 2), dtype=np.uint64)
    out = NsChimResult()
    out.ent, out.pieces, out.reads, out.species_count = ent.ctypes.data, pieces.ctypes.data, per_read.ctypes.data, count.ctypes.data
    eng._check(eng.L.ns_chimeric_select(eng.ctx, cg.ctypes.data, cg_off.ctypes.data, ent_off.ctypes.data, len(reads), ref_id.ctypes.data,
                                        ref_start.ctypes.data, nm.ctypes.data, reverse.ctypes.data, ref_total.ctypes.data, species.ctypes.data,
                                        len(ref_total), n_species, C.byref(out)))
    return out, ent, pieces, per_read, count, ent_off


def select_chimeric(eng, refs, records, species=None) -> dict:
    """What primary_and_unaligned_chimeric decides (G:267-410) for the records of chimeric_records, from the GPU (ns_chimeric_select over
    the primary alignments and their SA entries, ns_cigar_spans over the supplementary and secondary records).
    species: None — every reference is of one species, which is what the reference's genome mode does in effect (`species` keeps the value
    the header loop left, G:260, so only the "same" column moves); or {reference name: species}, e.g. built with species_of_reference.
    "selected": indices into `records` in the reference's written order — reads in primary order, the pieces of a chimeric read in query
    order (a piece the reference takes for the primary — its qstart is the primary's — is the primary record); "gap_length": int64, in
    read order, then piece order; "num_aligned"; "pos_strand"; "strandness"; "species_count": {species: [same, other]} (the key None
    without a mapping); "n_pieces" per read; "flags" per read (CHIM_*); "ent", "ent_off"; "ms_kernel", "ms_scan", "ms_spans"; and, for
    quant_items, "pieces", "primaries" / "others" (indices into `records`) and "spans" (cigar_parser's figures of the others).
    A non-primary piece is matched as the reference does (G:397-402): among the supplementary and secondary records between this primary
    and the next one, whatever their QNAME, the LAST one with equal (RNAME, cigar_parser qstart, qend, POS - 1).  A piece without a
    record raises ValueError naming the read; so does a CIGAR that is not one."""
    ref_index = {}
    for i, (name, _) in enumerate(refs):
        ref_index.setdefault(name, i)
    if species is None:
        names, sp_of = [None], [0] * len(refs)
    else:
        names = list(dict.fromkeys(species[name] for name, _ in refs))
        sp_index = {s: i for i, s in enumerate(names)}
        sp_of = [sp_index[species[name]] for name, _ in refs]
    primaries = [i for i, r in enumerate(records) if not r.flag & (0x4 | 0x100 | 0x800)]
    if not primaries:
        raise ValueError("no primary alignment")
    others = [i for i, r in enumerate(records) if r.flag & (0x100 | 0x800) and not r.flag & 0x4]
    reads, tags = [], []
    for i in primaries:
        r = records[i]
        if r.nm is None:
            raise ValueError("primary alignment of read %s has no NM:i tag" % r.qname)
        sa = sa_entries(r.sa, r.qname) if r.sa is not None else []
        for e in [(r.rname,)] + sa:
            if e[0] not in ref_index:
                raise ValueError("an alignment of read %s lies on %s, which has no @SQ line" % (r.qname, e[0]))
        if r.pos < 1:
            raise ValueError("alignment %s has POS %d" % (r.qname, r.pos))
        reads.append([(r.cigar, ref_index[r.rname], r.pos - 1, r.nm, bool(r.flag & 0x10))] + [(e[3], ref_index[e[0]], e[1], e[4], e[2]) for e in sa])
        tags.append(sa)
    out, ent, pieces, per_read, count, ent_off = chimeric_call(eng, reads, [ln for _, ln in refs], sp_of, len(names))
    if out.n_bad:
        bad = int(out.first_bad)
        r = int(np.searchsorted(ent_off, bad, side="right")) - 1
        raise ValueError("%d CIGAR(s) that are not one among the primary alignments and their SA entries; the first is entry %d of read %s: %.60s"
                         % (out.n_bad, bad - int(ent_off[r]), records[primaries[r]].qname, reads[r][bad - int(ent_off[r])][0]))
    spans, n_bad, first_bad, ms_spans = cigar_spans(eng, [records[i].cigar for i in others])
    if n_bad:
        r = records[others[first_bad]]
        raise ValueError("%d supplementary / secondary record(s) whose CIGAR is not one; the first is a record of read %s: %.60s" % (n_bad, r.qname, r.cigar))
    selected, gaps = [], []
    at = 0                                                   # the next of `others` behind the current primary
    for k, i in enumerate(primaries):
        nxt = primaries[k + 1] if k + 1 < len(primaries) else len(records)
        while at < len(others) and others[at] < i:
            at += 1
        e0, n = int(ent_off[k]), int(per_read["n_pieces"][k])
        own = pieces[e0:e0 + n]
        if not (own["is_primary"] == 1).all():
            found = {}
            j = at
            while j < len(others) and others[j] < nxt:       # first to last: the last record with a key keeps it
                o = records[others[j]]
                found[(o.rname, int(spans["qstart"][j]), int(spans["qend"][j]), o.pos - 1)] = others[j]
                j += 1
        for p in own:
            if p["gap"] != CHIM_NO_GAP:
                gaps.append(int(p["gap"]))
            if p["is_primary"]:
                selected.append(i)
                continue
            e = int(p["entry"])
            tag = tags[k][e - 1]
            key = (tag[0], int(ent["qstart"][e0 + e]), int(ent["qend"][e0 + e]), tag[1])
            if key not in found:
                raise ValueError("read %s: no supplementary or secondary record matches the chosen SA entry %s,%d,%s (query %d-%d)"
                                 % (records[i].qname, tag[0], tag[1] + 1, "-" if tag[2] else "+", key[1], key[2]))
            selected.append(found[key])
    assert len(gaps) == out.n_gaps
    return dict(selected=selected, gap_length=np.array(gaps, dtype=np.int64), num_aligned=len(primaries), pos_strand=int(out.pos_strand),
                strandness=float(out.pos_strand) / len(primaries), species_count={s: [int(count[i, 0]), int(count[i, 1])] for i, s in enumerate(names)},
                n_pieces=per_read["n_pieces"].astype(np.int64), flags=per_read["flags"].copy(), ent=ent, ent_off=ent_off,
                ms_kernel=float(out.ms_kernel), ms_scan=float(out.ms_scan), ms_spans=ms_spans,
                pieces=pieces, primaries=primaries, others=others, spans=spans)          # (for quant_items)


def chimeric_beta(species_count: dict, abundance: dict) -> float:
    """the shrinkage rate (G:449-455, 475): the median over the species with a recorded gap of other / (same + other) * 100 /
    (100 - abundance), abundance in percent (the reference's come from its EM, G:428: the caller's here)"""
    betas = []
    for sp, counts in species_count.items():
        other_prob = 100 - abundance[sp]
        if counts[0] + counts[1] == 0:
            continue
        betas.append(counts[1] / (counts[0] + counts[1]) * 100 / other_prob)
    if not betas:
        raise ValueError("no gap between pieces was recorded: there is no shrinkage rate")
    return statistics.median(betas)


def format_chimeric_info(n_gaps: int, num_aligned: int, beta=None) -> str:
    """the text of <prefix>_chimeric_info (G:472-475); the second line, written in metagenome mode, has no newline"""
    text = "Mean segments for each aligned read:\t" + str((n_gaps + num_aligned) / num_aligned) + "\n"
    if beta is not None:
        text += "Shrinkage rate (beta):\t" + str(beta)
    return text


def chimeric(prefix: str, path: str, eng, species=None, abundance=None, primary_sam: bool = True, pickles=None, quantify=None, normalize: bool = True):
    """primary_and_unaligned_chimeric (G:220-478): writes <prefix>_chimeric_info, adds gap_length —
    log10(gap + 1), bandwidth 0.01 (G:465-469) — to <prefix>_kde.npz next to the keys it holds (and writes <prefix>_gap_length.pkl by
    write_kde's rule), and, with primary_sam, <prefix>_primary.sam: the header and the selected lines, unchanged, in the reference's
    order — what its later steps read from <prefix>_primary.bam, for cs_from_sam, quals_from_sam, sam_records and length_records.
    abundance ({species: percent}, with a species mapping): the second line of _chimeric_info (chimeric_beta).
    quantify: None — no quantification, as before; "meta" — the EM over the species (species: the mapping, by default
    species_of_reference of every @SQ name) writes <prefix>_quantification.tsv and its abundances stand behind the shrinkage rate
    (abundance= next to it is a ValueError); "trans" — the EM over the transcripts writes the file (normalize: EM_trans').
    -> (refs, records, unaligned_len, strandness): read_lengths' arguments, the records being the selected ones."""
    if quantify not in (None, "meta", "trans"):
        raise ValueError("quantify must be None, 'meta' or 'trans'")
    if quantify == "meta" and abundance is not None:
        raise ValueError("quantify='meta' computes the abundances: abundance= cannot be given as well")
    if abundance is not None and species is None:
        raise ValueError("abundance needs the species mapping")
    refs, records, unaligned_len, header = chimeric_records(path)
    if quantify == "meta" and species is None:
        species = {name: species_of_reference(name) for name, _ in refs}
    sel = select_chimeric(eng, refs, records, species)
    if quantify is not None:
        items = quant_items(records, sel, refs, species if quantify == "meta" else None)
        res = em_quantify(eng, items, quant_targets(refs, quantify, species), quantify, normalize)
        with open(prefix + "_quantification.tsv", "w") as f:
            f.write(format_quantification(quantify, res["result"]))
        if quantify == "meta":
            abundance = res["result"]
    beta = chimeric_beta(sel["species_count"], abundance) if abundance is not None else None
    with open(prefix + "_chimeric_info", "w") as f:
        f.write(format_chimeric_info(len(sel["gap_length"]), sel["num_aligned"], beta))
    write_kde(prefix, {"gap_length": (np.log10(sel["gap_length"] + 1).astype(np.float64), 0.01)}, pickles, merge=True)
    if primary_sam:
        with open(prefix + "_primary.sam", "w") as f:
            f.writelines(header)
            f.writelines(records[i].line for i in sel["selected"])
    return refs, [tuple(records[i][:5]) for i in sel["selected"]], unaligned_len, sel["strandness"]


# ---- quantification: the EM over multi-mapping reads (src/get_primary_sam.py:44-142) -----------------------------------------------------------
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
    others, spans = sel["others"], sel["spans"]
    for k, i in enumerate(sel["primaries"]):
        while at < len(others) and others[at] < i:           # the records in front of this primary, in file order (G:397-405)
            o = records[others[at]]
            key = (o.qname, (int(spans["qstart"][at]), int(spans["qend"][at])))
            if key in quant:
                quant[key].append(name_of(o.rname))
            at += 1
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
    while at < len(others):
        o = records[others[at]]
        key = (o.qname, (int(spans["qstart"][at]), int(spans["qend"][at])))
        if key in quant:
            quant[key].append(name_of(o.rname))
        at += 1
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
    total_rpk = 0
    if normalize:
        for n, c in zip(names, counts):
            total_rpk += c / targets[n] * 1e3
    else:
        for c in counts:                                     # (the fold of sum() up to CPython 3.11)
            total_rpk = total_rpk + c
    result = {}
    for n, c in zip(names, counts):
        rpk = c / targets[n] * 1e3 if normalize else c
        result[n] = (c, rpk * 1e6 / total_rpk)
    out["result"] = result
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
    with open(prefix + "_quantification.tsv", "w") as f:
        f.write(format_quantification(kind, res["result"]))
    variation = abundance_variation(res["result"], expected) if kind == "meta" and expected is not None else None
    return res["result"], variation


# ---- the intron-retention model (src/model_intron_retention.py:35-219) ---------------------------------------------------------------------
class NsIrIntrons(C.Structure):
    """mirror of ns_ir_introns (include/nanosim_amd.h)"""
    _fields_ = [("n_trx", C.c_uint32), ("n_chrom", C.c_uint32), ("intr_off", C.c_void_p), ("intr_chrom", C.c_void_p), ("intr_start", C.c_void_p),
                ("intr_end", C.c_void_p), ("merged_off", C.c_void_p), ("merged_chrom", C.c_void_p), ("merged_start", C.c_void_p),
                ("merged_end", C.c_void_p)]


class NsIrTrainResult(C.Structure):
    """mirror of ns_ir_train_result (include/nanosim_amd.h)"""
    _fields_ = [("state", C.c_void_p), ("retained", C.c_void_p), ("first", C.c_uint64 * 2), ("states", C.c_uint64 * 4), ("n_bad", C.c_uint64),
                ("first_bad", C.c_uint64), ("ms_kernel", C.c_double)]


IR_NONE = 0xffffffff                                        # NS_IR_NONE
IR_READ_NONE, IR_READ_NO_IR, IR_READ_IR = 0, 1, 2           # NS_IR_READ_*: the state byte of a read

# a read of ir_alignments: its genome alignment (RNAME as it stands, 0-based start, CIGAR) and the transcript of its transcriptome alignment
IrRead = collections.namedtuple("IrRead", "qname chrom start cigar trx")


def _strip_chr(chrom: str) -> str:
    """M:61-62, 117-118 (str.strip: a set of characters)"""
    return chrom.strip("chr") if "chr" in chrom else chrom


def ir_introns(gff_path: str) -> dict:
    """dict_intron_info (M:38-66) with the chromosome kept: {transcript id: [(chrom, start, end), ...]} of the `intron` rows, in file
    order; every row whose id resolves makes an entry, so a transcript without introns has an empty list"""
    from .intron_retention import gff_features
    out: dict = {}
    for fid, ftype, chrom, start, end, _ in gff_features(gff_path):
        rows = out.setdefault(fid, [])
        if ftype == "intron":
            rows.append((chrom, start, end))
    return out


def _mapped_records(path: str):
    """the fields of every record of a SAM text file that is not unmapped, in file order"""
    with open(path) as f:
        for line in f:
            if line.startswith("@"):
                continue
            fld = line.rstrip("\n").split("\t")
            if len(fld) < 6 or int(fld[1]) & 0x4:
                continue
            yield fld


def ir_alignments(g_sam: str, t_sam: str):
    """The two joins of M:70-97 over SAM text: [IrRead] of every read that has a record in both files, in the order in which the
    genome file first names them.  Every record that is not unmapped counts, whatever its other FLAG bits, and a later record of a
    QNAME replaces what an earlier one gave (dict assignment: the value of the last, the place of the first).  The transcript is RNAME,
    cut at the first `.` when it begins with `ENST`."""
    genome, trx = {}, {}
    for fld in _mapped_records(g_sam):
        genome[fld[0]] = (fld[2], int(fld[3]) - 1, fld[5])
    for fld in _mapped_records(t_sam):
        trx[fld[0]] = fld[2].split(".")[0] if fld[2].startswith("ENST") else fld[2]
    return [IrRead(q, g[0], g[1], g[2], trx[q]) for q, g in genome.items() if q in trx]


def ir_tables(introns: dict) -> dict:
    """the tables of ns_ir_train from ir_introns' dict: ids for the transcripts that have an intron and for the chromosomes that carry
    one, the introns in file order, and per transcript their union as merged intervals sorted by (chromosome, start) — overlapping and
    touching introns are one interval, an empty intron (end == start) is in none"""
    trx_id, chrom_id = {}, {}
    intr_off, merged_off = [0], [0]
    ic, is_, ie, mc, ms, me = [], [], [], [], [], []
    for tid, rows in introns.items():
        if not rows:
            continue
        trx_id[tid] = len(trx_id)
        own = []
        for chrom, start, end in rows:
            if start < 0 or end < start or end >= 1 << 32:
                raise ValueError("intron %d-%d of transcript %s is out of range" % (start, end, tid))
            c = chrom_id.setdefault(chrom, len(chrom_id))
            ic.append(c); is_.append(start); ie.append(end)
            if end > start:
                own.append((c, start, end))
        own.sort()
        first = len(mc)
        for c, start, end in own:
            if len(mc) > first and mc[-1] == c and start <= me[-1]:
                me[-1] = max(me[-1], end)
            else:
                mc.append(c); ms.append(start); me.append(end)
        intr_off.append(len(ic)); merged_off.append(len(mc))
    u32 = lambda v: np.array(v, dtype=np.uint32)
    return dict(trx_id=trx_id, chrom_id=chrom_id, intr_off=np.array(intr_off, dtype=np.uint64), intr_chrom=u32(ic), intr_start=u32(is_),
                intr_end=u32(ie), merged_off=np.array(merged_off, dtype=np.uint64), merged_chrom=u32(mc), merged_start=u32(ms), merged_end=u32(me))


def ir_train_call(eng, tables: dict, cigars, start, chrom, trx):
    """ns_ir_train on reads given as CIGAR texts, 0-based starts, chromosome ids and transcript ids (IR_NONE: none):
    (the NsIrTrainResult, the state byte per read, the retained bitmap as a bool per intron); nothing is raised for bad CIGARs"""
    n = len(cigars)
    cg, cg_off = _pack(cigars)
    start, chrom, trx = (np.ascontiguousarray(v, dtype=np.uint32) for v in (start, chrom, trx))
    n_intr = int(tables["intr_off"][-1])
    T = NsIrIntrons()
    T.n_trx, T.n_chrom = len(tables["intr_off"]) - 1, len(tables["chrom_id"])
    for name in ("intr_off", "intr_chrom", "intr_start", "intr_end", "merged_off", "merged_chrom", "merged_start", "merged_end"):
        setattr(T, name, tables[name].ctypes.data if len(tables[name]) else None)
    state = np.zeros(n, dtype=np.uint8)
    words = np.zeros((n_intr + 31) // 32, dtype=np.uint32)
    out = NsIrTrainResult()
    out.state, out.retained = state.ctypes.data if n else None, words.ctypes.data if len(words) else None
    eng._check(eng.L.ns_ir_train(eng.ctx, cg.ctypes.data, cg_off.ctypes.data, start.ctypes.data if n else None, chrom.ctypes.data if n else None,
                                 trx.ctypes.data if n else None, n, C.addressof(T), C.addressof(out)))
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_intr].astype(bool)
    return out, state, bits


def count_intron_retention(eng, introns: dict, reads) -> dict:
    """What the loop of M:104-176 counts for the reads of ir_alignments against the introns of ir_introns, from the GPU (ns_ir_train):
    first = [no_IR, IR], states = [no_IR -> no_IR, no_IR -> IR, IR -> no_IR, IR -> IR], state = a byte per read (IR_READ_*),
    ir_info = {transcript: [(start, end), ...]} — its retained introns, distinct and sorted, transcripts in the order in which the reads
    first name them, those without a retained intron left out —, ms_kernel.  A CIGAR that is not one (`*` among them: pysam gives such
    a record no block) or a start outside 0 .. 2^32 - 1 raises ValueError."""
    tables = ir_tables(introns)
    for r in reads:
        if not 0 <= r.start < 1 << 32:
            raise ValueError("read %s: reference start %d is out of range" % (r.qname, r.start))
    chrom = [tables["chrom_id"].get(_strip_chr(r.chrom), IR_NONE) for r in reads]
    trx = [tables["trx_id"].get(r.trx, IR_NONE) for r in reads]
    out, state, bits = ir_train_call(eng, tables, [r.cigar for r in reads], [r.start for r in reads], chrom, trx)
    if out.n_bad:
        bad = reads[int(out.first_bad)]
        raise ValueError("%d reads have a CIGAR that is not one; the first: read %s, %.60s" % (out.n_bad, bad.qname, bad.cigar))
    ir_info = {}
    off, starts, ends = tables["intr_off"], tables["intr_start"], tables["intr_end"]
    for tid in dict.fromkeys(r.trx for r in reads):
        t = tables["trx_id"].get(tid)
        if t is None:
            continue
        a, b = int(off[t]), int(off[t + 1])
        kept = sorted(set((int(starts[i]), int(ends[i])) for i in range(a, b) if bits[i]))
        if kept:
            ir_info[tid] = kept
    return dict(first=[int(v) for v in out.first], states=[int(v) for v in out.states], state=state, ir_info=ir_info, ms_kernel=float(out.ms_kernel))


def format_ir_markov_model(counts: dict) -> str:
    """<prefix>_IR_markov_model (M:182-205): three rows of rounded ratios, `0.0` twice where a row's counts add up to 0"""
    f, s = counts["first"], counts["states"]
    text = "succedent\tno_IR\tIR\n"
    for name, pair in (("start", (f[0], f[1])), ("no_IR", (s[0], s[1])), ("IR", (s[2], s[3]))):
        total = pair[0] + pair[1]
        if total != 0:
            text += name + "\t" + str(round(pair[0] / float(total), 4)) + "\t" + str(round(pair[1] / float(total), 4)) + "\n"
        else:
            text += name + "\t0.0\t0.0\n"
    return text


def format_ir_info(ir_info: dict) -> str:
    """<prefix>_IR_info (M:208-216)"""
    text = "trx_name\tintron_spos\tintron_epos\n"
    for tid, kept in ir_info.items():
        if kept:
            text += tid + "\t" + ",".join(str(k[0]) for k in kept) + "\t" + ",".join(str(k[1]) for k in kept) + "\n"
    return text


def intron_retention(prefix: str, gff_path: str, g_sam: str, t_sam: str, eng) -> dict:
    """model_ir.intron_retention(prefix, gff, g_alnm, t_alnm): writes <prefix>_IR_markov_model and <prefix>_IR_info; -> the counts"""
    counts = count_intron_retention(eng, ir_introns(gff_path), ir_alignments(g_sam, t_sam))
    with open(prefix + "_IR_markov_model", "w") as f:
        f.write(format_ir_markov_model(counts))
    with open(prefix + "_IR_info", "w") as f:
        f.write(format_ir_info(counts["ir_info"]))
    return counts


def add_introns(annotation_path: str, out_path: str) -> int:
    """<prefix>_added_intron_final.gff3 from a GFF3 annotation, in place of GenomeTools (`gt gff3 -addintrons` and bequeath.lua,
    src/read_analysis.py:208-232): every line is kept where it is, except that the `exon` rows of a transcript stand together where its
    first one stood, sorted by start, with an `intron` row between two consecutive ones that leave a gap (an exon that overlaps or
    touches the exons in front of it leaves none); `intron` rows that such a transcript already has are dropped for the new ones.  The transcript of an exon is its ``transcript_id``, else its ``Parent`` (the first
    of several, `transcript:` cut off); every exon and intron row carries it as ``transcript_id``, which is what both readers of the
    file resolve first.  -> the number of intron rows written"""
    from .intron_retention import parse_gff_attributes
    lines, exons = [], {}                       # lines: text as it stands | ("exons", transcript) where its rows go | ("intron", transcript, text)
    with open(annotation_path) as f:
        for line in f:
            line = line if line.endswith("\n") else line + "\n"
            cols = line.rstrip("\n").split("\t")
            if line.startswith("#") or len(cols) < 9 or cols[2] not in ("exon", "intron"):
                lines.append(line)
                continue
            attr, _ = parse_gff_attributes(cols[8])
            tid = attr.get("transcript_id")
            if tid is None and "Parent" in attr:
                tid = attr["Parent"].split(",")[0]
                tid = tid[len("transcript:"):] if tid.startswith("transcript:") else tid
                cols[8] = cols[8].rstrip(";") + ";transcript_id=" + tid
            if tid is None:
                lines.append(line)
            elif cols[2] == "intron":
                lines.append(("intron", tid, line))
            else:
                if tid not in exons:
                    exons[tid] = []
                    lines.append(("exons", tid))
                exons[tid].append((int(cols[3]), int(cols[4]), len(exons[tid]), cols, attr.get("Parent")))
    n_introns = 0
    with open(out_path, "w") as f:
        for line in lines:
            if isinstance(line, str):
                f.write(line)
                continue
            if line[0] == "intron":
                if line[1] not in exons:        # (the intron rows of a transcript with exon rows are written anew)
                    f.write(line[2])
                continue
            tid = line[1]
            reach = None
            for start, end, _, cols, parent in sorted(exons[tid]):
                if reach is not None and start > reach + 1:
                    attrs = ("Parent=" + parent + ";" if parent else "") + "transcript_id=" + tid
                    f.write("\t".join([cols[0], cols[1], "intron", str(reach + 1), str(start - 1), ".", cols[6], ".", attrs]) + "\n")
                    n_introns += 1
                reach = end if reach is None else max(reach, end)
                f.write("\t".join(cols) + "\n")
    return n_introns


# ---- MAF input: the best hit per read (src/get_besthit_maf.py:8-56) -----------------------------------------------------------------------
class NsMafBestResult(C.Structure):
    """mirror of ns_maf_best_result (include/nanosim_amd.h)"""
    _fields_ = [("found", C.c_void_p), ("lines", C.c_void_p), ("records", C.c_void_p), ("figures", C.c_void_p), ("n_lines", C.c_uint64),
                ("n_pairs", C.c_uint64), ("n_kept", C.c_uint64), ("pos_strand", C.c_uint64), ("first_bad_line", C.c_uint64),
                ("first_bad_offset", C.c_uint64), ("ms_kernel", C.c_double)]


MAF_LINES_DTYPE = np.dtype([("ref_begin", "<u8"), ("ref_end", "<u8"), ("qry_begin", "<u8"), ("qry_end", "<u8")])                # ns_maf_best_lines
MAF_RECORD_DTYPE = np.dtype([("ref_name_at", "<u8"), ("ref_seq_at", "<u8"), ("qry_seq_at", "<u8"), ("ref_name_len", "<u4"), ("ref_seq_len", "<u4"),
                             ("qry_seq_len", "<u4"), ("ref_start", "<u4")])                                                   # ns_maf_best_record
MAF_FIGURES_DTYPE = np.dtype([("aligned_ref", "<u4"), ("ref_total", "<u4"), ("head", "<u4"), ("total", "<u4"), ("ht", "<i8")])  # ns_maf_best_figures


def _file_bytes(path: str) -> np.ndarray:
    """the bytes of a file as a uint8 array (mapped, not read; `.gz` as file_handler.gzopen: unpacked)"""
    if path.lower().endswith(".gz"):
        import gzip
        with gzip.open(path, "rb") as f:
            return np.frombuffer(f.read(), dtype=np.uint8)
    if os.path.getsize(path) == 0:
        return np.zeros(0, dtype=np.uint8)
    return np.memmap(path, dtype=np.uint8, mode="r")


def _line_number(text: np.ndarray, offset: int) -> int:
    """the 1-based line of the file in which byte `offset` stands"""
    return int(np.count_nonzero(text[:offset] == 10)) + 1


def _last_s_line(text: np.ndarray) -> int:
    """the offset of the last `s` line of the text (-1: none), looked for from the end in pieces"""
    n, step = len(text), 1 << 20
    hi = n
    while hi > 0:
        lo = max(0, hi - step)
        buf = text[lo:min(n, hi + 2)].tobytes()                    # (two bytes more: a start whose '\n' is the piece's last byte)
        at = max(buf.rfind(b"\ns "), buf.rfind(b"\ns\t"))
        if at >= 0:
            return lo + at + 1
        hi = lo
    return 0 if n >= 2 and text[:2].tobytes() in (b"s ", b"s\t") else -1


def besthit_call(eng, text, names=None) -> dict:
    """ns_maf_besthit on the bytes of a MAF file (a uint8 array) and, optionally, the names of a reads file (a list of bytes): the
    NsMafBestResult as `raw`, `lines` / `records` / `figure_rows` (copies of the per-kept-pair arrays, MAF_*_DTYPE) and `found` (a bool
    per name, None without names).  Raises nothing for a bad line (raw.first_bad_line < raw.n_lines) or an odd number of `s` lines
    (raw.n_lines & 1): the caller knows the file."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    out = NsMafBestResult()
    n_names = 0 if names is None else len(names)
    nm = nm_off = found = None
    if names is not None:
        found = np.zeros(n_names, dtype=np.uint8)
    if n_names:
        nm, nm_off = _pack(names)
        out.found = found.ctypes.data
    rc = eng.L.ns_maf_besthit(eng.ctx, text.ctypes.data if len(text) else None, len(text), nm.ctypes.data if n_names else None,
                              nm_off.ctypes.data if n_names else None, n_names, C.addressof(out))
    if not (int(out.n_lines) & 1):
        eng._check(rc)
    k = int(out.n_kept)

    def rows(ptr, dtype):
        if not k:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer(C.string_at(ptr, k * dtype.itemsize), dtype=dtype).copy()       # (the library's arrays live until its next call)
    return dict(raw=out, lines=rows(out.lines, MAF_LINES_DTYPE), records=rows(out.records, MAF_RECORD_DTYPE),
                figure_rows=rows(out.figures, MAF_FIGURES_DTYPE), found=None if names is None else found.astype(bool))


def figures_from_rows(rows, mode: str = "genome") -> dict:
    """length_figures_maf's dict from the figure rows of besthit_call (A:91-110)"""
    if mode not in LEN_MODES:
        raise ValueError("mode must be 'genome' or 'transcriptome'")
    head, ht = rows["head"].astype(np.int64), rows["ht"].astype(np.int64)
    take = ht != 0
    out = dict(aligned_ref_length=rows["aligned_ref"].astype(np.int64), total_length=rows["total"].astype(np.int64), ht_length=ht, head=head, tail=ht - head,
               head_vs_ht_ratio=head[take].astype(np.float64) / ht[take].astype(np.float64), ms_kernel=0.0)
    if mode == "transcriptome":
        out["total_ref_length"] = rows["ref_total"].astype(np.int64)
    return out


def fasta_lines(path: str):
    """the reads file as G:43-52 walks it, FASTA (possibly `.gz`): (names: the first word of every `>` header without the `>`, as bytes;
    owner: per sequence line the index of its header; length: len(line.strip()) of it — a blank line is a 0).  ValueError for a header
    without a name and a sequence line in front of the first header."""
    import gzip
    names, owner, length = [], [], []
    with (gzip.open(path, "rb") if path.lower().endswith(".gz") else open(path, "rb")) as f:
        for no, line in enumerate(f, 1):
            if line[:1] == b">":
                word = line.strip().split()[0][1:]
                if not word:
                    raise ValueError("%s:%d: a `>` header without a name" % (path, no))
                names.append(word)
            elif not names:
                raise ValueError("%s:%d: a sequence line in front of the first header (the reference stops with a NameError)" % (path, no))
            else:
                owner.append(len(names) - 1)
                length.append(len(line.strip()))
    return names, np.array(owner, dtype=np.int64), np.array(length, dtype=np.int64)


def besthit(eng, maf_path: str, reads_path=None, mode: str = "genome") -> dict:
    """besthit_and_unaligned (G:8-56) without its file: of the pairs of `s` lines of every query name of a LAST MAF file — as it is, or
    what `grep '^s '` left of it — the one with the largest size, of several the first, chosen on the GPU from the file's bytes
    (ns_maf_besthit).  -> `lines` (MAF_LINES_DTYPE: the byte ranges of the two lines of every kept pair, in file order), `num_aligned`,
    `pos_strand`, `strandness` (float(pos_strand) / num_aligned, G:41), `figures` (length_figures_maf's dict for the kept pairs; `mode`
    as there), `figure_rows`, `records` (maf_records' list for them), `unaligned_length` (int64: len(line.strip()) of every sequence line
    of every read of `reads_path` whose name is no query name, G:43-52; None without a reads file) and `ms_kernel`.
    The reads file is FASTA (`.gz` too, as file_handler.gzopen); the reference reads FASTQ with the same loop and counts its `+` and
    quality lines as sequence: not restated, give FASTA.
    ValueError with the file and the line: an odd number of `s` lines, a line whose start, size or srcSize is not made of digits that fit
    32 bits or that has fewer than 7 fields, a reference sequence longer than the query's (maf_records), a file without any alignment
    (the reference divides by zero), and fasta_lines' two."""
    names = owner = length = None
    if reads_path is not None:
        names, owner, length = fasta_lines(reads_path)
    text = _file_bytes(maf_path)
    r = besthit_call(eng, text, names)
    raw = r["raw"]
    if int(raw.n_lines) & 1:
        raise ValueError("%s:%d: an `s` line without its partner (odd number of `s` lines)" % (maf_path, _line_number(text, max(_last_s_line(text), 0))))
    if raw.first_bad_line < raw.n_lines:
        raise ValueError("%s:%d: not an `s` line of LAST: start, size and srcSize have to be decimal digits below 2^32, in 7 fields or more"
                         % (maf_path, _line_number(text, int(raw.first_bad_offset))))
    if not raw.n_kept:
        raise ValueError("%s: no alignment at all (the reference divides by zero, G:41)" % maf_path)
    recs = []
    for rec in r["records"].tolist():
        name_at, rs, qs, name_len, rl, ql, start = rec
        if rl > ql:
            raise ValueError("%s:%d: not two `s` lines with an aligned sequence each (the reference sequence is the longer one)"
                             % (maf_path, _line_number(text, rs)))
        recs.append((text[name_at:name_at + name_len].tobytes().decode(), start, text[rs:rs + rl].tobytes().decode(), text[qs:qs + rl].tobytes().decode()))
    num_aligned, pos_strand = int(raw.n_kept), int(raw.pos_strand)
    return dict(lines=r["lines"], num_aligned=num_aligned, pos_strand=pos_strand, strandness=float(pos_strand) / num_aligned,
                figures=figures_from_rows(r["figure_rows"], mode), figure_rows=r["figure_rows"], records=recs,
                unaligned_length=None if names is None else length[~r["found"][owner]],
                ms_kernel=float(raw.ms_kernel))


def write_besthit(prefix: str, maf_path: str, result: dict) -> None:
    """<prefix>_besthit.maf as G:35 writes it: the two lines of every kept pair as they stand in the file, in file order (a last line
    without '\\n' stays without)"""
    text = _file_bytes(maf_path)
    with open(prefix + "_besthit.maf", "wb") as f:
        for rb, re_, qb, qe in result["lines"].tolist():
            f.write(text[rb:re_].tobytes())
            f.write(text[qb:qe].tobytes())


def besthit_and_unaligned(prefix: str, maf_path: str, reads_path: str, eng):
    """besthit_and_unaligned(infile, outmaf, prefix) of G:8: writes <prefix>_besthit.maf, -> (unaligned_length, strandness)"""
    r = besthit(eng, maf_path, reads_path)
    write_besthit(prefix, maf_path, r)
    return r["unaligned_length"], r["strandness"]


def read_lengths_from_maf(prefix: str, figures: dict, unaligned_len, strandness: float, pickles=None, merge: bool = False) -> dict:
    """read_lengths for length figures that are there already (besthit's, or length_figures_maf's): the KDE files, <prefix>_strandness_rate
    and <prefix>_reads_alignment_rate; returns the figures"""
    write_kde(prefix, kde_models(figures, unaligned_len), pickles, merge)
    with open(prefix + "_strandness_rate", "w") as f:
        f.write(format_strandness(strandness))
    with open(prefix + "_reads_alignment_rate", "w") as f:
        f.write(format_alignment_rate(len(figures["total_length"]), 0 if unaligned_len is None else len(unaligned_len)))
    return figures


def train_genome_from_maf(prefix: str, maf_path: str, reads_path: str, eng, model_fit: bool = True, homopolymer: bool = False, min_hp_len: int = 5,
                          pickles=None) -> dict:
    """what `read_analysis.py genome -ga x.maf` runs behind the alignment (R:185-190, 605-611, 858-875): the best hit per read and
    <prefix>_besthit.maf, hist(prefix, "maf") from the kept pairs as they came from the GPU (the file is not read back), the read-length
    files, model_fitting unless model_fit is False (--no_model_fit) and, with `homopolymer`, the homopolymer-length model.  The prefix
    then opens with model.load_model(prefix) (with model_fit=False it needs a <prefix>_model_profile from elsewhere).  -> besthit's dict"""
    r = besthit(eng, maf_path, reads_path)
    write_besthit(prefix, maf_path, r)
    hist(prefix, [(ref, qry) for _, _, ref, qry in r["records"]], eng, "maf")
    read_lengths_from_maf(prefix, r["figures"], r["unaligned_length"], r["strandness"], pickles)
    if model_fit:
        model_fitting(prefix, eng)
    if homopolymer:
        homopolymer_lengths(prefix, r["records"], eng, min_hp_len)
    return r
