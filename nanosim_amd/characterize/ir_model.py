"""The intron-retention model (``intron_retention`` of src/model_intron_retention.py, M:35-219) is the ninth piece, and the last file of
a transcriptome prefix: ``<prefix>_IR_markov_model`` with ``<prefix>_IR_info``.  The reference walks the aligned blocks of every read
that has a genome and a transcriptome alignment through HTSeq's interval array; here the walk over a read's CIGAR and the introns of
its transcript, the six Markov counts and the retained introns come from the GPU (``ns_ir_train``; csrc/ns_ir_train.h names every
corner of the reference that is kept), and this module reads the annotation and the two SAM files and writes the files:

    characterize.add_introns("annotation.gff3", "training_added_intron_final.gff3")       # in place of GenomeTools
    characterize.intron_retention("training", "training_added_intron_final.gff3", "genome.sam", "transcriptome.sam", eng)

Deviations: SAM text instead of BAM; a CIGAR that is not one (`*` among them) and a start beyond 32 bits raise ValueError;
``add_introns`` is not pinned against GenomeTools' output."""
import collections
import ctypes as C

import numpy as np

from ..intron_retention import gff_features, parse_gff_attributes
from ._abi import _pack, arr, ptr, write_text
from .sam_table import SamTable
from .sam_text import sam_lines


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
    out: dict = {}
    for fid, ftype, chrom, start, end, _ in gff_features(gff_path):
        rows = out.setdefault(fid, [])
        if ftype == "intron":
            rows.append((chrom, start, end))
    return out


def _mapped_records(path: str):
    """the fields of every record of a SAM text file that is not unmapped, in file order"""
    if isinstance(path, SamTable):
        return iter(path.mapped_records())
    return sam_lines(path, 6, drop=0x4)


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
    start, chrom, trx = (arr(v, np.uint32) for v in (start, chrom, trx))
    n_intr = int(tables["intr_off"][-1])
    T = NsIrIntrons()
    T.n_trx, T.n_chrom = len(tables["intr_off"]) - 1, len(tables["chrom_id"])
    for name in ("intr_off", "intr_chrom", "intr_start", "intr_end", "merged_off", "merged_chrom", "merged_start", "merged_end"):
        setattr(T, name, ptr(tables[name]))
    state = np.zeros(n, dtype=np.uint8)
    words = np.zeros((n_intr + 31) // 32, dtype=np.uint32)
    out = NsIrTrainResult()
    out.state, out.retained = ptr(state), ptr(words)
    eng._check(eng.L.ns_ir_train(eng.ctx, cg.ctypes.data, cg_off.ctypes.data, ptr(start), ptr(chrom), ptr(trx), n, C.addressof(T), C.addressof(out)))
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
    write_text(prefix + "_IR_markov_model", format_ir_markov_model(counts))
    write_text(prefix + "_IR_info", format_ir_info(counts["ir_info"]))
    return counts


def add_introns(annotation_path: str, out_path: str) -> int:
    """<prefix>_added_intron_final.gff3 from a GFF3 annotation, in place of GenomeTools (`gt gff3 -addintrons` and bequeath.lua,
    src/read_analysis.py:208-232): every line is kept where it is, except that the `exon` rows of a transcript stand together where its
    first one stood, sorted by start, with an `intron` row between two consecutive ones that leave a gap (an exon that overlaps or
    touches the exons in front of it leaves none); `intron` rows that such a transcript already has are dropped for the new ones.  The transcript of an exon is its ``transcript_id``, else its ``Parent`` (the first
    of several, `transcript:` cut off); every exon and intron row carries it as ``transcript_id``, which is what both readers of the
    file resolve first.  -> the number of intron rows written"""
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
