"""cs and MD tags from the reference genome.  Every stage here needs a ``cs:Z`` or an ``MD:Z`` tag on its alignments (cs_of, sam_records),
as the reference does (``alnm.get_tag('MD')``, src/besthit_to_histogram.py:320-324: it assumes its own ``minimap2 --cs`` run).  The files
people have — what a basecaller or an earlier ``minimap2 -a`` wrote — carry CIGAR and SEQ and neither tag, often with ``=`` / ``X`` ops.
Both tags are a function of CIGAR, POS, SEQ and the reference genome; ``ns_calmd`` (csrc/ns_calmd.h, which states the rules of the text:
samtools calmd's MD, minimap2's short-form cs) computes them on the GPU against the engine's copy of the reference:

    tagged = characterize.with_reference(characterize.read_bam("calls.bam", eng), "genome.fa", eng)    # or a SAM path
    characterize.hist("training", characterize.cs_from_sam(tagged), eng)       # wherever a reader takes the path of a SAM file
    characterize.calmd("calls.sam", "genome.fa", "tagged.sam", eng)            # the text as a file

with_reference SETS THE REFERENCE OF THE ENGINE (eng.set_reference): what the engine simulated from before is replaced, and an engine
whose reference is set to something else between two iterations of the result has to be given back (`tagged.set_reference()`)."""
import ctypes as C

import numpy as np

from ..model import Reference, read_fasta
from ._abi import _pack, arr, ptr
from .sam_text import SamSource, _open_sam, _sam_refs

BATCH_BYTES = 64 << 20
CALMD_BAD_REASONS = {1: "the CIGAR does not parse", 2: "a CIGAR op outside MIDSH=X", 3: "a clip that is not outermost (S inside the H ops only)",
                     4: "the length of SEQ is not the sum of its S/M/=/X/I ops", 5: "a SEQ byte that is not a letter",
                     6: "a reference index outside the set reference", 7: "POS is 0", 8: "the alignment runs past the end of its chromosome",
                     9: "no M, = or X column at all"}


class NsCalmdResult(C.Structure):
    """mirror of ns_calmd_result (include/nanosim_amd.h)"""
    _fields_ = [("md", C.c_void_p), ("md_off", C.c_void_p), ("cs", C.c_void_p), ("cs_off", C.c_void_p), ("n_bad", C.c_uint64), ("first_bad", C.c_uint64),
                ("bad_reason", C.c_uint32), ("reserved", C.c_uint32), ("ms_kernel", C.c_double)]


def calmd_raw(eng, cigars, seqs, chrom, pos) -> dict:
    """ns_calmd as it answers: md / cs (bytes, the texts one behind the other), md_off / cs_off (uint64, len + 1), n_bad, first_bad,
    bad_reason, ms_kernel.  cigars, seqs: str or bytes each; chrom: indices into the reference set on the engine; pos: 1-based."""
    n = len(cigars)
    cg, cg_off = _pack(cigars)
    sq, sq_off = _pack(seqs)
    ch, ps = arr(chrom, np.uint32), arr(pos, np.uint32)
    if len(sq_off) != n + 1 or len(ch) != n or len(ps) != n:
        raise ValueError("cigars, seqs, chrom and pos differ in length")
    out = NsCalmdResult()
    eng._check(eng.L.ns_calmd(eng.ctx, cg.ctypes.data, cg_off.ctypes.data, sq.ctypes.data, sq_off.ctypes.data, ptr(ch), ptr(ps), n, C.addressof(out)))
    md_off = np.frombuffer(C.string_at(out.md_off, 8 * (n + 1)), dtype=np.uint64)             # (copies: the library's arrays live until its next call)
    cs_off = np.frombuffer(C.string_at(out.cs_off, 8 * (n + 1)), dtype=np.uint64)
    return dict(md=C.string_at(out.md, int(md_off[-1])), md_off=md_off, cs=C.string_at(out.cs, int(cs_off[-1])), cs_off=cs_off, n_bad=int(out.n_bad),
                first_bad=int(out.first_bad), bad_reason=int(out.bad_reason), ms_kernel=float(out.ms_kernel))


def cs_md_call(eng, cigars, seqs, chrom, pos) -> dict:
    """the MD and short-form cs text of these alignments against the reference set on the engine: md, md_off, cs, cs_off, ms_kernel as
    calmd_raw gives them.  ValueError that names the first bad record and why it is bad."""
    r = calmd_raw(eng, cigars, seqs, chrom, pos)
    if r["n_bad"]:
        i = r["first_bad"]
        cigar = cigars[i].decode() if isinstance(cigars[i], bytes) else cigars[i]
        raise ValueError("%d record(s) from which no MD / cs text can be made; the first is record %d (CIGAR %.60s, %d bases, reference %d, POS %d): %s"
                         % (r["n_bad"], i, cigar, len(seqs[i]), int(chrom[i]), int(pos[i]),
                            CALMD_BAD_REASONS.get(r["bad_reason"], "reason %d" % r["bad_reason"])))
    return r


def texts_of(r: dict, which: str):
    """the n texts of a cs_md_call result as str: which = "md" or "cs" """
    text, off = r[which].decode(), r[which + "_off"].tolist()
    return [text[a:b] for a, b in zip(off, off[1:])]


class TaggedText(SamSource):
    """The SAM text of `source` with MD:Z and cs:Z on every mapped record: iterating gives the header lines and then the records, each with
    its '\\n'.  A mapped record with SEQ that lacks MD:Z gets `\\tMD:Z:...` appended, one that lacks cs:Z `\\tcs:Z:...` behind it; a tag that
    is there stays as it stands, and so does every other byte of every line.  Unmapped records (FLAG 4, RNAME `*`, CIGAR `*`), records
    with SEQ `*` and lines of fewer than 11 fields pass through untouched.  Every iteration computes again (nothing is kept), about
    batch_bytes of SEQ per call of the library.  ValueError: an RNAME the FASTA does not hold, an @SQ line whose LN is not the FASTA's
    length of that name (the wrong reference), a record no text can be made from (with the record's name and the reason).
    `ms_kernel`, `n_records`, `n_tagged`: of the last iteration."""

    def __init__(self, source, reference, eng, batch_bytes: int = BATCH_BYTES):
        self.source, self.eng, self.batch_bytes = source, eng, int(batch_bytes)
        self.ref = reference if isinstance(reference, Reference) else read_fasta(str(reference), "linear", raw_names=True)
        self.index = {name: i for i, name in enumerate(self.ref.names)}
        self.lengths = np.diff(self.ref.chrom_off.astype(np.int64)).tolist()
        self.ms_kernel, self.n_records, self.n_tagged = 0.0, 0, 0
        self.set_reference()

    def __str__(self):
        return str(self.source)

    def set_reference(self):
        """this text's reference as the engine's"""
        self.eng.set_reference(self.ref)
        self.eng._calmd_reference = self.ref

    def _check_sq(self, line):
        refs = []
        _sam_refs(line.rstrip("\n").split("\t"), refs)
        for name, length in refs:
            if name in self.index and self.lengths[self.index[name]] != length:
                raise ValueError("%s: @SQ SN:%s has LN:%d, the reference has %d bases of that name: not the reference these reads were aligned to"
                                 % (self, name, length, self.lengths[self.index[name]]))

    def _flush(self, batch):
        """the lines of a batch: [(line, fields or None, lacks MD, lacks cs)]"""
        work = [b for b in batch if b[1] is not None]
        if work:
            chrom = []
            for _, fld, _, _ in work:
                if fld[2] not in self.index:
                    raise ValueError("%s: alignment %s lies on %s, which the reference does not hold" % (self, fld[0], fld[2]))
                chrom.append(self.index[fld[2]])
            pos = [int(fld[3]) if 0 <= int(fld[3]) < 2 ** 32 else 0 for _, fld, _, _ in work]
            r = calmd_raw(self.eng, [fld[5] for _, fld, _, _ in work], [fld[9] for _, fld, _, _ in work], chrom, pos)
            if r["n_bad"]:
                fld = work[r["first_bad"]][1]
                raise ValueError("%s: %d record(s) from which no MD / cs text can be made; the first is alignment %s (CIGAR %.60s, %d bases, %s:%s): %s"
                                 % (self, r["n_bad"], fld[0], fld[5], len(fld[9]), fld[2], fld[3],
                                    CALMD_BAD_REASONS.get(r["bad_reason"], "reason %d" % r["bad_reason"])))
            self.ms_kernel += r["ms_kernel"]
            md, cs = texts_of(r, "md"), texts_of(r, "cs")
        k = 0
        for line, fld, no_md, no_cs in batch:
            self.n_records += 1
            if fld is None:
                yield line
                continue
            end = "\n" if line.endswith("\n") else ""
            yield (line[:len(line) - len(end)] + ("\tMD:Z:" + md[k] if no_md else "") + ("\tcs:Z:" + cs[k] if no_cs else "") + end)
            self.n_tagged += 1
            k += 1

    def _lines(self):
        if isinstance(self.source, SamSource):
            yield from self.source
            return
        with _open_sam(self.source) as f:
            yield from f

    def __iter__(self):
        if getattr(self.eng, "_calmd_reference", None) is not self.ref:
            self.set_reference()
        self.ms_kernel, self.n_records, self.n_tagged = 0.0, 0, 0
        batch, held = [], 0
        for line in self._lines():
            if line[0] == "@":
                if batch:
                    yield from self._flush(batch)
                    batch, held = [], 0
                if line.startswith("@SQ\t"):
                    self._check_sq(line)
                yield line
                continue
            fld = line.rstrip("\n").split("\t")
            no_md = no_cs = False
            if len(fld) >= 11 and fld[2] != "*" and fld[5] != "*" and fld[9] != "*" and not int(fld[1]) & 4:
                no_md = not any(t.startswith("MD:Z:") for t in fld[11:])
                no_cs = not any(t.startswith("cs:Z:") for t in fld[11:])
            if not (no_md or no_cs):
                if batch:
                    batch.append((line, None, False, False))
                else:
                    self.n_records += 1
                    yield line
                continue
            batch.append((line, fld, no_md, no_cs))
            held += len(fld[9])
            if held >= self.batch_bytes:
                yield from self._flush(batch)
                batch, held = [], 0
        if batch:
            yield from self._flush(batch)


def with_reference(source, reference, eng, batch_bytes: int = BATCH_BYTES) -> TaggedText:
    """`source` — the path of a SAM text file or a SamSource (read_bam's BamText) — with MD:Z and cs:Z computed from `reference` (the path
    of a FASTA file, read with model.read_fasta(..., raw_names=True), or a model.Reference whose names are the RNAMEs) on the GPU, for
    sam_lines and every reader over it.  It sets the reference on `eng`: THIS REPLACES THE ENGINE'S REFERENCE."""
    return TaggedText(source, reference, eng, batch_bytes)


def calmd(source, reference, out_path: str, eng):
    """writes the SAM text of with_reference(source, reference, eng); -> (the number of records, how many of them got a tag)"""
    tagged = with_reference(source, reference, eng)
    with open(out_path, "w") as f:
        for line in tagged:
            f.write(line)
    return tagged.n_records, tagged.n_tagged
