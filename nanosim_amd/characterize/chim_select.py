"""What chimeric() (chimeric_reads, whose docstring describes the stage) and quantify() (quantification) both start from: the records
of a SAM file with their NM and SA tags and the split-alignment choice over them (``ns_chimeric_select``, ``ns_cigar_spans``)."""
import collections
import ctypes as C

import numpy as np

from ._abi import _pack, arr, check_bad, ptr
from .sam_table import SamTable
from .sam_text import no_sq_line, sam_lines


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
    if isinstance(path, SamTable):
        return path.chimeric_records()
    refs, records, unaligned, header = [], [], [], []
    seen_primary = False
    for line, fld in sam_lines(path, 11, refs, header, lines=True):
        flag = int(fld[1])
        seq_len = 0 if fld[9] == "*" else len(fld[9])
        if flag & 0x4:
            unaligned.append(seq_len)
            continue
        nm = sa = None
        for t in fld[11:]:                                   # (written out, not two sam_tag calls: this reader looks at every record's tags)
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
            raise no_sq_line(r.qname, r.rname)
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
    eng._check(eng.L.ns_cigar_spans(eng.ctx, cg.ctypes.data, cg_off.ctypes.data, n, ptr(out), C.addressof(n_bad),
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
    ref_total, species = arr(ref_total, np.uint64), arr(species, np.uint32)
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
    ref_index = {name: i for i, (name, _) in reversed(list(enumerate(refs)))}            # (of equal names the first)
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

    def bad_entry(bad):
        r = int(np.searchsorted(ent_off, bad, side="right")) - 1
        return "entry %d of read %s: %.60s" % (bad - int(ent_off[r]), records[primaries[r]].qname, reads[r][bad - int(ent_off[r])][0])
    check_bad(out.n_bad, out.first_bad, "CIGAR(s) that are not one among the primary alignments and their SA entries", bad_entry)
    spans, n_bad, first_bad, ms_spans = cigar_spans(eng, [records[i].cigar for i in others])
    check_bad(n_bad, first_bad, "supplementary / secondary record(s) whose CIGAR is not one",
              lambda i: "a record of read %s: %.60s" % (records[others[i]].qname, records[others[i]].cigar))
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
