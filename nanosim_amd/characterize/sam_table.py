"""The index of a SAM text is the thirteenth piece: ``ns_sam_index`` (csrc/ns_sam_index.h) finds the lines, the fields and the tags
cs:Z: MD:Z: NM:i: SA:Z: of SAM text on the GPU from the bytes of the file, and a ``SamTable`` keeps the rows it leaves — offsets, FLAG,
POS, NM — next to the bytes.  Every reader of the stages takes a table in the place of a path and returns what it returns for the path,
without splitting a line again; a run over one alignment file builds its table once:

    table = characterize.SamTable("training.sam", eng)          # or SamTable(characterize.read_bam("training.bam", eng), eng)
    refs, recs, unaligned_len, strandness = characterize.primary_and_unaligned(table)
    primary = table.primary()                                   # a view: the rows without FLAG 0x4 / 0x100 / 0x800, the same bytes
    characterize.hist("training", characterize.cs_from_sam(primary), eng)
    primary.write_sam("training_primary.sam")

The strings a reader returns are slices of the text at the row's offsets.  A number the index does not call plain (anything but 1-10
decimal digits below 2^32) is handed to int() as its field text, for a row on which the path reader would have called int() on that
field: int() raises or accepts exactly where the path reader does.
Deviations: SAM text with a '\\r' or a byte >= 0x80 raises ValueError — text mode's universal newlines and UTF-8 are not restated; such
a file goes through the path readers.  chimeric_records converts the NM:i: field that counts, the last one (the path reader converts
every NM:i: field of a record on its way to the last)."""
import ctypes as C
import os
import re

import numpy as np

from ._abi import arr, ptr
from .sam_text import SamSource, _open_sam, _sam_refs, get_cs, no_sq_line


class NsSamIndexResult(C.Structure):
    """mirror of ns_sam_index_result (include/nanosim_amd.h)"""
    _fields_ = [("rows", C.c_void_p), ("header", C.c_void_p), ("n_records", C.c_uint64), ("n_header", C.c_uint64), ("n_odd", C.c_uint64),
                ("n_cs", C.c_uint64), ("n_md", C.c_uint64), ("ms_kernel", C.c_double)]


SAM_ROW_DTYPE = np.dtype([("begin", "<u8"), ("end", "<u8"), ("n_fields", "<u4"), ("bits", "<u4"), ("field_end", "<u4", (11,)), ("flag", "<u4"),
                          ("pos", "<u4"), ("nm", "<u4"), ("tag_at", "<u4", (4,)), ("tag_len", "<u4", (4,))])                  # ns_sam_row
SAM_SPAN_DTYPE = np.dtype([("begin", "<u8"), ("end", "<u8")])                                                                # ns_sam_span
SAM_FLAG_ODD, SAM_POS_ODD, SAM_NM_ODD = 1, 2, 4              # NS_SAM_*: ns_sam_row.bits
SAM_HAS_CS, SAM_HAS_MD, SAM_HAS_NM, SAM_HAS_SA = 16, 32, 64, 128
SAM_TAG_CS, SAM_TAG_MD, SAM_TAG_NM, SAM_TAG_SA = 0, 1, 2, 3  # the index of a tag in tag_at / tag_len
SAM_BATCH_BYTES = 1 << 28

_CLIP_HEAD = re.compile(r'^(?:\d+H)?(\d+)S')                 # (qualities.quals_from_sam's)
_CLIP_TAIL = re.compile(r'(\d+)S(?:\d+H)?$')


def sam_index_call(eng, text) -> dict:
    """ns_sam_index on SAM text (a uint8 array that begins at a line start): `rows` (SAM_ROW_DTYPE) and `header` (SAM_SPAN_DTYPE), copies
    of the call's arrays with offsets into `text`, and the NsSamIndexResult as `raw`"""
    text = arr(text, np.uint8)
    out = NsSamIndexResult()
    eng._check(eng.L.ns_sam_index(eng.ctx, ptr(text), len(text), C.addressof(out)))

    def rows(address, n, dtype):
        if not n:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer(C.string_at(address, n * dtype.itemsize), dtype=dtype).copy()          # (the library's arrays live until its next call)
    return dict(raw=out, rows=rows(out.rows, int(out.n_records), SAM_ROW_DTYPE), header=rows(out.header, int(out.n_header), SAM_SPAN_DTYPE))


def _cut(text, lo: int, want: int) -> int:
    """where the batch that begins at `lo` ends: behind the last '\\n' of its `want` bytes, behind the first one after them when they
    hold none (a line longer than the batch), at the end of the text at the latest"""
    n = len(text)
    if lo + want >= n:
        return n
    step, hi = 1 << 16, lo + want
    while hi > lo:                                          # backwards, in pieces
        a = max(lo, hi - step)
        at = text[a:hi].tobytes().rfind(b"\n")
        if at >= 0:
            return a + at + 1
        hi = a
    hi = lo + want
    while hi < n:                                           # forwards
        at = text[hi:hi + step].tobytes().find(b"\n")
        if at >= 0:
            return hi + at + 1
        hi += step
    return n


class SamTable(SamSource):
    """The rows of ns_sam_index over a whole SAM text and a handle on its bytes.  `source`: the path of a SAM text file, which is mapped,
    or a SamSource (read_bam's BamText, with_reference's TaggedText), whose lines are joined.  The text goes through the call in batches
    of about `batch_bytes`, each cut behind a '\\n'.
    rows / header: SAM_ROW_DTYPE / SAM_SPAN_DTYPE with offsets into the whole text, in file order; n_cs / n_md: the records of the
    text that carry the tag; ms_kernel: the calls' sum.  One method per reader of the stages (length_records, primary_and_unaligned,
    cs_from_sam, quals_from_sam, sam_records, chimeric_records, mapped_records), which the readers call when they are given a table.
    primary() and take() are views: tables over the same bytes and header lines with some of the rows; a reader takes a view as it
    would take the file write_sam writes of it.  Iterating a table gives its lines (a SamSource), those of a view the header lines first."""

    def __init__(self, source, eng, batch_bytes: int = SAM_BATCH_BYTES):
        self._name = str(source)
        self._view = False
        if isinstance(source, SamSource):
            text = np.frombuffer("".join(source).encode(), dtype=np.uint8)
        else:
            _open_sam(source).close()                       # (its ValueError for the gzip magic)
            text = np.memmap(source, dtype=np.uint8, mode="r") if os.path.getsize(source) else np.zeros(0, dtype=np.uint8)
        rows, header = [], []
        self.n_cs = self.n_md = 0
        self.ms_kernel = 0.0
        lo, batch_bytes = 0, max(1, int(batch_bytes))
        while lo < len(text):
            hi = _cut(text, lo, batch_bytes)
            r = sam_index_call(eng, text[lo:hi])
            if r["raw"].n_odd:
                batch = np.asarray(text[lo:hi])
                at = lo + int(np.flatnonzero((batch == 13) | (batch >= 128))[0])
                raise ValueError("%s:%d: a '\\r' or a byte that is not ASCII: a SamTable takes plain SAM text with '\\n' line ends; the readers "
                                 "take the path of such a file themselves" % (self._name, int(np.count_nonzero(np.asarray(text[:at]) == 10)) + 1))
            for a in (r["rows"], r["header"]):
                a["begin"] += lo
                a["end"] += lo
            rows.append(r["rows"])
            header.append(r["header"])
            self.n_cs += int(r["raw"].n_cs)
            self.n_md += int(r["raw"].n_md)
            self.ms_kernel += float(r["raw"].ms_kernel)
            lo = hi
        self.rows = np.concatenate(rows) if rows else np.zeros(0, dtype=SAM_ROW_DTYPE)
        self.header = np.concatenate(header) if header else np.zeros(0, dtype=SAM_SPAN_DTYPE)
        self._set_text(text)

    def _set_text(self, text):
        self._text = text
        self._bytes = memoryview(text) if len(text) else memoryview(b"")

    def __str__(self):
        return self._name

    def __len__(self):
        return len(self.rows)

    # ---- views, lines ----
    def take(self, indices) -> "SamTable":
        """a view of the rows `indices` (of this table's rows), in the order given"""
        t = SamTable.__new__(SamTable)
        t._name, t._view, t.header, t.n_cs, t.n_md, t.ms_kernel = self._name, True, self.header, self.n_cs, self.n_md, self.ms_kernel
        t.rows = self.rows[np.asarray(indices, dtype=np.int64)]
        t._set_text(self._text)
        return t

    def primary(self) -> "SamTable":
        """a view of the primary records: FLAG without 0x4, 0x100 and 0x800 (a FLAG that is not plain is taken as int() takes it)"""
        sel = np.arange(len(self.rows))
        flags, plain = self._flags(sel)
        if plain:
            return self.take(np.flatnonzero(flags & 0x904 == 0))
        c = self._Cursor(self, sel)
        return self.take([j for j in range(len(sel)) if not c.flag(j) & 0x904])

    def _span(self, begin: int, end: int) -> str:
        return str(self._bytes[begin:end], "ascii")

    def _line(self, begin: int, end: int) -> str:
        """a line as a file gives it: with its '\\n' where it has one"""
        return self._span(begin, end + 1 if end < len(self._text) else end)

    def header_lines(self):
        """the header lines as they stand, in file order"""
        return [self._line(b, e) for b, e in self.header.tolist()]

    def __iter__(self):
        spans = [(b, e) for b, e in self.header.tolist()] + list(zip(self.rows["begin"].tolist(), self.rows["end"].tolist()))
        if not self._view:
            spans.sort()
        for b, e in spans:
            yield self._line(b, e)

    def write_sam(self, path: str) -> None:
        """the header lines, then the lines of the rows, as they stand (each with a '\\n')"""
        with open(path, "wb") as f:
            for b, e in self.header.tolist() + list(zip(self.rows["begin"].tolist(), self.rows["end"].tolist())):
                f.write(self._bytes[b:e])
                f.write(b"\n")

    # ---- what the readers share ----
    def _stream(self, min_fields: int, refs=None):
        """sam_lines(path, min_fields, refs) over the rows: (the positions in self.rows of the records it gives, in order; the exception
        that ends it behind them, None without: the int() of a bad LN of an @SQ line)"""
        sel = np.flatnonzero(self.rows["n_fields"] >= min_fields)
        err = None
        if refs is not None:
            for b, e in self.header.tolist():
                if self._bytes[b:b + 4] == b"@SQ\t":
                    try:
                        _sam_refs(self._span(b, e).split("\t"), refs)
                    except ValueError as x:
                        sel = sel[:0] if self._view else sel[self.rows["begin"][sel] < b]
                        err = x
                        break
        return sel, err

    def _flags(self, sel):
        """(FLAG of the rows `sel` as an int64 array, whether every one of them is plain: the others are 0 in the array)"""
        return self.rows["flag"][sel].astype(np.int64), not np.any(self.rows["bits"][sel] & SAM_FLAG_ODD)

    def _fields(self, sel):
        """(begin of every field 0 .. 10 of the rows `sel`, their ends), two int64 arrays of 11 columns, offsets into the text"""
        begin = self.rows["begin"][sel].astype(np.int64)[:, None]
        fe = self.rows["field_end"][sel].astype(np.int64)
        fs = np.concatenate([np.zeros((len(sel), 1), dtype=np.int64), fe[:, :10] + 1], axis=1)
        return begin + fs, begin + fe

    def _is_star(self, fs, fe, k: int):
        """per row: field k is `*`"""
        one = fe[:, k] - fs[:, k] == 1
        if not len(self._text):
            return one
        return one & (np.asarray(self._text[np.minimum(fs[:, k], len(self._text) - 1)]) == 42)

    def _tags(self, sel, tag: int):
        """(begin, end) lists of the tag's value per row of `sel`, and a bool list: the row has it"""
        at = self.rows["begin"][sel].astype(np.int64) + self.rows["tag_at"][sel, tag]
        has = (self.rows["bits"][sel] & (SAM_HAS_CS << tag)) != 0
        return at.tolist(), (at + self.rows["tag_len"][sel, tag]).tolist(), has.tolist()

    class _Cursor:
        """the rows `sel` of a table as a reader walks them: f(j, k) field k of row j as text, flag(j) / pos(j) the number, through
        int() of the field's text where it is not plain"""

        def __init__(self, table, sel):
            self.t = table
            fs, fe = table._fields(sel)
            self.fs_a, self.fe_a = fs, fe
            self._cols = {}                                 # k -> (begin of field k per row, its end), as lists, made when a reader first asks
            self._flag = table.rows["flag"][sel].tolist()
            self._pos = table.rows["pos"][sel].tolist()
            self.bits = table.rows["bits"][sel].tolist()

        def col(self, k: int):
            c = self._cols.get(k)
            if c is None:
                c = self._cols[k] = (self.fs_a[:, k].tolist(), self.fe_a[:, k].tolist())
            return c

        def f(self, j: int, k: int) -> str:
            b, e = self.col(k)
            return self.t._span(b[j], e[j])

        def flag(self, j: int) -> int:
            return int(self.f(j, 1)) if self.bits[j] & SAM_FLAG_ODD else self._flag[j]

        def pos(self, j: int) -> int:
            return int(self.f(j, 3)) if self.bits[j] & SAM_POS_ODD else self._pos[j]

        def star(self, k: int):
            return self.t._is_star(self.fs_a, self.fe_a, k).tolist()

    def _cs_of(self, c, j: int, cs, md) -> str:
        """sam_text.cs_of for row j of the cursor: the cs tag, else from CIGAR + MD"""
        if cs[2][j]:
            return self._span(cs[0][j], cs[1][j])
        if not md[2][j]:
            raise ValueError("alignment %s has neither a cs nor an MD tag" % c.f(j, 0))
        return get_cs(c.f(j, 5), self._span(md[0][j], md[1][j]))

    # ---- the readers ----
    def length_records(self):
        """lengths.length_records of the text"""
        refs, records = [], []
        sel, err = self._stream(6, refs)
        c = self._Cursor(self, sel)
        for j, star in enumerate(c.star(5)):
            if not star:
                records.append((c.f(j, 0), c.flag(j), c.f(j, 2), c.pos(j), c.f(j, 5)))
        if err is not None:
            raise err
        known = set(n for n, _ in refs)
        for r in records:
            if r[2] not in known:
                raise no_sq_line(r[0], r[2])
        return refs, records

    def primary_and_unaligned(self):
        """lengths.primary_and_unaligned of the text"""
        refs, records, pos_strand = [], [], 0
        sel, err = self._stream(11, refs)
        c = self._Cursor(self, sel)
        flags, plain = self._flags(sel)
        fs, fe = c.fs_a, c.fe_a
        seq_len = np.where(self._is_star(fs, fe, 9), 0, fe[:, 9] - fs[:, 9])
        if not plain:                                       # a FLAG that is not plain: the loop of the path reader, int() where it has one
            unaligned = []
            for j in range(len(sel)):
                flag = c.flag(j)
                if not flag & (0x4 | 0x100 | 0x800):
                    records.append((c.f(j, 0), flag, c.f(j, 2), c.pos(j), c.f(j, 5)))
                    if flag == 0:
                        pos_strand += 1
                elif flag & 0x4:
                    unaligned.append(int(seq_len[j]))
            unaligned = np.array(unaligned, dtype=np.int64)
        else:
            primary = flags & 0x904 == 0
            for j in np.flatnonzero(primary).tolist():
                records.append((c.f(j, 0), c._flag[j], c.f(j, 2), c.pos(j), c.f(j, 5)))
            pos_strand = int(np.count_nonzero(flags[primary] == 0))
            unaligned = seq_len[~primary & (flags & 0x4 != 0)].astype(np.int64)
        if err is not None:
            raise err
        if not records:
            raise ValueError("%s holds no primary alignment" % self._name)
        return refs, records, unaligned, float(pos_strand) / len(records)

    def cs_from_sam(self):
        """errors.cs_from_sam of the text"""
        sel, _ = self._stream(11)
        c = self._Cursor(self, sel)
        cs, md = self._tags(sel, SAM_TAG_CS), self._tags(sel, SAM_TAG_MD)
        return [self._cs_of(c, j, cs, md) for j, star in enumerate(c.star(5)) if not star]

    def quals_from_sam(self, primary_only: bool = True):
        """qualities.quals_from_sam of the text"""
        aligned, unmapped = [], []
        drop = 0x100 | 0x800 if primary_only else 0x100
        sel, _ = self._stream(11)
        c = self._Cursor(self, sel)
        cs, md = self._tags(sel, SAM_TAG_CS), self._tags(sel, SAM_TAG_MD)
        for j, star in enumerate(c.star(10)):
            flag = c.flag(j)
            if flag & 0x4:
                if not star:
                    unmapped.append(c.f(j, 10))
            elif not flag & drop:
                if star:
                    raise ValueError("alignment %s has no QUAL" % c.f(j, 0))
                text = self._cs_of(c, j, cs, md)
                cigar = c.f(j, 5)
                h, t = _CLIP_HEAD.match(cigar), _CLIP_TAIL.search(cigar)
                aligned.append((text, c.f(j, 10), int(h.group(1)) if h else 0, int(t.group(1)) if t else 0))
        return aligned, unmapped

    def sam_records(self):
        """sam_pairs.sam_records of the text"""
        out = []
        sel, _ = self._stream(11)
        rows = self.rows[sel]
        width = rows["field_end"][:, 1].astype(np.int64) - rows["field_end"][:, 0] - 1
        keep = (rows["bits"] & SAM_FLAG_ODD == 0) & (((rows["flag"] == 0) & (width == 1)) | ((rows["flag"] == 16) & (width == 2)))       # FLAG is the text `0` or `16`
        sel = sel[keep]
        c = self._Cursor(self, sel)
        md = self._tags(sel, SAM_TAG_MD)
        for j in range(len(sel)):
            if not md[2][j]:
                raise ValueError("alignment %s has no MD tag" % c.f(j, 0))
            cigar = c.f(j, 5)
            if "H" in cigar:
                raise ValueError("alignment %s has a hard clip in its CIGAR (src/pairwise2maf.py:59-67 stops on it)" % c.f(j, 0))
            out.append((c.f(j, 0), c._flag[j], c.f(j, 2), c.pos(j), cigar, self._span(md[0][j], md[1][j]), c.f(j, 9)))
        return out

    def chimeric_records(self):
        """chim_select.chimeric_records of the text"""
        from .chim_select import ChimRecord, sa_entries
        refs, records, unaligned = [], [], []
        seen_primary = False
        sel, err = self._stream(11, refs)
        c = self._Cursor(self, sel)
        nm_tag, sa_tag = self._tags(sel, SAM_TAG_NM), self._tags(sel, SAM_TAG_SA)
        nms = self.rows["nm"][sel].tolist()
        star = c.star(9)
        seq_b, seq_e = c.col(9)
        begin, end = self.rows["begin"][sel].tolist(), self.rows["end"][sel].tolist()
        for j in range(len(sel)):
            flag = c.flag(j)
            seq_len = 0 if star[j] else seq_e[j] - seq_b[j]
            if flag & 0x4:
                unaligned.append(seq_len)
                continue
            nm = sa = None
            if nm_tag[2][j]:
                nm = int(self._span(nm_tag[0][j], nm_tag[1][j])) if c.bits[j] & SAM_NM_ODD else nms[j]
            if sa_tag[2][j]:
                sa = self._span(sa_tag[0][j], sa_tag[1][j])
            if not flag & (0x100 | 0x800):
                seen_primary = True
                if nm is None:
                    raise ValueError("primary alignment of read %s has no NM:i tag" % c.f(j, 0))
                if nm < 0:
                    raise ValueError("primary alignment of read %s has a negative NM" % c.f(j, 0))
            elif not seen_primary:
                raise ValueError("record of read %s (FLAG %d) stands in front of the first primary alignment" % (c.f(j, 0), flag))
            records.append(ChimRecord(c.f(j, 0), flag, c.f(j, 2), c.pos(j), c.f(j, 5), nm, sa, seq_len, self._line(begin[j], end[j])))
        if err is not None:
            raise err
        if not seen_primary:
            raise ValueError("%s holds no primary alignment" % self._name)
        known = set(n for n, _ in refs)
        for r in records:
            if r.rname not in known:
                raise no_sq_line(r.qname, r.rname)
            if r.sa is not None and not r.flag & (0x100 | 0x800):
                for e in sa_entries(r.sa, r.qname):
                    if e[0] not in known:
                        raise ValueError("an SA entry of read %s lies on %s, which has no @SQ line" % (r.qname, e[0]))
        return refs, records, np.array(unaligned, dtype=np.int64), self.header_lines()

    def mapped_rows(self) -> np.ndarray:
        """the positions in self.rows of the records chimeric_records keeps, in its order: 11 fields or more and not unmapped"""
        sel, _ = self._stream(11)
        flags, plain = self._flags(sel)
        if plain:
            return sel[flags & 0x4 == 0]
        c = self._Cursor(self, sel)
        return sel[[j for j in range(len(sel)) if not c.flag(j) & 0x4]]

    def unmapped_quals(self):
        """the second list of quals_from_sam alone: QUAL of the unmapped records that have one"""
        sel, _ = self._stream(11)
        c = self._Cursor(self, sel)
        return [c.f(j, 10) for j, star in enumerate(c.star(10)) if c.flag(j) & 0x4 and not star]

    def mapped_records(self):
        """what ir_model._mapped_records gives for the text, as a list: the fields of every record of six fields or more that is not
        unmapped.  Fields 0 .. 10 come from the row's offsets; what stands behind them — the optional fields — is cut at its tabs."""
        out = []
        sel, _ = self._stream(6)
        c = self._Cursor(self, sel)
        n_fields, end = self.rows["n_fields"][sel].tolist(), self.rows["end"][sel].tolist()
        for j in range(len(sel)):
            if c.flag(j) & 0x4:
                continue
            fld = [c.f(j, k) for k in range(min(n_fields[j], 11))]
            if n_fields[j] > 11:
                fld += self._span(c.col(10)[1][j] + 1, end[j]).split("\t")
            out.append(fld)
        return out
