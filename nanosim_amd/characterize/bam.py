"""BAM as alignment input: what the reference's aligner step writes (``minimap2 ... | samtools view -b``, src/read_analysis.py:84,136,170)
and every stage of it opens through pysam.  Here the records are decoded to SAM text on the GPU (``ns_bam_to_sam``, csrc/ns_bam.h): byte
for byte what ``samtools view -h`` prints, which is what the seven readers of sam_text take:

    bam = characterize.read_bam("training_primary.bam", eng)
    characterize.hist("training", characterize.cs_from_sam(bam), eng)       # wherever a reader takes the path of a SAM file
    characterize.bam_to_sam("training.bam", "training.sam", eng)            # the text as a file

This module reads the container.  BGZF: the blocks are walked by their BSIZE (the `BC` subfield of the gzip member's extra field),
inflated in a thread pool, and checked against their CRC32 and ISIZE.  The header: ``BAM\\1``, l_text and the text, n_ref, and per
reference l_name, the name and l_ref; a text without any @SQ line gets one ``@SQ\\tSN:<name>\\tLN:<l_ref>`` per entry of the dictionary
behind its @HD line, as htslib prints it.  The inflated bytes go to the library in batches of whole blocks (about BATCH_BYTES) with the
unconsumed tail of the call before in front: memory is bounded by the batch, not by the file.
ValueError, with the file: a member that is not a BGZF block or lacks the BC field, a bad CRC or ISIZE, a truncated last block, a file
without the empty end-of-file block at its end, a header that is not one, and a bad record, with its number, its offset in the inflated
stream and the reason."""
import ctypes as C
import io
import mmap
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ._abi import _pack, ptr
from .sam_text import SamSource

BATCH_BYTES = 64 << 20
INFLATE_THREADS = 16
BAD_REASONS = {1: "block_size is negative or smaller than what the record's own counts need", 2: "l_seq is negative",
               3: "a refID outside [-1, n_ref)", 4: "the name is not NUL-terminated", 5: "a tag of an unknown type",
               6: "a Z or H tag without a NUL inside the record", 7: "a tag's count or value runs past the record",
               8: "the file ends inside a record"}


class NsBamResult(C.Structure):
    """mirror of ns_bam_result (include/nanosim_amd.h)"""
    _fields_ = [("text", C.c_void_p), ("line_off", C.c_void_p), ("n_records", C.c_uint64), ("n_text", C.c_uint64), ("consumed", C.c_uint64),
                ("first_bad", C.c_uint64), ("first_bad_offset", C.c_uint64), ("bad_reason", C.c_uint32), ("reserved", C.c_uint32),
                ("ms_kernel", C.c_double)]


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_blocks(path: str):
    """the BGZF blocks of a file that hold data, in order: (the raw deflate data, CRC32, ISIZE, the block's offset) of each.  The empty
    end-of-file block has to stand at the end of the file: that is looked at first, so that a truncated file fails before any work."""
    size = os.path.getsize(path)
    if size == 0:
        raise ValueError("%s: an empty file is not a BAM file" % path)
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
        if m[:2] != b"\x1f\x8b":
            raise ValueError("%s: not a BGZF file (no gzip magic)" % path)
        if size < len(BGZF_EOF) or m[size - len(BGZF_EOF):size] != BGZF_EOF:
            raise ValueError("%s: no empty end-of-file block at the end: the file is truncated" % path)
        at = 0
        while at < size:
            if size - at < 18:
                raise ValueError("%s: truncated: %d bytes behind the last BGZF block, at offset %d" % (path, size - at, at))
            if m[at:at + 3] != b"\x1f\x8b\x08" or not m[at + 3] & 4:
                raise ValueError("%s: the gzip member at offset %d has no BC field: gzip, not BGZF" % (path, at))
            xlen, = struct.unpack_from("<H", m, at + 10)
            x, x_end, bsize = at + 12, at + 12 + xlen, None
            if x_end > size:
                raise ValueError("%s: truncated inside the BGZF block at offset %d" % (path, at))
            while x + 4 <= x_end:
                si1, si2, slen = struct.unpack_from("<BBH", m, x)
                if (si1, si2, slen) == (66, 67, 2) and x + 6 <= x_end:
                    bsize, = struct.unpack_from("<H", m, x + 4)
                x += 4 + slen
            if bsize is None:
                raise ValueError("%s: the gzip member at offset %d has no BC field: gzip, not BGZF" % (path, at))
            total = bsize + 1
            if total < 12 + xlen + 8:
                raise ValueError("%s: the BGZF block at offset %d is smaller than its own header" % (path, at))
            if at + total > size:
                raise ValueError("%s: truncated: the BGZF block at offset %d has %d bytes, the file ends after %d" % (path, at, total, size - at))
            crc, isize = struct.unpack_from("<II", m, at + total - 8)
            if isize:
                yield m[x_end:at + total - 8], crc, isize, at
            at += total


def _inflate(path, block):
    data, crc, isize, at = block
    try:
        raw = zlib.decompress(data, -15)
    except zlib.error as e:
        raise ValueError("%s: the BGZF block at offset %d does not inflate: %s" % (path, at, e))
    if len(raw) != isize:
        raise ValueError("%s: the BGZF block at offset %d inflates to %d bytes, its ISIZE says %d" % (path, at, len(raw), isize))
    if zlib.crc32(raw) != crc:
        raise ValueError("%s: bad CRC32 in the BGZF block at offset %d" % (path, at))
    return raw


def inflated_batches(path: str, batch_bytes: int = BATCH_BYTES):
    """the inflated bytes of a BGZF file as a sequence of bytes objects, each the whole blocks of about batch_bytes"""
    with ThreadPoolExecutor(max_workers=min(INFLATE_THREADS, os.cpu_count() or 1)) as pool:
        group, held = [], 0
        for block in bgzf_blocks(path):
            group.append(block)
            held += block[2]
            if held >= batch_bytes:
                yield b"".join(pool.map(lambda b: _inflate(path, b), group))
                group, held = [], 0
        if group:
            yield b"".join(pool.map(lambda b: _inflate(path, b), group))


def _read_header(path, batches):
    """(header text, [(name, length)], the inflated bytes behind the header that were read along) from the iterator over the batches"""
    buf = b""

    def need(n):
        nonlocal buf
        while len(buf) < n:
            more = next(batches, None)
            if more is None:
                raise ValueError("%s: the file ends inside the BAM header" % path)
            buf += more
    need(8)
    if buf[:4] != b"BAM\1":
        raise ValueError("%s: not a BAM file: the inflated bytes do not begin with BAM\\1" % path)
    l_text, = struct.unpack_from("<i", buf, 4)
    if l_text < 0:
        raise ValueError("%s: not a BAM header: l_text is negative" % path)
    need(12 + l_text)
    text = buf[8:8 + l_text].split(b"\0", 1)[0].decode()
    n_ref, = struct.unpack_from("<i", buf, 8 + l_text)
    if n_ref < 0:
        raise ValueError("%s: not a BAM header: n_ref is negative" % path)
    at, refs = 12 + l_text, []
    for _ in range(n_ref):
        need(at + 4)
        l_name, = struct.unpack_from("<i", buf, at)
        if l_name < 1:
            raise ValueError("%s: not a BAM header: the name of reference %d has no bytes" % (path, len(refs)))
        need(at + 4 + l_name + 4)
        name = buf[at + 4:at + 4 + l_name].split(b"\0", 1)[0]
        l_ref, = struct.unpack_from("<i", buf, at + 4 + l_name)
        refs.append((name, l_ref))
        at += 8 + l_name
    if text and not text.endswith("\n"):
        text += "\n"
    lines = text.splitlines(True)
    if refs and not any(x.startswith("@SQ\t") for x in lines):
        k = 1 if lines and lines[0].startswith("@HD") else 0
        lines[k:k] = ["@SQ\tSN:%s\tLN:%d\n" % (name.decode(), l_ref) for name, l_ref in refs]
    return "".join(lines), refs, buf[at:]


def bam_call(eng, data, final: bool, ref_names=None, ref_off=None) -> NsBamResult:
    """ns_bam_to_sam on inflated BAM records (bytes or a uint8 array that begins at a record boundary); ref_names / ref_off: _pack of
    the names of the header's dictionary.  Raises nothing for a bad record: the caller knows the file.  The arrays of the result are
    the library's until its next call."""
    a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    out = NsBamResult()
    n_ref = 0 if ref_off is None else len(ref_off) - 1
    eng._check(eng.L.ns_bam_to_sam(eng.ctx, ptr(a), len(a), 1 if final else 0, ptr(ref_names) if n_ref else None, ptr(ref_off) if n_ref else None,
                                   n_ref, C.addressof(out)))
    return out


class BamText(SamSource):
    """The SAM text of a BAM file: iterating gives its lines, the header's first, each with its '\\n', as a SAM file opened for reading
    does; every iteration decodes the file again (nothing of the text is kept).  `header`: the header lines as one string; `refs`:
    [(name, length)] of the reference dictionary; `path` and str(): the file, for messages."""

    def __init__(self, path: str, eng, batch_bytes: int = BATCH_BYTES):
        self.path, self.eng, self.batch_bytes = str(path), eng, batch_bytes
        self.header, self.refs, _ = _read_header(self.path, inflated_batches(self.path, min(batch_bytes, 1 << 20)))
        self.ms_kernel = 0.0

    def __str__(self):
        return self.path

    def texts(self):
        """per batch: (the text of its records as bytes, the offsets of its lines — len + 1 of them, uint64)"""
        batches = inflated_batches(self.path, self.batch_bytes)
        _, refs, tail = _read_header(self.path, batches)
        names, off = _pack([name for name, _ in refs])
        done_records = done_bytes = 0
        self.ms_kernel = 0.0
        more = next(batches, None)
        while True:
            final = more is None
            data = tail if final else (tail + more if tail else more)
            r = bam_call(self.eng, data, final, names, off)
            if r.bad_reason:
                raise ValueError("%s: record %d, at offset %d of the inflated records, is bad: %s"
                                 % (self.path, done_records + int(r.first_bad), done_bytes + int(r.first_bad_offset),
                                    BAD_REASONS.get(int(r.bad_reason), "reason %d" % r.bad_reason)))
            self.ms_kernel += float(r.ms_kernel)
            n = int(r.n_records)
            if n:
                yield (C.string_at(r.text, int(r.n_text)),
                       np.frombuffer(C.string_at(r.line_off, 8 * (n + 1)), dtype=np.uint64))         # (copies: the library's arrays live until its next call)
            done_records += n
            done_bytes += int(r.consumed)
            if final:
                return
            tail = data[int(r.consumed):]
            more = next(batches, None)

    def __iter__(self):
        yield from self.header.splitlines(True)
        for text, _ in self.texts():
            yield from io.TextIOWrapper(io.BytesIO(text))           # (the lines as open(path) gives them for the same text in a file)


def read_bam(path: str, eng) -> BamText:
    """the SAM text of a BAM file, decoded on the GPU, for sam_lines and every reader over it"""
    return BamText(path, eng)


def bam_to_sam(path: str, out_path: str, eng) -> int:
    """writes what `samtools view -h` prints for the BAM file; -> the number of records"""
    bam = read_bam(path, eng)
    n = 0
    with open(out_path, "wb") as f:
        f.write(bam.header.encode())
        for text, off in bam.texts():
            f.write(text)
            n += len(off) - 1
    return n
