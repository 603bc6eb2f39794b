"""Test-side BAM writer: SAM text -> BAM records -> BGZF blocks, written from the layout of the format (record fields little-endian:
block_size, refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next_refID, next_pos, tlen, name, cigar, seq, qual, tags) and
sharing no code with the decoder under test (nanosim_amd/csrc/ns_bam.h, nanosim_amd/characterize/bam.py)."""
import re
import struct
import zlib

SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
INT_FORMATS = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def reg2bin(beg: int, end: int) -> int:
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def smallest_int_type(v: int) -> str:
    for t, lo, hi in (("C", 0, 255), ("c", -128, 127), ("S", 0, 65535), ("s", -32768, 32767), ("I", 0, 2 ** 32 - 1), ("i", -2 ** 31, 2 ** 31 - 1)):
        if lo <= v <= hi:
            return t
    raise ValueError(v)


def tag_bytes(tag: str, typ: str, value) -> bytes:
    """one optional field; typ is the STORED type (A c C s S i I f Z H, or B with value = (subtype, [elements]))"""
    head = tag.encode() + typ.encode()
    if typ == "A":
        return head + value.encode()
    if typ in INT_FORMATS:
        return head + struct.pack(INT_FORMATS[typ], value)
    if typ == "f":
        return head + struct.pack("<f", value)
    if typ in "ZH":
        return head + value.encode() + b"\0"
    if typ == "B":
        sub, elements = value
        fmt = "<f" if sub == "f" else INT_FORMATS[sub]
        return head + sub.encode() + struct.pack("<I", len(elements)) + b"".join(struct.pack(fmt, e) for e in elements)
    raise ValueError(typ)


def text_tag(field: str) -> bytes:
    """a `TG:T:value` field of SAM text (an `i` is stored in the smallest type that holds it)"""
    tag, typ, value = field.split(":", 2)
    if typ == "i":
        return tag_bytes(tag, smallest_int_type(int(value)), int(value))
    if typ == "f":
        return tag_bytes(tag, "f", float(value))
    if typ == "B":
        sub, *elements = value.split(",")
        return tag_bytes(tag, "B", (sub, [float(e) if sub == "f" else int(e) for e in elements]))
    return tag_bytes(tag, typ, value)


def cigar_words(cigar: str):
    if cigar == "*":
        return []
    return [int(n) << 4 | CIGAR_OPS.index(op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def record(name, flag, ref_id, pos, mapq, cigar, next_ref_id, next_pos, tlen, seq, qual, tags=b"") -> bytes:
    """one record, block_size included.  pos / next_pos: as SAM has them (1-based); cigar: a string or a list of words; seq: a string
    (`*`: none); qual: a string (`*`: 0xff bytes) or bytes as they are stored; tags: bytes"""
    words = cigar_words(cigar) if isinstance(cigar, str) else list(cigar)
    bases = "" if seq == "*" else seq
    packed = bytearray((len(bases) + 1) // 2)
    for i, c in enumerate(bases):
        packed[i >> 1] |= SEQ_CODES.index(c) << (0 if i & 1 else 4)
    if isinstance(qual, str):
        quals = b"\xff" * len(bases) if qual == "*" else bytes(ord(c) - 33 for c in qual)
    else:
        quals = bytes(qual)
    assert len(quals) == len(bases)
    ref_len = sum(w >> 4 for w in words if w & 15 in (0, 2, 3, 7, 8)) or 1                 # M D N = X
    nm = name.encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref_id, pos - 1, len(nm), mapq, reg2bin(max(pos - 1, 0), max(pos - 1, 0) + ref_len), len(words), flag, len(bases),
                       next_ref_id, next_pos - 1, tlen)
    body += nm + b"".join(struct.pack("<I", w) for w in words) + bytes(packed) + quals + tags
    return struct.pack("<i", len(body)) + body


def parse_sam(text: str):
    """(the header text, [(name, length)] of its @SQ lines, the records as bytes) of SAM text whose records have 11 fields or more"""
    header, refs, lines = [], [], []
    for line in text.splitlines():
        if line.startswith("@"):
            header.append(line + "\n")
            if line.startswith("@SQ\t"):
                t = dict(x.split(":", 1) for x in line.split("\t")[1:])
                refs.append((t["SN"], int(t["LN"])))
        elif line:
            lines.append(line.split("\t"))
    index = {n: i for i, (n, _) in enumerate(refs)}
    index["*"] = -1
    recs = []
    for f in lines:
        rid = index[f[2]]
        nid = rid if f[6] == "=" else index[f[6]]
        recs.append(record(f[0], int(f[1]), rid, int(f[3]), int(f[4]), f[5], nid, int(f[7]), int(f[8]), f[9], f[10], b"".join(text_tag(x) for x in f[11:])))
    return "".join(header), refs, recs


def bam_header(text: str, refs) -> bytes:
    t = text.encode()
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for name, length in refs:
        n = name.encode() + b"\0"
        out += struct.pack("<i", len(n)) + n + struct.pack("<i", length)
    return out


def bgzf_block(data: bytes, crc=None, level: int = 6) -> bytes:
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = z.compress(data) + z.flush()
    total = 12 + 6 + len(cdata) + 8
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1) + cdata +
            struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data)))


def bgzf(data: bytes, block: int = 65280, eof: bool = True) -> bytes:
    """the bytes as BGZF blocks of `block` inflated bytes (the last one shorter), with the empty end-of-file block unless eof is False"""
    out = [bgzf_block(data[i:i + block]) for i in range(0, len(data), block)]
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def sam_to_bam(text: str, block: int = 65280) -> bytes:
    header, refs, recs = parse_sam(text)
    return bgzf(bam_header(header, refs) + b"".join(recs), block)
