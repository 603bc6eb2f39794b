"""BAM input of the training side without a GPU ("BAM input"): the container side (nanosim_amd/characterize/bam.py: BGZF,
header, batches) as it is, and the record decode through the engine's own walks compiled for the host (tests/bam_host.cpp over
nanosim_amd/csrc/ns_bam.h, behind the signature of ns_bam_to_sam).  The BAM files are written by tests/bam_lib.py, which shares no code
with the decoder; one record and one header are put together here with literal struct.pack calls against both.  Expected lines are
written out by hand or are the SAM text the BAM was made from.  The check_* functions take an engine: tests/test_gpu_zzzzzzzzz_bam.py
runs them on the GPU."""
import ctypes as C
import gzip
import json
import os
import struct
import subprocess
import types
import zlib

import numpy as np
import pytest

from nanosim_amd import characterize, engine, model
from tests import bam_lib, test_sam_text
from tests.bam_lib import record, tag_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND_OPS, LANE_BYTES, SLICE_BASES, STRLEN_BYTES, FLOAT_SLOT, FLOAT_CHARS = 64, 16, 4096, 8, 16, 12       # ns_bam.h (checked against the header below)
LANES = 64
REFS = [("chr1", 1000), ("chr2", 500), ("chr3", 300)]
HEADER = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + "@PG\tID:minimap2\tPN:minimap2\n"


class HostError(Exception):
    pass


def build_host(lanes: int = 1):
    """an object that stands in for an Engine: its ns_bam_to_sam is the engine's per-wavefront code compiled for the host with one lane
    (or, lanes = 64, on the lock-step wavefront of tests/wave64_host.h)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libbam_host.so" if lanes == 1 else "libbam_host%d.so" % lanes)
    mine = "%s.%d" % (so, os.getpid())                               # (built under a name of its own and moved: test processes may run side by side)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-DBAM_HOST_LANES=%d" % lanes, "-o", mine,
                           os.path.join(ROOT, "tests", "bam_host.cpp")])
    os.replace(mine, so)
    L = C.CDLL(so)
    L.bam_host_to_sam.restype = C.c_int
    L.bam_host_to_sam.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.bam_host_guard.restype = C.c_int
    L.bam_host_guard.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]
    L.bam_host_constant.restype = C.c_uint32
    L.bam_host_constant.argtypes = [C.c_int]

    def check(rc):
        if rc:
            raise HostError("bam_host_to_sam returned %d" % rc)
    return types.SimpleNamespace(ctx=None, _check=check, L=types.SimpleNamespace(ns_bam_to_sam=L.bam_host_to_sam), constant=L.bam_host_constant,
                                 guard=L.bam_host_guard)


@pytest.fixture(scope="module")
def host():
    return build_host()


def raw(eng, data: bytes, final: bool = True, refs=REFS):
    """ns_bam_to_sam on inflated records -> dict(text: bytes, line_off: list, n, consumed, first_bad, first_bad_offset, reason)"""
    names, off = characterize._pack([n for n, _ in refs])
    r = characterize.bam_call(eng, data, final, names, off)
    n = int(r.n_records)
    return dict(text=C.string_at(r.text, int(r.n_text)) if n else b"", n=n, consumed=int(r.consumed),
                line_off=np.frombuffer(C.string_at(r.line_off, 8 * (n + 1)), dtype=np.uint64).tolist() if n else [],
                first_bad=int(r.first_bad), first_bad_offset=int(r.first_bad_offset), reason=int(r.bad_reason), ms_kernel=float(r.ms_kernel))


def lines_of(eng, records, refs=REFS):
    """the lines of these records (bytes each), decoded in one call; checks line_off against them"""
    data = b"".join(records)
    r = raw(eng, data, True, refs)
    assert (r["reason"], r["n"], r["consumed"]) == (0, len(records), len(data)), r
    off = r["line_off"]
    assert off[0] == 0 and off[-1] == len(r["text"]) and len(off) == len(records) + 1
    out = [r["text"][a:b] for a, b in zip(off, off[1:])]
    assert all(x.endswith(b"\n") and x.count(b"\n") == 1 for x in out)
    return out


def write_bam(tmp_path, name, sam_text, block=65280):
    path = os.path.join(str(tmp_path), name)
    with open(path, "wb") as f:
        f.write(bam_lib.sam_to_bam(sam_text, block))
    return path


def decoded(eng, path) -> str:
    return "".join(characterize.read_bam(path, eng))


# ---- the writer and the decoder against bytes and a line put together here -------------------------------------------------------------
def test_writer_and_decoder_against_a_record_packed_by_hand(host, tmp_path):
    name = b"read/1\0"
    cigar = [3 << 4 | 4, 5 << 4 | 0, 1 << 4 | 1, 2 << 4 | 2, 1 << 4 | 0]                 # 3S5M1I2D1M
    seq = bytes([0x12, 0x48, 0x1f, 0x84, 0x21])                                       # A C G T A N T G C A
    qual = bytes([40, 40, 39, 39, 0, 1, 2, 93, 30, 30])
    tags = b"NMC\x03" + b"dvf" + struct.pack("<f", 0.25) + b"cs" + b"Z" + b":5+a-cg:1\0" + b"tsA+"
    body = (struct.pack("<i", 1) + struct.pack("<i", 99) + struct.pack("<B", len(name)) + struct.pack("<B", 60) + struct.pack("<H", 4681) +
            struct.pack("<H", len(cigar)) + struct.pack("<H", 16) + struct.pack("<i", 10) + struct.pack("<i", 2) + struct.pack("<i", 199) +
            struct.pack("<i", -150) + name + b"".join(struct.pack("<I", w) for w in cigar) + seq + qual + tags)
    rec = struct.pack("<i", len(body)) + body
    line = "read/1\t16\tchr2\t100\t60\t3S5M1I2D1M\tchr3\t200\t-150\tACGTANTGCA\tIIHH!\"#~??\tNM:i:3\tdv:f:0.25\tcs:Z::5+a-cg:1\tts:A:+\n"
    text = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:500\n@SQ\tSN:chr3\tLN:300\n"
    t = text.encode()
    header = (b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", 3) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 1000) +
              struct.pack("<i", 5) + b"chr2\0" + struct.pack("<i", 500) + struct.pack("<i", 5) + b"chr3\0" + struct.pack("<i", 300))
    # the writer
    h, refs, recs = bam_lib.parse_sam(text + line)
    assert (h, refs) == (text, REFS) and recs == [rec]
    assert bam_lib.bam_header(h, refs) == header
    assert reg_bin_of(rec) == 4681 == bam_lib.reg2bin(99, 99 + 8)
    # the decoder
    assert lines_of(host, [rec]) == [line.encode()]
    path = os.path.join(str(tmp_path), "hand.bam")
    with open(path, "wb") as f:
        f.write(bam_lib.bgzf(header + rec))
    bam = characterize.read_bam(path, host)
    assert bam.header == text and bam.refs == [(b"chr1", 1000), (b"chr2", 500), (b"chr3", 300)] and str(bam) == path and bam.path == path
    assert list(bam) == (text + line).splitlines(True) == list(bam)                  # (re-iterable)
    # the BGZF block by hand: a gzip member with the BC field, raw deflate, CRC32 and ISIZE
    blk = bam_lib.bgzf_block(b"hello")
    assert blk[:4] == b"\x1f\x8b\x08\x04" and blk[10:18] == struct.pack("<HBBHH", 6, 66, 67, 2, len(blk) - 1)
    assert zlib.decompress(blk[18:-8], -15) == b"hello" and blk[-8:] == struct.pack("<II", zlib.crc32(b"hello"), 5)
    assert gzip.decompress(bam_lib.bgzf(b"hello" * 3, 4)) == b"hello" * 3 and bam_lib.EOF_BLOCK == characterize.BGZF_EOF


def reg_bin_of(rec: bytes) -> int:
    return struct.unpack_from("<H", rec, 4 + 10)[0]


# ---- SAM texts the project has: decoded BAM == the text ----------------------------------------------------------------------------
def encodable(text: str) -> str:
    """the records of a SAM text of tests/test_sam_text.py that a BAM file can hold for REFS — 11 fields or more, on chr1, chr2 or `*` —
    under HEADER (the @SQ line without LN has no place in a BAM dictionary)"""
    keep = [x for x in text.splitlines(True) if not x.startswith("@") and len(x.split("\t")) >= 11 and x.split("\t")[2] in ("chr1", "chr2", "*")]
    return HEADER + "".join(keep)


def golden_sams():
    out = {}
    for name in ("reference_read_len.json.gz", "reference_chimeric_train.json.gz"):
        with gzip.open(os.path.join(ROOT, "tests", "golden", name), "rt") as f:
            out[name] = json.load(f)["sam"]
    return out


def check_project_texts(eng, tmp_path):
    """-> {name: (the SAM text, its BAM file)}"""
    texts = {"sam_text_" + v: encodable(test_sam_text.text_of(v)) for v in test_sam_text.VARIANTS}
    texts.update(golden_sams())
    done = {}
    for name, text in texts.items():
        path = write_bam(tmp_path, name + ".bam", text)
        got = decoded(eng, path)
        assert got == text, name
        done[name] = (text, path)
    assert sum(t.count("\n") for t, _ in done.values()) > 1000
    return done


def test_host_decodes_the_project_sam_texts(host, tmp_path):
    check_project_texts(host, tmp_path)


def check_stage_equality(eng, tmp_path):
    """every reader of test_sam_text.READERS returns or raises the same on the BamText as on the SAM file of the same records"""
    seen = set()
    for v in test_sam_text.VARIANTS:
        text = encodable(test_sam_text.text_of(v))
        sam = os.path.join(str(tmp_path), v + ".sam")
        with open(sam, "w") as f:
            f.write(text)
        bam = characterize.read_bam(write_bam(tmp_path, v + ".bam", text), eng)
        want = test_sam_text.observe(sam)
        for name, reader in test_sam_text.READERS.items():
            try:
                got = {"returns": test_sam_text.plain(reader(bam))}
            except Exception as e:
                got = {"raises": [type(e).__name__, str(e).replace(bam.path, "<path>")]}
            assert json.loads(json.dumps(got)) == json.loads(json.dumps(want[name])), (v, name)
            seen.add((name, "returns" in got))
    assert all((name, True) in seen for name in test_sam_text.READERS) and sum(1 for _, ok in seen if not ok) >= 5


def test_every_reader_gives_the_same_on_bam_as_on_sam(host, tmp_path):
    check_stage_equality(host, tmp_path)


# ---- corner cases, each with its line written out --------------------------------------------------------------------------------------
FLOATS = [0.0, 1e-5, 123456.7, 1e10, 1e-45, float("inf"), float("-inf"), float("nan"), -0.0, 0.1, 1234567.0, -1.17549435e-38, 3.4028235e38, 100000.0,
          1e6, 0.0001, 0.00001234]


def g(x) -> str:
    """C's printf("%g", (double)(float)x)"""
    return "%g" % float(np.float32(x))


def corner_cases():
    """[(record bytes, its line)]"""
    S = "=ACMGRSVTWYHKDBN"
    ints = (tag_bytes("Xc", "c", -128) + tag_bytes("XC", "C", 255) + tag_bytes("Xs", "s", -32768) + tag_bytes("XS", "S", 65535) +
            tag_bytes("Xi", "i", -2147483648) + tag_bytes("XI", "I", 4294967295) + tag_bytes("Xj", "I", 2147483649) + tag_bytes("X0", "c", 0) + tag_bytes("X1", "i", -1))
    arrays = (tag_bytes("Bc", "B", ("c", [-1, 0, 127, -128])) + tag_bytes("BC", "B", ("C", [0, 255])) + tag_bytes("Bs", "B", ("s", [-300, 300])) +
              tag_bytes("BS", "B", ("S", [65535])) + tag_bytes("Bi", "B", ("i", [-2147483648, 7])) + tag_bytes("BI", "B", ("I", [4294967295, 0])) +
              tag_bytes("Bf", "B", ("f", [1.5, -0.25, 1e10])) + tag_bytes("B0", "B", ("c", [])) + tag_bytes("F0", "B", ("f", [])))
    cases = [
        (record("e0", 4, -1, 0, 0, "*", -1, 0, 0, "*", "*"), "e0\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"),
        (record("e1", 0, 0, 1, 255, "1M", -1, 0, 0, "A", "I"), "e1\t0\tchr1\t1\t255\t1M\t*\t0\t0\tA\tI\n"),
        (record("e2", 0, 0, 2, 1, "2M", -1, 0, 0, "NT", "!~"), "e2\t0\tchr1\t2\t1\t2M\t*\t0\t0\tNT\t!~\n"),
        (record("odd", 16, 1, 500, 60, "17=", -1, 0, 0, S + "A", "ABCDEFGHIJKLMNOPQ"), "odd\t16\tchr2\t500\t60\t17=\t*\t0\t0\t" + S + "A\tABCDEFGHIJKLMNOPQ\n"),
        (record("even", 16, 1, 500, 60, "16X", -1, 0, 0, S, "ABCDEFGHIJKLMNOP"), "even\t16\tchr2\t500\t60\t16X\t*\t0\t0\t" + S + "\tABCDEFGHIJKLMNOP\n"),
        (record("noqual", 0, 0, 7, 60, "4M", -1, 0, 0, "ACGT", "*"), "noqual\t0\tchr1\t7\t60\t4M\t*\t0\t0\tACGT\t*\n"),
        (record("q255", 0, 0, 7, 60, "4M", -1, 0, 0, "ACGT", bytes([0, 0xff, 93, 5])), b"q255\t0\tchr1\t7\t60\t4M\t*\t0\t0\tACGT\t!\x20~&\n"),
        (record("nocig", 0, 0, 7, 60, "*", -1, 0, 0, "ACGT", "IIII"), "nocig\t0\tchr1\t7\t60\t*\t*\t0\t0\tACGT\tIIII\n"),
        (record("ops", 0, 0, 7, 60, "1M2I3D4N5S6H7P8=9X", -1, 0, 0, "AC", "II"), "ops\t0\tchr1\t7\t60\t1M2I3D4N5S6H7P8=9X\t*\t0\t0\tAC\tII\n"),
        (record("badop", 0, 0, 7, 60, [5 << 4 | 9, 268435455 << 4 | 15], -1, 0, 0, "AC", "II"), "badop\t0\tchr1\t7\t60\t5?268435455?\t*\t0\t0\tAC\tII\n"),
        (record("ints", 0, 0, 7, 60, "2M", -1, 0, 0, "AC", "II", ints),
         "ints\t0\tchr1\t7\t60\t2M\t*\t0\t0\tAC\tII\tXc:i:-128\tXC:i:255\tXs:i:-32768\tXS:i:65535\tXi:i:-2147483648\tXI:i:4294967295\tXj:i:2147483649\tX0:i:0\tX1:i:-1\n"),
        (record("arrays", 0, 0, 7, 60, "2M", -1, 0, 0, "AC", "II", arrays),
         "arrays\t0\tchr1\t7\t60\t2M\t*\t0\t0\tAC\tII\tBc:B:c,-1,0,127,-128\tBC:B:C,0,255\tBs:B:s,-300,300\tBS:B:S,65535\tBi:B:i,-2147483648,7\t"
         "BI:B:I,4294967295,0\tBf:B:f,1.5,-0.25,1e+10\tB0:B:c\tF0:B:f\n"),
        (record("strings", 0, 0, 7, 60, "2M", -1, 0, 0, "AC", "II", tag_bytes("Z0", "Z", "") + tag_bytes("ZZ", "Z", "a b:c\td") + tag_bytes("HH", "H", "1AE301") +
                tag_bytes("AA", "A", "!") + tag_bytes("Z1", "Z", "x")),
         "strings\t0\tchr1\t7\t60\t2M\t*\t0\t0\tAC\tII\tZ0:Z:\tZZ:Z:a b:c\td\tHH:H:1AE301\tAA:A:!\tZ1:Z:x\n"),
        (record("floats", 0, 0, 7, 60, "2M", -1, 0, 0, "AC", "II", b"".join(tag_bytes("f%x" % (i % 16), "f", x) for i, x in enumerate(FLOATS)) +
                tag_bytes("fB", "B", ("f", FLOATS))),
         "floats\t0\tchr1\t7\t60\t2M\t*\t0\t0\tAC\tII\t" + "\t".join("f%x:f:%s" % (i % 16, g(x)) for i, x in enumerate(FLOATS)) + "\tfB:B:f," +
         ",".join(g(x) for x in FLOATS) + "\n"),
        # the long-CIGAR rule: first op `S` of l_seq and a CG:B:I tag -> the tag's ops, the tag not printed
        (record("cg", 0, 0, 7, 60, [4 << 4 | 4, 30 << 4 | 3], -1, 0, 0, "ACGT", "IIII",
                tag_bytes("NM", "C", 1) + tag_bytes("CG", "B", ("I", [1 << 4 | 4, 70000 << 4 | 0, 3 << 4 | 1])) + tag_bytes("zz", "Z", "after")),
         "cg\t0\tchr1\t7\t60\t1S70000M3I\t*\t0\t0\tACGT\tIIII\tNM:i:1\tzz:Z:after\n"),
        (record("nocg", 0, 0, 7, 60, [4 << 4 | 4, 30 << 4 | 3], -1, 0, 0, "ACGT", "IIII", tag_bytes("NM", "C", 1)),
         "nocg\t0\tchr1\t7\t60\t4S30N\t*\t0\t0\tACGT\tIIII\tNM:i:1\n"),
        (record("cgi", 0, 0, 7, 60, [4 << 4 | 4, 30 << 4 | 3], -1, 0, 0, "ACGT", "IIII", tag_bytes("CG", "B", ("i", [16, 32]))),      # a CG tag, but not B:I
         "cgi\t0\tchr1\t7\t60\t4S30N\t*\t0\t0\tACGT\tIIII\tCG:B:i,16,32\n"),
        (record("cglen", 0, 0, 7, 60, [3 << 4 | 4, 30 << 4 | 3], -1, 0, 0, "ACGT", "IIII", tag_bytes("CG", "B", ("I", [16, 32]))),    # S, but not of l_seq
         "cglen\t0\tchr1\t7\t60\t3S30N\t*\t0\t0\tACGT\tIIII\tCG:B:I,16,32\n"),
        (record("same", 1, 1, 10, 60, "2M", 1, 90, 82, "AC", "II"), "same\t1\tchr2\t10\t60\t2M\t=\t90\t82\tAC\tII\n"),
        (record("third", 1, 1, 10, 60, "2M", 2, 1, 0, "AC", "II"), "third\t1\tchr2\t10\t60\t2M\tchr3\t1\t0\tAC\tII\n"),
        (record("mateun", 9, 1, 10, 60, "2M", -1, 0, -2147483648, "AC", "II"), "mateun\t9\tchr2\t10\t60\t2M\t*\t0\t-2147483648\tAC\tII\n"),
        (record("unplaced", 5, -1, 0, 0, "*", 0, 2147483647, 2147483647, "AC", "II"), "unplaced\t5\t*\t0\t0\t*\tchr1\t2147483647\t2147483647\tAC\tII\n"),
        (record("n" * 254, 65535, 2, 300, 0, "*", -1, 0, 0, "*", "*"), "n" * 254 + "\t65535\tchr3\t300\t0\t*\t*\t0\t0\t*\t*\n"),
    ]
    return [(r, l if isinstance(l, bytes) else l.encode()) for r, l in cases]


def check_corner_cases(eng):
    cases = corner_cases()
    got = lines_of(eng, [r for r, _ in cases])
    for (_, want), line in zip(cases, got):
        assert line == want
    for r, want in cases:                                            # ... and each alone
        assert lines_of(eng, [r]) == [want]
    assert g(1e-45) == "1.4013e-45" and g(123456.7) == "123457" and g(1e10) == "1e+10" and g(float("inf")) == "inf" and g(1e-5) == "1e-05"
    assert raw(eng, b"", True)["n"] == 0 and raw(eng, b"", False)["reason"] == 0


def test_host_corner_cases(host):
    check_corner_cases(host)


def test_header_without_sq_lines_gets_them_behind_hd(host, tmp_path):
    rec = record("r", 0, 1, 5, 60, "2M", -1, 0, 0, "AC", "II")
    for text, want in (("@HD\tVN:1.6\n@PG\tID:x\n", "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:500\n@SQ\tSN:chr3\tLN:300\n@PG\tID:x\n"),
                       ("@PG\tID:x", "@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:500\n@SQ\tSN:chr3\tLN:300\n@PG\tID:x\n"),
                       ("", "@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:500\n@SQ\tSN:chr3\tLN:300\n"),
                       ("@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n", "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n")):
        path = os.path.join(str(tmp_path), "nosq.bam")
        with open(path, "wb") as f:
            f.write(bam_lib.bgzf(bam_lib.bam_header(text, REFS) + rec))
        assert decoded(host, path) == want + "r\t0\tchr2\t5\t60\t2M\t*\t0\t0\tAC\tII\n"
        refs = []
        assert [f[0] for f in characterize.sam_lines(characterize.read_bam(path, host), 11, refs=refs)] == ["r"]
        assert refs == ([("chr1", 1000)] if "@SQ" in text else REFS)


# ---- sizes around the constants of the header ------------------------------------------------------------------------------------------
def sized_sam_text():
    """SAM text whose records sit at -1, 0, +1 around the constants of ns_bam.h — CIGAR ops per round, bytes per lane pass and per
    wavefront pass of the bulk fields, the bytes of a round of the NUL search, the slice length — each at 16 name lengths, so that
    record and line begin at every offset modulo 16; odd and even l_seq"""
    rng = np.random.default_rng(20261020)
    codes = np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)
    lines = []
    shapes = []
    for d in (-1, 0, 1):
        shapes += [(SLICE_BASES + d, 3, 5), (2 * SLICE_BASES + d, 1, 0), (LANE_BYTES * LANES + d, ROUND_OPS + d, LANE_BYTES + d),
                   (LANE_BYTES + d, 2 * ROUND_OPS + d, LANE_BYTES * LANES + d), (2 * LANE_BYTES + d, 1, STRLEN_BYTES * LANES + d), (33 + d, 0, STRLEN_BYTES + d)]
    for k, (l_seq, n_ops, z_len) in enumerate(shapes):
        for pad in range(16 if l_seq < 2 * SLICE_BASES - 1 else 4):
            seq = codes[rng.integers(0, 16, l_seq)].tobytes().decode()
            qual = rng.integers(33, 127, l_seq).astype(np.uint8).tobytes().decode()
            cigar = "".join("%d%s" % (10 ** int(rng.integers(0, 9)) + int(rng.integers(0, 9)), "MIDNSHP=X"[int(rng.integers(0, 9))]) for _ in range(n_ops)) or "*"
            z = rng.integers(33, 127, z_len).astype(np.uint8).tobytes().decode()
            lines.append("s%02d%s\t%d\tchr%d\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\tcs:Z:%s\tBc:B:s%s\n"
                         % (k, "x" * pad, 16 * (pad & 1), 1 + k % 3, 1 + pad, pad, cigar, seq, qual, k * 1000 - 7000, z,
                            "".join(",%d" % v for v in rng.integers(-32768, 32768, max(n_ops, 1)))))
    return HEADER + "".join(lines)


def check_sized_records(eng):
    text = sized_sam_text()
    _, _, recs = bam_lib.parse_sam(text)
    want = [x.encode() for x in text.splitlines(True) if not x.startswith("@")]
    starts = np.cumsum([0] + [len(r) for r in recs])[:-1]
    assert set(int(s) % 16 for s in starts) == set(range(16)) and set(int(s) % 16 for s in np.cumsum([len(x) for x in want])) == set(range(16))
    got = lines_of(eng, recs)
    assert len(got) == len(want) > 200
    for a, b in zip(got, want):
        assert a == b
    return b"".join(got)


def test_host_sizes_around_the_constants(host):
    assert [host.constant(i) for i in range(6)] == [ROUND_OPS, LANE_BYTES, SLICE_BASES, STRLEN_BYTES, FLOAT_SLOT, FLOAT_CHARS]
    src = open(os.path.join(ROOT, "nanosim_amd", "csrc", "ns_bam.h")).read()
    for name, v in (("BAM_ROUND_OPS", ROUND_OPS), ("BAM_LANE_BYTES", LANE_BYTES), ("BAM_SLICE_BASES", SLICE_BASES), ("BAM_STRLEN_BYTES", STRLEN_BYTES)):
        assert "#define %s %du" % (name, v) in src
    check_sized_records(host)


def check_floats_many_and_none(eng):
    """a batch without any float; several floats per record; more floats than the first list holds (4 per record + 1024)"""
    rng = np.random.default_rng(7)
    none = [record("n%d" % i, 0, 0, 1 + i, 60, "4M", -1, 0, 0, "ACGT", "IIII", tag_bytes("NM", "C", i)) for i in range(70)]
    assert lines_of(eng, none) == [b"n%d\t0\tchr1\t%d\t60\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:%d\n" % (i, 1 + i, i) for i in range(70)]
    for per_record, n_rec in ((3, 70), (2500, 3)):
        recs, want = [], []
        for i in range(n_rec):
            v = rng.standard_normal(per_record).astype(np.float32) * np.float32(10.0) ** rng.integers(-8, 9, per_record).astype(np.float32)
            recs.append(record("f%d" % i, 0, 0, 1, 60, "4M", -1, 0, 0, "ACGT", "IIII",
                               tag_bytes("de", "f", float(v[0])) + tag_bytes("zz", "Z", "between") + tag_bytes("fv", "B", ("f", [float(x) for x in v[1:]]))))
            want.append(("f%d\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tde:f:%s\tzz:Z:between\tfv:B:f,%s\n" % (i, g(v[0]), ",".join(g(x) for x in v[1:]))).encode())
        assert lines_of(eng, recs) == want


def test_host_batches_with_and_without_floats(host):
    check_floats_many_and_none(host)


def test_python_g_equals_the_c_library(tmp_path):
    """the oracle of the float cases: Python's "%g" against printf("%g") on 50 000 random bit patterns and the special values"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    src, exe = os.path.join(out, "g.c"), os.path.join(out, "g")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\nint main(void) { float v; while (fread(&v, 4, 1, stdin) == 1) printf("%g\\n", (double)v); return 0; }\n')
    subprocess.check_call(["gcc", "-O1", "-o", exe, src])
    bits = np.random.default_rng(1).integers(0, 2 ** 32, 50000, dtype=np.uint64).astype(np.uint32)
    v = np.concatenate([bits.view(np.float32), np.array(FLOATS, dtype=np.float32)])
    v = v[~(np.isnan(v) & np.signbit(v))]                            # (a nan with the sign bit prints as -nan in C)
    got = subprocess.run([exe], input=v.tobytes(), capture_output=True, check=True).stdout.decode().split("\n")[:-1]
    assert got == [g(x) for x in v] and max(len(x) for x in got) <= FLOAT_CHARS


# ---- batching --------------------------------------------------------------------------------------------------------------------------
def check_batching(eng):
    """one call == two calls cut at every byte position of a record (final = 0, then the tail); final = 1 with a partial record is bad"""
    cases = corner_cases()
    recs = [r for r, _ in cases[:4]] + [cases[13][0]]
    data, whole = b"".join(recs), b"".join(l for _, l in cases[:4]) + cases[13][1]
    bounds = np.cumsum([0] + [len(r) for r in recs]).tolist()
    for cut in range(bounds[1], bounds[3] + 1):
        first = raw(eng, data[:cut], False)
        k = max(i for i, b in enumerate(bounds) if b <= cut)
        assert (first["reason"], first["n"], first["consumed"]) == (0, k, bounds[k]), cut
        second = raw(eng, data[first["consumed"]:], True)
        assert second["reason"] == 0 and first["text"] + second["text"] == whole
        assert first["line_off"][1:] + [first["line_off"][-1] + x for x in second["line_off"][1:]] == np.cumsum([len(l) for _, l in cases[:4]] + [len(cases[13][1])]).tolist()
        if cut not in bounds:
            bad = raw(eng, data[:cut], True)
            assert (bad["reason"], bad["first_bad"], bad["first_bad_offset"], bad["n"], bad["text"]) == (8, k, bounds[k], 0, b""), cut


def test_host_batches_cut_at_every_byte(host):
    check_batching(host)


def test_bam_text_in_small_batches_and_blocks(host, tmp_path):
    """BGZF blocks of 1 byte and of 65 280 bytes, a record across three blocks, batches smaller than a record"""
    text = golden_sams()["reference_read_len.json.gz"]
    small = HEADER + "".join(x for x in test_sam_text.text_of("all_ok").splitlines(True) if x.startswith(("fwd", "rev", "clip")))
    p1 = write_bam(tmp_path, "one.bam", small, 1)
    assert decoded(host, p1) == small
    for block, batch in ((65280, 64 << 20), (97, 64 << 20), (65280, 1000), (300, 1)):
        p = write_bam(tmp_path, "b%d.bam" % block, text, block)
        bam = characterize.BamText(p, host, batch)
        assert "".join(bam) == text
    long_rec = HEADER + "long\t0\tchr1\t1\t60\t700M\t*\t0\t0\t" + "ACGT" * 175 + "\t" + "I" * 700 + "\n"       # > 1 000 bytes: blocks of 400 cut it twice
    assert decoded(host, write_bam(tmp_path, "three.bam", long_rec + "next\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n", 400)).endswith("I\nnext\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n")
    out = os.path.join(str(tmp_path), "out.sam")
    assert characterize.bam_to_sam(p, out, host) == text.count("\n") - sum(1 for x in text.splitlines() if x.startswith("@"))
    assert open(out).read() == text


def test_bgzf_errors_and_paths_given_to_sam_lines(host, tmp_path):
    text = HEADER + "r\t0\tchr1\t1\t60\t2M\t*\t0\t0\tAC\tII\n"
    good = bam_lib.sam_to_bam(text)

    def fails(data, piece, name="bad.bam"):
        p = os.path.join(str(tmp_path), name)
        with open(p, "wb") as f:
            f.write(data)
        with pytest.raises(ValueError) as e:
            "".join(characterize.read_bam(p, host))
        assert piece in str(e.value) and p in str(e.value), str(e.value)
    inflated = bam_lib.bam_header(HEADER, REFS) + record("r", 0, 0, 1, 60, "2M", -1, 0, 0, "AC", "II")
    fails(bam_lib.bgzf_block(inflated, crc=zlib.crc32(inflated) ^ 1) + bam_lib.EOF_BLOCK, "bad CRC32")
    fails(bam_lib.bgzf(inflated, eof=False), "no empty end-of-file block")
    fails(good[:-len(bam_lib.EOF_BLOCK) - 5], "truncated")                                  # cut inside the last block
    fails(good[:-len(bam_lib.EOF_BLOCK) - 40] + bam_lib.EOF_BLOCK, "truncated: the BGZF block at offset 0")
    fails(gzip.compress(inflated) + bam_lib.EOF_BLOCK, "no BC field")
    blk = bytearray(bam_lib.bgzf_block(inflated))
    blk[12:14] = b"XY"                                               # the extra field is there, its subfield is not BC
    fails(bytes(blk) + bam_lib.EOF_BLOCK, "no BC field")
    fails(bam_lib.bgzf(b"BAM\2" + inflated[4:]), "not a BAM file")
    fails(bam_lib.bgzf(inflated[:20]), "ends inside the BAM header")
    fails(bam_lib.bgzf(inflated[:-3]), "record 0, at offset 0 of the inflated records, is bad: the file ends inside a record")
    first = record("r", 0, 0, 1, 60, "2M", -1, 0, 0, "AC", "II")
    fails(bam_lib.bgzf(inflated + record("s", 0, 7, 1, 60, "2M", -1, 0, 0, "AC", "II")),
          "record 1, at offset %d of the inflated records, is bad: a refID outside" % len(first))
    # sam_lines: a SAM path as ever, a BamText, and a BAM path, which names read_bam
    sam, bam = os.path.join(str(tmp_path), "r.sam"), os.path.join(str(tmp_path), "r.bam")
    with open(sam, "w") as f:
        f.write(text)
    with open(bam, "wb") as f:
        f.write(good)
    header, refs = [], []
    assert list(characterize.sam_lines(sam, 11, refs, header, lines=True)) == list(characterize.sam_lines(characterize.read_bam(bam, host), 11, lines=True))
    assert "".join(header) == HEADER and refs == REFS
    with pytest.raises(ValueError, match="read_bam") as e:
        list(characterize.sam_lines(bam, 11))
    assert bam in str(e.value)
    with pytest.raises(ValueError, match="read_bam"):
        characterize.cs_from_sam(bam)


# ---- malformed records -----------------------------------------------------------------------------------------------------------------
def malformed():
    """[(name, bytes: one good record and one bad one, reason, the index of the bad record, its offset)]"""
    good = record("good", 0, 0, 1, 60, "2M", -1, 0, 0, "ACG", "III", tag_bytes("NM", "C", 0))
    base = record("bad", 0, 1, 1, 60, "2M1I", 1, 5, 0, "ACG", "III")

    def patched(at, fmt, value, rec=base):
        b = bytearray(rec)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    def with_tags(tags):
        return record("bad", 0, 1, 1, 60, "2M1I", 1, 5, 0, "ACG", "III", tags)
    cases = [
        ("l_seq larger than the record", patched(4 + 16, "<i", 400), 1),
        ("n_cigar larger than the record", patched(4 + 12, "<H", 60000), 1),
        ("block_size below the fixed fields", struct.pack("<i", 20) + base[4:24], 1),
        ("block_size negative", struct.pack("<i", -5) + base[4:], 1),
        ("block_size one below the fixed fields", struct.pack("<i", 31) + base[4:35] + good, 1),
        ("block_size of the fixed fields alone: no name", struct.pack("<i", 32) + base[4:12] + b"\0" + base[13:16] + struct.pack("<H", 0) + base[18:20] +
         struct.pack("<i", 0) + base[24:36], 4),
        ("l_seq negative", patched(4 + 16, "<i", -1), 2),
        ("refID == n_ref", patched(4, "<i", 3), 3),
        ("refID -2", patched(4, "<i", -2), 3),
        ("next_refID -2", patched(4 + 20, "<i", -2), 3),
        ("next_refID beyond", patched(4 + 20, "<i", 1 << 30), 3),
        ("next_refID == n_ref", patched(4 + 20, "<i", 3), 3),
        ("refID == n_ref, next_refID the last", patched(4 + 20, "<i", 2, patched(4, "<i", 3)), 3),
        ("name without NUL", patched(4 + 32 + 3, "<B", 120), 4),
        ("l_read_name 0", record("", 0, 1, 1, 60, "*", 1, 5, 0, "*", "*")[:12] + b"\0" + record("", 0, 1, 1, 60, "*", 1, 5, 0, "*", "*")[13:], 4),
        ("tag type Q", with_tags(tag_bytes("NM", "C", 1) + b"XQQ\1"), 5),
        ("B subtype Z", with_tags(b"XBBZ" + struct.pack("<I", 1) + b"a"), 5),
        ("B subtype A", with_tags(b"XBBA" + struct.pack("<I", 1) + b"a"), 5),
        ("Z without NUL", with_tags(tag_bytes("NM", "C", 1) + b"XZZ" + b"abcdefghijklmnopqrstu"), 6),
        ("H without NUL", with_tags(b"XHH1A"), 6),
        ("Z empty without NUL", with_tags(b"XZZ"), 6),
        ("B count past the record", with_tags(b"XBBi" + struct.pack("<I", 3) + struct.pack("<ii", 1, 2)), 7),
        ("B count 2^32 - 1", with_tags(b"XBBc" + struct.pack("<I", 0xffffffff) + b"ab"), 7),
        ("B without count", with_tags(b"XBBc\1\0"), 7),
        ("B with three bytes of count", with_tags(b"XBBc\0\0\0"), 7),
        ("B with three bytes of count, a record behind", with_tags(b"XBBc\0\0\0") + good, 7),
        ("i with two bytes", with_tags(b"XIi\1\0"), 7),
        ("two stray bytes", with_tags(tag_bytes("NM", "C", 1) + b"XI"), 7),
    ]
    out = [(name, good + bad, reason, 1, len(good)) for name, bad, reason in cases]
    out.append(("bad first, good second", base[:4] + patched(4 + 16, "<i", -7)[4:] + good, 2, 0, 0))
    out.append(("file ends inside a record", good + base[:-1], 8, 1, len(good)))
    out.append(("file ends inside block_size", good + base[:2], 8, 1, len(good)))
    return out


def check_malformed(eng):
    good = record("good", 0, 0, 1, 60, "2M", -1, 0, 0, "ACG", "III", tag_bytes("NM", "C", 0))
    line = b"good\t0\tchr1\t1\t60\t2M\t*\t0\t0\tACG\tIII\tNM:i:0\n"
    cases = malformed()
    assert set(c[2] for c in cases) == set(range(1, 9))
    for name, data, reason, index, offset in cases:
        r = raw(eng, data, True)
        assert (r["reason"], r["first_bad"], r["first_bad_offset"], r["n"], r["text"], r["consumed"]) == (reason, index, offset, 0, b"", 0), name
        assert lines_of(eng, [good]) == [line]                       # ... and a good record afterwards
    assert set(characterize.BAD_REASONS) == set(range(1, 9))


def test_host_malformed_records(host):
    check_malformed(host)


# ---- the edges of the rounds: what one lane cannot show (run on the one-lane build, on 64 lanes in lock step and on the GPU) ---------------
Z_LENGTHS = (7, 8, 9, 511, 512, 513)                                 # around the bytes of a lane and of a wavefront in the search for a NUL
ROUND_COUNTS = (63, 64, 65, 129)                                     # elements of a B array and ops of a CIGAR around the rounds


def placed(rec: bytes, pos: int) -> bytes:
    """the record at POS pos (1-based), its bin left as it is: beyond 2^29 the writer's reg2bin has no bin, and no line shows one"""
    b = bytearray(rec)
    struct.pack_into("<i", b, 4 + 4, pos - 1)
    return bytes(b)


def edge_cases():
    """[(record bytes, its line)]"""
    cases = [
        (record("same0", 1, 0, 10, 60, "2M", 0, 90, 82, "AC", "II"), "same0\t1\tchr1\t10\t60\t2M\t=\t90\t82\tAC\tII\n"),
        (record("other0", 1, 1, 10, 60, "2M", 0, 90, 82, "AC", "II"), "other0\t1\tchr2\t10\t60\t2M\tchr1\t90\t82\tAC\tII\n"),
        (record("un0", 5, -1, 0, 0, "*", 0, 90, 0, "AC", "II"), "un0\t5\t*\t0\t0\t*\tchr1\t90\t0\tAC\tII\n"),
        (record("last", 1, 2, 10, 60, "2M", 2, 90, 82, "AC", "II"), "last\t1\tchr3\t10\t60\t2M\t=\t90\t82\tAC\tII\n"),
        (placed(record("ten", 1, 0, 1, 60, "2M", 1, 10 ** 9 - 1, -10 ** 9, "AC", "II", tag_bytes("BI", "B", ("I", [10 ** 9, 10 ** 9 - 1])) +
                       tag_bytes("Bi", "B", ("i", [-10 ** 9, 10 ** 9, 10 ** 9 - 1, 1 - 10 ** 9])) + tag_bytes("XI", "I", 10 ** 9) + tag_bytes("Xi", "i", -10 ** 9)), 10 ** 9),
         "ten\t1\tchr1\t1000000000\t60\t2M\tchr2\t999999999\t-1000000000\tAC\tII\tBI:B:I,1000000000,999999999\tBi:B:i,-1000000000,1000000000,999999999,-999999999"
         "\tXI:i:1000000000\tXi:i:-1000000000\n"),
        (placed(record("nine", 1, 0, 1, 60, "2M", 1, 10 ** 9, 10 ** 9, "AC", "II"), 10 ** 9 - 1), "nine\t1\tchr1\t999999999\t60\t2M\tchr2\t1000000000\t1000000000\tAC\tII\n"),
        (record("tlen9", 1, 0, 1, 60, "2M", 1, 1, 10 ** 9 - 1, "AC", "II"), "tlen9\t1\tchr1\t1\t60\t2M\tchr2\t1\t999999999\tAC\tII\n"),
        (record("op9", 0, 0, 1, 60, [(10 ** 8) << 4 | 2, (10 ** 8 - 1) << 4 | 3, 2 << 4], -1, 0, 0, "AC", "II"), "op9\t0\tchr1\t1\t60\t100000000D99999999N2M\t*\t0\t0\tAC\tII\n"),
    ]
    rng = np.random.default_rng(20261022)
    for k, n in enumerate(Z_LENGTHS):                                # a Z value whose NUL is the very last byte of the record
        z = rng.integers(33, 127, n).astype(np.uint8).tobytes().decode()
        cases.append((record("z%d" % n, 0, 0, 1 + k, 60, "2M", -1, 0, 0, "AC", "II", tag_bytes("NM", "C", k) + tag_bytes("zz", "Z", z)),
                      "z%d\t0\tchr1\t%d\t60\t2M\t*\t0\t0\tAC\tII\tNM:i:%d\tzz:Z:%s\n" % (n, 1 + k, k, z)))
    limits = {"c": (-128, 128), "C": (0, 256), "s": (-32768, 32768), "S": (0, 65536), "i": (-2 ** 31, 2 ** 31), "I": (0, 2 ** 32)}
    for n in ROUND_COUNTS:                                           # B arrays; behind each the bytes of the next tag, which are no element
        tags, text = b"", ""
        for sub in "cCsSiIf":
            if sub == "f":
                v = [float(np.float32(x)) for x in rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)]
                shown = [g(x) for x in v]
            else:
                v = [int(x) for x in rng.integers(limits[sub][0], limits[sub][1], n)]
                shown = ["%d" % x for x in v]
            tags += tag_bytes("B" + sub, "B", (sub, v))
            text += "\tB%s:B:%s,%s" % (sub, sub, ",".join(shown))
        cases.append((record("b%d" % n, 0, 0, 1, 60, "2M", -1, 0, 0, "AC", "II", tags + tag_bytes("zz", "Z", "behind")),
                      "b%d\t0\tchr1\t1\t60\t2M\t*\t0\t0\tAC\tII%s\tzz:Z:behind\n" % (n, text)))
        cases.append((record("l%d" % n, 0, 0, 1, 60, "2M", -1, 0, 0, "AC", "II", tag_bytes("BS", "B", ("S", list(range(300, 300 + n))))),     # ... or the next record
                      "l%d\t0\tchr1\t1\t60\t2M\t*\t0\t0\tAC\tII\tBS:B:S,%s\n" % (n, ",".join("%d" % x for x in range(300, 300 + n)))))
    for n in ROUND_COUNTS:                                           # CIGARs; behind the ops the bytes of SEQ, which are no op
        ops = [(int(rng.integers(1, 5000)), "MIDNSHP=X"[int(rng.integers(0, 9))]) for _ in range(n)]
        cigar = "".join("%d%s" % o for o in ops)
        cases.append((record("c%d" % n, 0, 0, 1, 60, cigar, -1, 0, 0, "TGCATGCATGCA", "IIIIIIIIIIII"),
                      "c%d\t0\tchr1\t1\t60\t%s\t*\t0\t0\tTGCATGCATGCA\tIIIIIIIIIIII\n" % (n, cigar)))
    return [(r, l.encode()) for r, l in cases]


def edge_malformed():
    """[(name, bytes, reason, the index of the bad record, its offset)]: a Z value without a NUL that ends its record, and directly
    behind it a record whose first byte — the low byte of its block_size — is 0"""
    behind = record("behind", 0, 0, 1, 60, "2M", -1, 0, 0, "AC", "II", tag_bytes("zz", "Z", "x" * 206))
    assert len(behind) == 4 + 256 and behind[0] == 0
    out = []
    for n in Z_LENGTHS:
        bad = record("bad", 0, 1, 1, 60, "2M1I", 1, 5, 0, "ACG", "III", tag_bytes("NM", "C", 1) + b"XZZ" + b"v" * n)
        out.append(("Z without NUL of %d bytes, a 0 byte behind the record" % n, bad + behind, 6, 0, 0))
        out.append(("... behind a good record", behind + bad + behind, 6, 1, len(behind)))
    return out


def check_edge_cases(eng):
    cases = edge_cases()
    got = lines_of(eng, [r for r, _ in cases])
    for (_, want), line in zip(cases, got):
        assert line == want
    for r, want in cases:                                            # ... each alone, where its last byte is the last of the buffer
        assert lines_of(eng, [r]) == [want]
    behind = edge_malformed()[0][1][-260:]
    for name, data, reason, index, offset in edge_malformed():
        r = raw(eng, data, True)
        assert (r["reason"], r["first_bad"], r["first_bad_offset"], r["n"], r["text"], r["consumed"]) == (reason, index, offset, 0, b"", 0), name
    assert lines_of(eng, [behind]) == [b"behind\t0\tchr1\t1\t60\t2M\t*\t0\t0\tAC\tII\tzz:Z:" + b"x" * 206 + b"\n"]
    return len(cases)


def check_no_references(eng):
    """a file without reference sequences: unmapped records decode, a refID or next_refID of 0 is outside the references"""
    un = record("un", 4, -1, 0, 0, "*", -1, 0, 0, "AC", "II")
    assert lines_of(eng, [un, un], refs=[]) == [b"un\t4\t*\t0\t0\t*\t*\t0\t0\tAC\tII\n"] * 2
    for bad in (record("r0", 4, 0, 1, 0, "*", -1, 0, 0, "AC", "II"), record("n0", 4, -1, 0, 0, "*", 0, 1, 0, "AC", "II")):
        r = raw(eng, un + bad + un, True, refs=[])
        assert (r["reason"], r["first_bad"], r["first_bad_offset"], r["n"], r["text"]) == (3, 1, len(un), 0, b""), bad


def check_store_guards(host):
    """the host build alone (the engine has no such entry): bam_write on room that is shorter or longer than measured — short
    lines cut at every byte, f and B:f bodies included; longer ones inside their tags, behind the first SEQ byte, of no byte — says so and stores nothing outside it"""
    names, off = characterize._pack([n for n, _ in REFS])
    done = 0
    short = [record("g%d" % k, 0, 0, 1, 60, "2M1I", -1, 0, 0, "ACG", "III", tags) for k, tags in enumerate((                # lines cut at every byte
        tag_bytes("de", "f", 0.25) + tag_bytes("zz", "Z", "behind"), tag_bytes("de", "f", -1.17549435e-38) + tag_bytes("fv", "B", ("f", [1e10, 0.5])),
        tag_bytes("fv", "B", ("f", [1.5, -2.25, 1e-5])) + tag_bytes("XA", "A", "!"), tag_bytes("NM", "i", -7) + tag_bytes("de", "f", 3.0),
        tag_bytes("Bs", "B", ("s", [-300, 7, 300])) + tag_bytes("HH", "H", "1AE3")))]
    assert all(len(r) < 100 for r in short)
    for rec in short + [r for r, _ in corner_cases() + edge_cases()]:
        assert host.guard(rec, len(rec), names.ctypes.data, off.ctypes.data, len(REFS)) == 0
        done += 1
    assert done > 50 and sum(1 for _, line in corner_cases() + edge_cases() if b":f:" in line or b":B:f" in line) >= 6    # (f and B:f among them)


def test_host_edges_of_the_rounds(host):
    assert check_edge_cases(host) > 25
    check_no_references(host)
    check_store_guards(host)


def test_host_code_is_clean_under_the_sanitizers(tmp_path):
    """the walks as a stand-alone program under -fsanitize=address,undefined: every malformed record gives its reason, the good files
    their text (n_text and the checksum of the text and the offsets)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBAM_HOST_MAIN", "-o", exe,
                           os.path.join(ROOT, "tests", "bam_host.cpp")])

    def run(data, final=1):
        p = os.path.join(str(tmp_path), "records.bin")
        with open(p, "wb") as f:
            f.write(data)
        a, b = subprocess.check_output([exe, p, str(final)] + [n for n, _ in REFS], text=True).strip().split("\n")
        return [int(x) for x in a.split()], int(b)

    def checksum(text, line_off):
        s = 0
        for c in text:
            s = (s * 31 + c) & (2 ** 64 - 1)
        for o in line_off:
            s = (s * 31 + o) & (2 ** 64 - 1)
        return s
    for name, data, reason, index, offset in malformed() + edge_malformed():
        assert run(data) == ([0, 0, 0, index, offset, reason], 0), name
    cases = corner_cases()
    data, text = b"".join(r for r, _ in cases), b"".join(l for _, l in cases)
    offs = np.cumsum([0] + [len(l) for _, l in cases]).tolist()
    assert run(data) == ([len(cases), len(text), len(data), -1, -1, 0], checksum(text, offs))
    assert run(data[:-1], 0) == ([len(cases) - 1, offs[-2], len(data) - len(cases[-1][0]), -1, -1, 0], checksum(text[:offs[-2]], offs[:-1]))
    sized = sized_sam_text()
    _, _, recs = bam_lib.parse_sam(sized)
    want = b"".join(x.encode() for x in sized.splitlines(True) if not x.startswith("@"))
    got, _ = run(b"".join(recs))
    assert got[:2] == [len(recs), len(want)] and got[5] == 0
    assert run(b"") == ([0, 0, 0, -1, -1, 0], 0)


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------
def test_struct_layout_export_and_abi():
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    c = os.path.join(out, "bam_layout.c")
    with open(c, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "nanosim_amd.h"\nint main(void) {\n'
                'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ns_bam_result), offsetof(ns_bam_result, line_off), offsetof(ns_bam_result, n_records),\n'
                '       offsetof(ns_bam_result, consumed), offsetof(ns_bam_result, first_bad_offset), offsetof(ns_bam_result, bad_reason), offsetof(ns_bam_result, ms_kernel));\n'
                'printf("%d %d %d %u\\n", NS_BAM_BAD_BLOCK_SIZE, NS_BAM_BAD_TAG_COUNT, NS_BAM_BAD_TRUNCATED, (unsigned)NS_ABI_VERSION);\nreturn 0; }\n')
    exe = os.path.join(out, "bam_layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
    a, b = subprocess.check_output([exe], text=True).strip().split("\n")
    R = characterize.NsBamResult
    assert [int(x) for x in a.split()] == [C.sizeof(R), R.line_off.offset, R.n_records.offset, R.consumed.offset, R.first_bad_offset.offset,
                                           R.bad_reason.offset, R.ms_kernel.offset]
    assert [int(x) for x in b.split()] == [1, 7, 8, model.NS_ABI_VERSION] and model.NS_ABI_VERSION == 7
    assert "ns_bam_to_sam" in engine.EXPORTS
    for name in ("read_bam", "bam_to_sam", "BamText", "bam_call", "NsBamResult", "bgzf_blocks"):
        assert hasattr(characterize, name), name
