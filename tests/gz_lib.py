"""What the tests of the compressed output share (tests/test_gz_wave64.py, tests/test_gz_code_fuzz.py, tests/test_gpu_gz_bytes.py): the
inputs the issue of the feature names, the host wavefront program of tests/gz_wave_host.cpp, the two readers every member has to satisfy —
Python's gzip and the project's own BGZF walk (nanosim_amd/characterize/bam.py: BC/BSIZE, CRC32, ISIZE) — and, behind them, the judges that
do not forgive: ref_member, a plain encoder that says what the bytes of a member ARE under a given code, and ref_code_checks, which says
what a code has to be.  Neither takes anything from ns_gz.h but the ns_gz_code it is handed."""
import ctypes
import gzip
import heapq
import os
import struct
import subprocess
import zlib

import numpy as np

from nanosim_amd import engine
from nanosim_amd.characterize import bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = engine.NS_GZ_BLOCK_BYTES
S = B // 64
LENGTHS = [1, 3, 4, S - 1, S, S + 1, 63 * S + 1, B - 1, B]
STARTS = [0, 1, 15]
# the sizes of the sweeps against the plain encoder: every one up to two lanes and two bytes, around 31, 62 and 63 lanes, the block itself
SWEEP_SIZES = list(range(1, 2 * S + 3)) + [S * k + d for k in (31, 62, 63) for d in range(-2, 3)] + [B - 2, B - 1, B]
KINDS = ["acgt", "one", "random", "lacking", "fib"]
MUST_BE_STORED = {"random", "lacking"}


def fib_counts():
    h = np.zeros(256, dtype=np.uint64)
    a, b = 1, 1
    for v in range(40):
        h[100 + v] = a
        a, b = b, a + b
    return h


def counts_of(data: bytes) -> np.ndarray:
    return np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256).astype(np.uint64)


def make_input(kind: str, n: int, seed: int = 1):
    """(the bytes, the counts the code is built from)"""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    if kind == "acgt":
        a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)
        a[79::80] = 10
        return a.tobytes(), counts_of(a.tobytes())
    if kind == "one":
        return b"A" * n, counts_of(b"A" * n)
    if kind == "random":
        a = rng.integers(0, 256, n, dtype=np.uint8)
        if n >= B:                                      # every value at least once: the code lacks none, the block is stored for its size
            a[:256] = np.arange(256, dtype=np.uint8)
        return a.tobytes(), counts_of(a.tobytes())
    if kind == "lacking":                               # one byte in the middle that the code has no code for
        a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)
        a[n // 2] = ord("N")
        h = counts_of(a.tobytes())
        h[ord("N")] = 0
        return a.tobytes(), h
    if kind == "fib":
        h = fib_counts()
        p = h[100:140].astype(np.float64)
        a = rng.choice(np.arange(100, 140, dtype=np.uint8), n, p=p / p.sum())
        return a.tobytes(), h
    raise ValueError(kind)


def check_members(members: bytes, data: bytes, tmp_dir: str, name: str = "m.gz"):
    """gzip gives the input back, and the BGZF walk accepts every member: BSIZE, CRC32, ISIZE <= B, member <= 65536.  Returns the
    (offset, stored) of the members."""
    assert gzip.decompress(members) == data
    path = os.path.join(tmp_dir, name)
    with open(path, "wb") as f:
        f.write(members + bam.BGZF_EOF)
    blocks = list(bam.bgzf_blocks(path))
    raw, out, at_expected = [], [], 0
    for k, blk in enumerate(blocks):
        deflate, crc, isize, at = blk
        assert at == at_expected
        assert 0 < isize <= B
        total = 18 + len(deflate) + 8
        assert total <= 65536
        at_expected += total
        raw.append(bam._inflate(path, blk))
        out.append((at, deflate[0] == 1))
        if k + 1 < len(blocks):
            assert isize == B                          # only the last block of a range is short
    assert at_expected == len(members)
    assert b"".join(raw) == data
    assert len(blocks) == (len(data) + B - 1) // B
    return out


_BUILT = {}


def build_program(sanitize: str | None = None) -> str:
    """the host program, compiled once per process and setting"""
    if sanitize not in _BUILT:
        _BUILT[sanitize] = _build_program(sanitize)
    return _BUILT[sanitize]


def _build_program(sanitize: str | None = None) -> str:
    exe = os.path.join(ROOT, "tests", "_tmp", "gz_wave_host" + ("_" + sanitize.split(",")[0] if sanitize else ""))
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "gz_wave_host.cpp")])
    return exe


def counts_payload(counts) -> bytes:
    """256 counts, or a code as it stands (a Code or an engine.NsGzCode)"""
    return code_bytes(counts) if isinstance(counts, (Code, ctypes.Structure)) else np.ascontiguousarray(counts, dtype="<u8").tobytes()


def run_program(exe: str, tmp_dir: str, jobs):
    """jobs: (data, counts or a code, start[, where in its buffer the first member begins]) each.  Returns per job (the members, [(input bytes, member bytes, stored) per block])"""
    lines, seen = [], {}

    def file_of(kind, payload):                         # (jobs that share an input or a code share its file)
        if (kind, payload) not in seen:
            seen[kind, payload] = os.path.join(tmp_dir, "%s%d.bin" % (kind, len(seen)))
            with open(seen[kind, payload], "wb") as f:
                f.write(payload)
        return seen[kind, payload]
    for k, (data, counts, start, *dst_start) in enumerate(jobs):
        po = os.path.join(tmp_dir, "out%d.bin" % k)
        pc = file_of("code", counts_payload(counts))
        lines.append("%s %s %d %s %d\n" % (file_of("in", data), pc, start, po, dst_start[0] if dst_start else 0))
    pj = os.path.join(tmp_dir, "jobs.txt")
    with open(pj, "w") as f:
        f.writelines(lines)
    done = subprocess.run([exe, pj], capture_output=True, text=True)
    assert done.returncode == 0, (done.stdout[-2000:], done.stderr[-4000:])
    blocks = [[] for _ in jobs]
    for ln in done.stdout.splitlines():
        k, n, m, stored = (int(x) for x in ln.split())
        blocks[k].append((n, m, bool(stored)))
    out = []
    for k in range(len(jobs)):
        with open(os.path.join(tmp_dir, "out%d.bin" % k), "rb") as f:
            out.append((f.read(), blocks[k]))
    return out


# ---------------------------------------------------------------------------------------------------------
# the plain reference: slow and obvious, big integers as bit strings
# ---------------------------------------------------------------------------------------------------------
class Code:
    """an ns_gz_code as plain Python values (engine.NsGzCode has the same four names)"""
    def __init__(self, len_, code, header_bits, header):
        self.len, self.code, self.header_bits, self.header = list(len_), list(code), int(header_bits), bytes(header)

    def struct(self):
        c = engine.NsGzCode()
        c.len[:], c.code[:], c.header_bits = self.len, self.code, self.header_bits
        c.header[:] = self.header + bytes(engine.NS_GZ_HEADER_BYTES - len(self.header))
        return c


def plain_code(c) -> Code:
    """an engine.NsGzCode as a Code"""
    return Code(c.len[:], c.code[:], c.header_bits, bytes(c.header))


def code_bytes(code) -> bytes:
    """the bytes of the ns_gz_code struct"""
    return bytes(code.struct() if isinstance(code, Code) else code)


def bits_lsb(v: int, n: int) -> str:
    """the low n bits of v as text, bit 0 first: the order deflate packs a Huffman code that is kept bit-reversed, and every other field"""
    return format(v & ((1 << n) - 1), "0%db" % n)[::-1] if n else ""


def pack_lsb(bits: str) -> bytes:
    bits += "0" * (-len(bits) % 8)
    return int(bits[::-1], 2).to_bytes(len(bits) // 8, "little") if bits else b""


def header_text(code) -> str:
    return bits_lsb(int.from_bytes(bytes(code.header), "little"), int(code.header_bits))


def assemble(code, data: bytes) -> bytes:
    """the deflate block of `data` under the code: header bits, literals, end-of-block"""
    lens = list(code.len)
    assert all(lens[b] for b in set(data)), "a byte has no code"
    text = [bits_lsb(code.code[s], lens[s]) for s in range(257)]
    return pack_lsb(header_text(code) + "".join([text[b] for b in data]) + text[256])


def coded_bytes(code, data: bytes):
    """the bytes of the dynamic block of `data`; None when the code lacks one of its bytes"""
    lens = list(code.len)
    if any(lens[b] == 0 for b in set(data)):
        return None
    return (int(code.header_bits) + sum([lens[b] for b in data]) + lens[256] + 7) // 8


def ref_member(code, data: bytes) -> bytes:
    """the BGZF member of 1 .. B bytes under the code: stored exactly when the code lacks a byte or the dynamic block is LONGER"""
    n = len(data)
    assert 1 <= n <= B
    coded = coded_bytes(code, data)
    if coded is None or coded > 5 + n:
        block = b"\x01" + struct.pack("<HH", n, n ^ 0xffff) + data
    else:
        block = assemble(code, data)
        assert len(block) == coded
    size = 18 + len(block) + 8
    fixed = bytes([0x1f, 0x8b, 0x08, 0x04,            # ID1 ID2, CM deflate, FLG: FEXTRA
                   0x00, 0x00, 0x00, 0x00,            # MTIME
                   0x00, 0xff,                        # XFL, OS unknown
                   0x06, 0x00,                        # XLEN
                   0x42, 0x43, 0x02, 0x00])           # 'B' 'C', SLEN 2
    return fixed + struct.pack("<H", size - 1) + block + struct.pack("<II", zlib.crc32(data), n)


def ref_members(code, data: bytes) -> bytes:
    return b"".join(ref_member(code, data[at:at + B]) for at in range(0, len(data), B))


def ref_is_stored(member: bytes) -> bool:
    return member[18] == 1


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]          # RFC 1951 3.2.7


def canonical(lens):
    """RFC 1951 3.2.2: {symbol: the code as text, first bit first}"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 17, 0
    for l in range(1, 17):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = format(nxt[l], "0%db" % l)
            nxt[l] += 1
    return out


def parse_header(bits: str):
    """a small reader of RFC 1951 3.2.7 over bit text: (the HLIT + 257 literal lengths, the HDIST + 1 distance lengths, the tokens as
    (symbol, what its extra bits say), the 19 code-length lengths, HCLEN + 4, the bits read)"""
    at = 0

    def take(n):
        nonlocal at
        v = int(bits[at:at + n][::-1], 2) if n else 0
        assert at + n <= len(bits), "the header ends early"
        at += n
        return v
    assert take(1) == 1 and take(2) == 2, "BFINAL 1, BTYPE 10"
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl_len = [0] * 19
    for k in range(hclen):
        cl_len[CL_ORDER[k]] = take(3)
    decode = {v: s for s, v in canonical(cl_len).items()}
    lens, tokens = [], []
    while len(lens) < hlit + hdist:
        word = ""
        while word not in decode:
            assert at < len(bits) and len(word) < 7, "no code-length code"
            word += bits[at]
            at += 1
        s = decode[word]
        if s < 16:
            lens.append(s); tokens.append((s, 0))
        elif s == 16:
            r = 3 + take(2)
            assert lens, "a repeat of nothing"
            lens += [lens[-1]] * r; tokens.append((16, r))
        else:
            r = 3 + take(3) if s == 17 else 11 + take(7)
            lens += [0] * r; tokens.append((s, r))
    assert len(lens) == hlit + hdist, "a run crosses the end of the lengths"
    return lens[:hlit], lens[hlit:], tokens, cl_len, hclen, at


def huffman_cost(weights) -> int:
    """the sum of weight * depth of a Huffman tree (unique, whatever the ties)"""
    h = [int(w) for w in weights]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        s = heapq.heappop(h) + heapq.heappop(h)
        cost += s
        heapq.heappush(h, s)
    return cost


def ref_code_checks(hist, code, rng=None) -> dict:
    """what a code of the histogram has to be; returns what the census of a fuzz counts"""
    hist = [int(x) for x in hist]
    lens = [int(x) for x in code.len]
    assert len(lens) == 257 and max(lens) <= 15
    assert all((lens[v] == 0) == (hist[v] == 0) for v in range(256))
    assert lens[256] > 0
    used = [l for l in lens if l]
    kraft = sum(1 << (15 - l) for l in used)
    single = len(used) == 1
    assert kraft == (1 << 14 if single else 1 << 15) and (not single or used == [1])
    want = canonical(lens)
    for s in range(257):
        assert bits_lsb(code.code[s], lens[s]) == want.get(s, ""), s                # (kept bit-reversed: bit 0 goes first)
        assert code.code[s] >> lens[s] == 0
    freq = [h for h in hist if h] + [1]
    cost, best = sum(f * l for f, l in zip(hist + [1], lens)), huffman_cost(freq) if len(freq) > 1 else 1
    assert cost >= best
    if max(lens) < 15:
        assert cost == best
    hb = int(code.header_bits)
    assert 17 <= hb <= 1880
    raw = bytes(code.header)
    assert len(raw) == engine.NS_GZ_HEADER_BYTES and int.from_bytes(raw, "little") >> hb == 0
    lit, dist, tokens, cl_len, hclen, read = parse_header(header_text(code))
    assert lit == lens and dist == [0] and read == hb
    cl_used = [l for l in cl_len if l]
    assert len(cl_used) >= 2 and sum(1 << (7 - l) for l in cl_used) == 1 << 7
    cl_freq = {}
    for s, _ in tokens:
        cl_freq[s] = cl_freq.get(s, 0) + 1
    assert {s for s in range(19) if cl_len[s]} == set(cl_freq)              # no code for a token that does not occur ...
    cl_cost, cl_best = sum(f * cl_len[s] for s, f in cl_freq.items()), huffman_cost(cl_freq.values())
    assert cl_cost >= cl_best
    if max(cl_len) < 7:                                                     # ... and the cheapest one for those that do
        assert cl_cost == cl_best
    vals = [v for v in range(256) if hist[v]]
    text = bytes(vals + ([vals[int(i)] for i in rng.integers(0, len(vals), 200)] if rng is not None and vals else []))
    assert zlib.decompress(assemble(code, text), -15) == text
    return {"max_len": max(lens), "binds": cost > best, "cl_max": max(cl_len), "single": single, "hclen": hclen, "tokens": tokens, "header_bits": hb}


# ---------------------------------------------------------------------------------------------------------
# the other modes of the host program
# ---------------------------------------------------------------------------------------------------------
def run_mode(exe: str, mode: str, tmp_dir: str, payload: bytes, name: str = None) -> str:
    path = os.path.join(tmp_dir, name or mode + ".bin")
    with open(path, "wb") as f:
        f.write(payload)
    done = subprocess.run([exe, mode, path], capture_output=True, text=True)
    assert done.returncode == 0, (done.stdout[-2000:], done.stderr[-4000:])
    return done.stdout


def build_codes(exe: str, tmp_dir: str, hists):
    """gz_code_build of every histogram in one child process: ([(Code, rc, gz_code_valid's verdict)], crc_tab, lane_pow)"""
    payload = b"".join(np.ascontiguousarray(h, dtype="<u8").tobytes() for h in hists)
    lines = run_mode(exe, "code", tmp_dir, payload).splitlines()
    out = []
    for k in range(len(hists)):
        head, ln, cd, hd = lines[4 * k:4 * k + 4]
        w = head.split()
        assert w[0] == "hist" and int(w[1]) == k and ln.startswith("len ") and cd.startswith("code ") and hd.startswith("header ")
        out.append((Code([int(x) for x in ln.split()[1:]], [int(x) for x in cd.split()[1:]], int(w[4]), bytes.fromhex(hd.split()[1])), int(w[2]), bool(int(w[3]))))
    null, crc, pw = lines[4 * len(hists):]
    assert null == "null -1 -1", null                       # NS_EINVAL for a null histogram and for a null code
    assert crc.startswith("crc_tab ") and pw.startswith("lane_pow ")
    return out, [int(x) for x in crc.split()[1:]], [int(x) for x in pw.split()[1:]]


def codes_of(exe: str, tmp_dir: str, hists):
    """the codes alone, each one built and valid"""
    got, _, _ = build_codes(exe, tmp_dir, hists)
    assert all(rc == 0 and ok for _, rc, ok in got)
    return [c for c, _, _ in got]


def long_header_code() -> Code:
    """A code with a header of 1879 bits, one short of the longest there is, by hand: value 0 has 1 bit, the 255 others and end-of-block 9 (zeros with a
    little of everything deflate well under it), every one of the 258 lengths is a token of its own with no repeats, and the code-length
    code gives the three tokens in use (1, 9, 0) 7, 7 and 6 bits and
    the short codes to tokens nobody uses — wasteful, complete, and deflate to every reader.  gz_code_build cannot be made to write a
    header this long (it picks the best code-length code), but any caller may hand one in, and the walk then has whole prefix words in
    lanes 0 .. 62."""
    lens = [1] + [9] * 256
    cl_len = [0] * 19
    cl_len[1], cl_len[9], cl_len[0] = 7, 7, 6
    for s, l in zip((16, 17, 18, 2, 3), (1, 2, 3, 4, 5)):
        cl_len[s] = l
    assert sum(1 << (7 - l) for l in cl_len if l) == 1 << 7
    cl = canonical(cl_len)
    bits = "1" + bits_lsb(2, 2) + bits_lsb(0, 5) + bits_lsb(0, 5) + bits_lsb(19 - 4, 4) + "".join(bits_lsb(cl_len[s], 3) for s in CL_ORDER)
    bits += "".join(cl[l] for l in lens + [0])
    assert len(bits) == 17 + 57 + 257 * 7 + 6 == 1879
    code = [int(w[::-1], 2) for _, w in sorted(canonical(lens).items())]
    return Code(lens, code, len(bits), pack_lsb(bits) + bytes(engine.NS_GZ_HEADER_BYTES - 235))
