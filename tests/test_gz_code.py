"""The code of a compressed stream ("BGZF output"): ns_gz_code_build through ctypes, no engine and no GPU.  Every code is checked
for what deflate asks of it (lengths of 15 bits at most, a complete prefix code, canonical, no code where the count is 0), and zlib's own
inflate is the judge of the block header: Python assembles header bits + the codes of a byte string + end-of-block, and
zlib.decompress(raw, -15) must give the string back."""
import zlib

import numpy as np
import pytest

from nanosim_amd import engine


@pytest.fixture(scope="module", autouse=True)
def lib():
    import __graft_entry__ as g
    g.build()
    return engine.load_library()


def fib_hist():
    h = np.zeros(256, dtype=np.uint64)
    a, b = 1, 1
    for v in range(40):                 # 40 values with Fibonacci counts: the plain Huffman tree is 39 deep
        h[100 + v] = a
        a, b = b, a + b
    return h


def hist_of(values, counts):
    h = np.zeros(256, dtype=np.uint64)
    h[list(values)] = counts
    return h


HISTS = {
    "acgt_newline": hist_of(b"ACGT\n", [3000, 2000, 2100, 2900, 125]),
    "one_value": hist_of(b"A", [1000]),
    "two_values": hist_of(b"AC", [7, 5]),
    "uniform_256": np.full(256, 1000, dtype=np.uint64),
    "fibonacci_40": fib_hist(),
    "one_next_to_2_40": hist_of([0, 255, 7], [1, 1 << 40, 1]),
}


def text_for(h, n=3000, seed=5):
    """a byte string over the values of the histogram, every value at least once"""
    vals = np.flatnonzero(h).astype(np.uint8)
    rng = np.random.default_rng(seed)
    return np.concatenate([vals, rng.choice(vals, n)]).tobytes()


def rev(code, n):
    return int(format(code, "0%db" % n)[::-1], 2) if n else 0


def assemble(code, data):
    """the deflate block of `data` under the code: header bits, literals, end-of-block, as a bit string packed from bit 0 up"""
    acc, n = int.from_bytes(bytes(code.header), "little") & ((1 << code.header_bits) - 1), code.header_bits
    for b in list(data) + [256]:
        assert code.len[b], "byte %d has no code" % b
        acc |= code.code[b] << n
        n += code.len[b]
    return acc.to_bytes((n + 7) // 8, "little")


@pytest.mark.parametrize("name", sorted(HISTS))
def test_code_properties_and_zlib_reads_the_block(name):
    h = HISTS[name]
    c = engine.build_gz_code(h)
    lens = np.array(c.len[:], dtype=np.int64)
    assert lens.max() <= 15
    assert lens[256] > 0
    assert ((lens[:256] == 0) == (h == 0)).all()
    coded = lens[lens > 0]
    kraft = sum(2.0 ** -int(l) for l in coded)
    assert kraft <= 1.0
    if len(coded) >= 2:
        assert kraft == 1.0
    # canonical (RFC 1951 3.2.2): codes of one length ascend with the symbol, the first of a length follows from the shorter ones
    nxt, code = {}, 0
    for l in range(1, 16):
        code = (code + int((lens == l - 1).sum() if l > 1 else 0)) << 1
        nxt[l] = code
    for s in range(257):
        if lens[s]:
            assert rev(c.code[s], int(lens[s])) == nxt[int(lens[s])], s
            nxt[int(lens[s])] += 1
    assert 17 <= c.header_bits <= 1880
    assert not any(bytes(c.header)[(c.header_bits + 7) // 8:])
    data = text_for(h)
    assert zlib.decompress(assemble(c, data), -15) == data
    assert zlib.decompress(assemble(c, b""), -15) == b""


def test_fibonacci_counts_reach_the_limit_and_rare_values_stay_short_of_it():
    c = engine.build_gz_code(HISTS["fibonacci_40"])
    assert max(c.len[:]) == 15
    c = engine.build_gz_code(HISTS["one_next_to_2_40"])
    assert c.len[255] == 1 and max(c.len[:]) <= 3


def test_empty_histogram_still_gives_a_block_zlib_reads():
    c = engine.build_gz_code(np.zeros(256, dtype=np.uint64))
    assert c.len[256] == 1 and not any(c.len[:256])
    assert zlib.decompress(assemble(c, b""), -15) == b""


def test_bound_and_constants():
    L = engine.load_library()
    B = engine.NS_GZ_BLOCK_BYTES
    assert B % 64 == 0 and B & (B - 1) == 0 and B <= 65280
    for n, r in ((0, 0), (1, 1), (B, 1), (B + 1, 1), (10 * B + 5, 7)):
        assert L.ns_gz_bound(n, r) >= n + 31 * (n // B + r)          # every block stored: 18 + 5 + 8 bytes around it
    member = engine.gz_header_member(b"hello\n")
    import gzip
    assert gzip.decompress(member + engine.BGZF_EOF) == b"hello\n"
    assert len(engine.BGZF_EOF) == 28 and gzip.decompress(engine.BGZF_EOF) == b""
