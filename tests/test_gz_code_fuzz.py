"""The code builder of the compressed output ("BGZF output"; gz_huff_lengths, gz_canonical, the run-length tokens, gz_code_valid
and gz_dev_code of nanosim_amd/csrc/ns_gz.h) without an engine and without a GPU: the `code` and `valid` modes of tests/gz_wave_host.cpp, a
g++ program, so that scripts/mutation_audit.py --gz can run this file against every mutant of the builder.  The judge is
gz_lib.ref_code_checks — lengths, Kraft sum, canonical codes, the cost of a heapq Huffman tree, a plain reader of RFC 1951 3.2.7 over the
header, zlib's inflate — over a fixed-seed fuzz of histograms, and token lists, CRC tables and spoiled codes written out by hand.

tests/test_gz_code.py judges the library that ships, through ctypes; this file the same text in a program of its own."""
import zlib

import numpy as np
import pytest

from tests import gz_lib as G

U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def exe():
    return G.build_program()


def hist_at(values, counts):
    h = np.zeros(256, dtype=np.uint64)
    for v, c in zip(values, counts):
        h[int(v)] = int(c)
    return h


def fuzz_hists():
    """about 2 000 histograms: (class, 256 counts)"""
    rng = np.random.default_rng(20261021)
    fib = [1, 1]
    while len(fib) < 80:
        fib.append(fib[-1] + fib[-2])
    out = []

    def some(k):                                    # k values, every other time one block of neighbours (long runs of equal lengths)
        if rng.integers(2):
            return np.sort(rng.choice(256, k, replace=False))
        return (int(rng.integers(256)) + np.arange(k)) % 256
    for _ in range(230):
        k = int(rng.integers(1, 257))
        out.append(("uniform", hist_at(some(k), rng.integers(1, 21, k))))
        out.append(("exp40", hist_at(some(k), [int(np.exp(x)) for x in rng.uniform(0, 40, k)])))
        out.append(("geometric", hist_at(some(k), rng.geometric(rng.uniform(0.01, 0.5), k))))
        out.append(("ones", hist_at(some(k), [1] * k)))
        out.append(("pow2", hist_at(some(k), [1 << int(e) for e in rng.integers(0, 63, k)])))
        out.append(("one_to_three", hist_at(some(k), rng.integers(1, 4, k))))
        out.append(("saturating", hist_at(some(k), [U64 - int(d) for d in rng.integers(0, 6, k)])))
        k = int(rng.integers(2, 81))
        out.append(("fibonacci", hist_at(some(k), rng.permutation(fib[:k]))))
    for bits in range(1, 9):                        # 2^bits - 1 values of one count: with end-of-block, every code has `bits` bits
        for c in (1, 7, 1 << 40, U64):
            out.append(("flat", hist_at(some((1 << bits) - 1), [c] * ((1 << bits) - 1))))
    for k in (0, 1, 2, 255, 256):
        for _ in range(30):
            out.append(("used_%d" % k, hist_at(some(k), [int(np.exp(x)) for x in rng.uniform(0, 20, k)])))
    return out


def test_fuzz_of_histograms_against_the_plain_judge(exe, tmp_path):
    hists = fuzz_hists()
    assert 1900 <= len(hists) <= 2100
    got, _, _ = G.build_codes(exe, str(tmp_path), [h for _, h in hists])
    rng = np.random.default_rng(7)
    census = {}
    for (name, h), (code, rc, valid) in zip(hists, got):
        assert rc == 0 and valid, name
        info = G.ref_code_checks(h, code, rng)
        c = census.setdefault(name, {"n": 0, "binds": 0, "cl7": 0, "single": 0, "hclen": set()})
        c["n"] += 1; c["binds"] += info["binds"]; c["cl7"] += info["cl_max"] == 7; c["single"] += info["single"]; c["hclen"].add(info["hclen"])
    print({k: {**v, "hclen": sorted(v["hclen"])} for k, v in census.items()})
    assert set(census) == {"uniform", "exp40", "geometric", "ones", "pow2", "fibonacci", "one_to_three", "saturating", "flat", "used_0", "used_1", "used_2", "used_255", "used_256"}
    assert all(c["n"] >= 30 for c in census.values())
    assert sum(c["binds"] for c in census.values()) >= 20                  # the 15-bit limit binds: the code costs more than the plain tree
    assert census["fibonacci"]["binds"] and census["exp40"]["binds"] and census["pow2"]["binds"]
    assert sum(c["cl7"] for c in census.values()) >= 1                     # a code-length code of 7 bits
    assert census["used_0"]["single"] == census["used_0"]["n"] and sum(c["single"] for c in census.values()) == census["used_0"]["n"]
    # HCLEN + 4: the largest is 19 (a length of 15, the last of the order).  The smallest that a literal code can give is 5, not the 4 of
    # the format: end-of-block always has a length, the first length in the order is 8 at place 5, and 255 values of one count (with
    # end-of-block 256 codes of 8 bits) use no other
    hclen = set().union(*(c["hclen"] for c in census.values()))
    assert min(hclen) == 5 and max(hclen) == 19


def test_all_of_one_count_over_255_values_is_the_shortest_hclen(exe, tmp_path):
    h = np.full(256, 3, dtype=np.uint64)
    h[77] = 0
    code, = G.codes_of(exe, str(tmp_path), [h])
    info = G.ref_code_checks(h, code)
    assert info["hclen"] == 5 and sorted(set(code.len)) == [0, 8]
    assert info["tokens"] == [(8, 0)] + [(16, 6)] * 12 + [(16, 4), (0, 0), (8, 0)] + [(16, 6)] * 29 + [(16, 4), (0, 0)]


def test_equal_counts_get_their_lengths_in_the_order_of_the_values(exe, tmp_path):
    """(freq, symbol) ascending: of 256 values of one count the FIRST shares the deepest pair with end-of-block; of values 3, 4, 5 with
    one count and a heavier 9, value 3 is the one that goes down with end-of-block"""
    flat, few = np.full(256, 1000, dtype=np.uint64), hist_at([3, 4, 5, 9], [2, 2, 2, 4])
    a, b = G.codes_of(exe, str(tmp_path), [flat, few])
    assert a.len == [9] + [8] * 255 + [9]
    assert {v: l for v, l in enumerate(b.len) if l} == {3: 3, 4: 2, 5: 2, 9: 2, 256: 3}
    G.ref_code_checks(flat, a); G.ref_code_checks(few, b)


def test_two_tokens_alone_get_one_bit_each(exe, tmp_path):
    """127 values of one count at every other place: with end-of-block 128 codes of 7 bits, no run of three zeros and no run of four
    equal lengths, so the only tokens are 7 and 0 — the fewest a literal code can have (end-of-block's length and the 0 of the distance
    code are always there), and the code-length code is one bit for each"""
    h = hist_at(range(1, 255, 2), [1] * 127)
    code, = G.codes_of(exe, str(tmp_path), [h])
    info = G.ref_code_checks(h, code)
    assert {s for s, _ in info["tokens"]} == {0, 7} and info["cl_max"] == 1 and info["hclen"] == 6
    assert info["header_bits"] == 17 + 3 * 6 + 258


# a zero run of k between value 0 (count 5: 1 bit) and value k + 1 (count 3: 2 bits, like end-of-block); the zeros behind, written out
ZERO_RUNS = {
    2: [(1, 0), (0, 0), (0, 0), (2, 0), (18, 138), (18, 114), (2, 0), (0, 0)],
    3: [(1, 0), (17, 3), (2, 0), (18, 138), (18, 113), (2, 0), (0, 0)],
    10: [(1, 0), (17, 10), (2, 0), (18, 138), (18, 106), (2, 0), (0, 0)],
    11: [(1, 0), (18, 11), (2, 0), (18, 138), (18, 105), (2, 0), (0, 0)],
    138: [(1, 0), (18, 138), (2, 0), (18, 116), (2, 0), (0, 0)],
    139: [(1, 0), (18, 138), (0, 0), (2, 0), (18, 115), (2, 0), (0, 0)],
    140: [(1, 0), (18, 138), (0, 0), (0, 0), (2, 0), (18, 114), (2, 0), (0, 0)],
    141: [(1, 0), (18, 138), (17, 3), (2, 0), (18, 113), (2, 0), (0, 0)],
    148: [(1, 0), (18, 138), (17, 10), (2, 0), (18, 106), (2, 0), (0, 0)],
    149: [(1, 0), (18, 138), (18, 11), (2, 0), (18, 105), (2, 0), (0, 0)],
}
# runs of equal lengths that are not zero: the values 10 .. with a count of 4 each, a heavier value where the tree needs one, and a
# chain of light values that takes end-of-block away from them.  (the counts, the lengths they must get, the tokens)
EQUAL_RUNS = {
    3: ({10: 4, 11: 4, 12: 4, 200: 1, 201: 2}, {10: 2, 11: 2, 12: 2, 200: 4, 201: 3, 256: 4},
        [(17, 10), (2, 0), (2, 0), (2, 0), (18, 138), (18, 49), (4, 0), (3, 0), (18, 54), (4, 0), (0, 0)]),
    4: ({10: 4, 11: 4, 12: 4, 13: 4, 100: 5, 200: 1, 201: 3}, {10: 3, 11: 3, 12: 3, 13: 3, 100: 2, 200: 4, 201: 3, 256: 4},
        [(17, 10), (3, 0), (16, 3), (18, 86), (2, 0), (18, 99), (4, 0), (3, 0), (18, 54), (4, 0), (0, 0)]),
    7: ({**{10 + i: 4 for i in range(7)}, 200: 1, 201: 2}, {**{10 + i: 3 for i in range(7)}, 200: 5, 201: 4, 256: 5},
        [(17, 10), (3, 0), (16, 6), (18, 138), (18, 45), (5, 0), (4, 0), (18, 54), (5, 0), (0, 0)]),
    8: ({**{10 + i: 4 for i in range(8)}, 100: 20, 200: 1, 201: 3, 202: 6, 203: 12},
        {**{10 + i: 4 for i in range(8)}, 100: 2, 200: 6, 201: 5, 202: 4, 203: 3, 256: 6},
        [(17, 10), (4, 0), (16, 6), (4, 0), (18, 82), (2, 0), (18, 99), (6, 0), (5, 0), (4, 0), (3, 0), (18, 52), (6, 0), (0, 0)]),
}


def test_token_rule_by_hand(exe, tmp_path):
    """16 repeats the last length 3 to 6 times, 17 stands for 3 to 10 zeros, 18 for 11 to 138: every threshold from both sides.  A token
    is (symbol, the lengths it stands for: 0 for a length of its own)"""
    hists = [np.zeros(256, dtype=np.uint64)]
    hists += [hist_at([0, k + 1], [5, 3]) for k in ZERO_RUNS]
    hists += [hist_at(list(c), list(c.values())) for c, _, _ in EQUAL_RUNS.values()]
    codes = G.codes_of(exe, str(tmp_path), hists)
    infos = [G.ref_code_checks(h, c) for h, c in zip(hists, codes)]
    assert infos[0]["tokens"] == [(18, 138), (18, 118), (1, 0), (0, 0)]                  # a zero run of 256
    for k, code, info in zip(ZERO_RUNS, codes[1:], infos[1:]):
        assert {v: l for v, l in enumerate(code.len) if l} == {0: 1, k + 1: 2, 256: 2}, k
        assert info["tokens"] == ZERO_RUNS[k], k
    n = 1 + len(ZERO_RUNS)
    for (r, (_, lens, tokens)), code, info in zip(EQUAL_RUNS.items(), codes[n:], infos[n:]):
        assert {v: l for v, l in enumerate(code.len) if l} == lens, r
        assert info["tokens"] == tokens, r


def reflect32(v):
    return int(format(v, "032b")[::-1], 2)


def x_power(e):
    """x^e modulo the CRC-32 polynomial, bit k the coefficient of x^k"""
    poly = 0x104c11db7

    def mul(a, b):
        p = 0
        while b:
            if b & 1:
                p ^= a
            a <<= 1; b >>= 1
        while p.bit_length() > 32:
            p ^= poly << (p.bit_length() - 33)
        return p
    r, base = 1, 2
    while e:
        if e & 1:
            r = mul(r, base)
        base = mul(base, base); e >>= 1
    return r


def test_crc_tables_of_the_device_code(exe, tmp_path):
    _, crc_tab, lane_pow = G.build_codes(exe, str(tmp_path), [G.fib_counts()])
    assert len(crc_tab) == 256 and len(lane_pow) == 64
    for v in range(256):                                # crc32 of one byte: the register 0xffffffff ^ v through the table, inverted
        assert zlib.crc32(bytes([v])) == (crc_tab[v ^ 0xff] ^ 0x00ffffff) ^ 0xffffffff, v
    for l in range(64):                                 # (the issue of the feature asks for lanes 0, 62 and 63: they are among these)
        assert lane_pow[l] == reflect32(x_power(8 * G.S * (63 - l))), l
    assert lane_pow[63] == 0x80000000


def test_code_valid_on_spoiled_codes(exe, tmp_path):
    good, = G.codes_of(exe, str(tmp_path), [G.fib_counts()])
    assert max(good.len) == 15 and good.len[100] == 15

    def spoiled(**kw):
        c = G.Code(good.len, good.code, good.header_bits, good.header)
        for k, v in kw.items():
            if k == "header_bits":
                c.header_bits = v
            else:
                getattr(c, k[:-1] if k.endswith("_") else k)[v[0]] = v[1]
        return c
    cases = [
        (good, True),
        (spoiled(len_=(100, 16)), False),                                   # a length of 16
        (spoiled(len_=(256, 16)), False),
        (spoiled(len_=(0, 16)), False),
        (spoiled(code=(139, 1 << good.len[139])), False),                   # a code with a bit above its length
        (spoiled(code=(256, 1 << good.len[256])), False),
        (spoiled(code=(100, 1 << 15)), False),
        (spoiled(code=(100, (1 << 15) - 1)), True),                         # ... and the longest code that fits
        (spoiled(len_=(256, 0), code=(256, 0)), False),                     # no end-of-block
        (spoiled(header_bits=16), False), (spoiled(header_bits=17), True),
        (spoiled(header_bits=1880), True), (spoiled(header_bits=1881), False),
        (spoiled(header_bits=0), False), (spoiled(header_bits=1 << 31), False),
    ]
    out = G.run_mode(exe, "valid", str(tmp_path), b"".join(G.code_bytes(c) for c, _ in cases)).split()
    assert [bool(int(x)) for x in out] == [ok for _, ok in cases]
