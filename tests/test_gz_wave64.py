"""The block walk of the compressed output at 64 lanes without a GPU ("BGZF output"): nanosim_amd/csrc/ns_gz.h compiled for
the host on the lock-step wavefront of tests/wave64_host.h (tests/gz_wave_host.cpp: 64 host threads, every collective a rendezvous).  The
stand-alone program writes whole members; it runs as a child process, built plain, under -fsanitize=address,undefined (the input in a
buffer of exactly its size at byte 0, 1 and 15 of a 16-aligned allocation, the members in a buffer of exactly their sum) and under
-fsanitize=thread (every word of the staging image and every byte of a member is stored by one lane; what another lane wrote is read
behind the fence only).  Nothing is loaded into Python under a sanitizer.

Every output must gunzip to its input, and the BGZF walk of characterize/bam.py must accept every member.  Readers forgive a lot (a
stored block is always a valid answer), so every output must also BE the members of gz_lib.ref_members, the plain encoder, byte for byte:
the inputs of the feature, a sweep of sizes around every lane and word boundary under codes of its own, inputs whose dynamic block is
exactly as long as the stored one, a code with a header of 1 879 bits; gz_member with a wrong size stores nothing; gz_block_at against a
linear scan."""
import numpy as np
import pytest

from tests import gz_lib as G

JOBS = [(kind, n, start) for kind in G.KINDS for n in G.LENGTHS for start in G.STARTS]


def run_all(exe, tmp_path):
    inputs = {(kind, n): G.make_input(kind, n) for kind in G.KINDS for n in G.LENGTHS}
    # (the members begin at byte `start` of their buffer as well: 0, 1 and 3 modulo 4, so that the single bytes in front of the aligned
    # words have a lane of their own to race with under -fsanitize=thread)
    got = G.run_program(exe, str(tmp_path), [inputs[kind, n] + (start, start) for kind, n, start in JOBS])
    codes = dict(zip(inputs, G.codes_of(exe, str(tmp_path), [counts for _, counts in inputs.values()])))
    first = {}
    for (kind, n, start), (members, blocks) in zip(JOBS, got):
        data = inputs[kind, n][0]
        where = "%s, %d bytes at %d" % (kind, n, start)
        assert members == G.ref_members(codes[kind, n], data), where
        walked = G.check_members(members, data, str(tmp_path))
        assert len(blocks) == len(walked) == 1, where
        assert blocks[0][0] == n and blocks[0][1] == len(members) and blocks[0][2] == walked[0][1], where
        assert len(members) <= n + 31, where                       # never more than the stored block
        if kind in G.MUST_BE_STORED:
            assert blocks[0][2], where
        elif n >= G.S - 1:
            assert not blocks[0][2], where                         # (the walk's coded path is what the other kinds are here for)
            if kind != "fib":                                      # a Huffman code spends less than entropy + 1 bits per byte (the 15-bit
                p = G.counts_of(data)[G.counts_of(data) > 0] / n    # limit does not bind below 16 values); 26 + 235 bytes around them
                assert len(members) <= n * (1.0 - float((p * np.log2(p)).sum())) / 8 + 261, where
        assert first.setdefault((kind, n), members) == members, where      # the start of the input changes nothing
    return got


def test_wave64_members_gunzip_and_pass_the_bgzf_walk(tmp_path):
    run_all(G.build_program(), tmp_path)


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_wave64_program_is_clean_under_the_sanitizers(tmp_path, sanitize):
    run_all(G.build_program(sanitize), tmp_path)


def test_wave64_two_blocks_and_a_short_one(tmp_path):
    """more than one block per input: the second and third member begin wherever the one before ends"""
    data, counts = G.make_input("acgt", 2 * G.B + 77)
    (members, blocks), = G.run_program(G.build_program(), str(tmp_path), [(data, counts, 3)])
    walked = G.check_members(members, data, str(tmp_path))
    assert [b[0] for b in blocks] == [G.B, G.B, 77] and [w[0] for w in walked][1:] == [blocks[0][1], blocks[0][1] + blocks[1][1]]
    code, = G.codes_of(G.build_program(), str(tmp_path), [counts])
    assert members == G.ref_members(code, data)


def sweep_jobs():
    """(data, counts or the long-header code, start, dst start): every size up to two lanes and two bytes, the sizes around 31, 62 and 63
    lanes and the block itself, each under four codes of its own — 2, 5, 60 and 256 values with counts exp(U(0, 9)), the bytes drawn by
    those counts — and the sizes of a lane or more under the hand-made code with the long header as well"""
    S, sizes = G.S, G.SWEEP_SIZES
    rng = np.random.default_rng(20261021)
    long_code = G.long_header_code()
    jobs = []
    for n in sizes:
        for n_values in (2, 5, 60, 256):
            values = rng.choice(256, n_values, replace=False)
            weights = np.exp(rng.uniform(0, 9, n_values))
            counts = np.zeros(256, dtype=np.uint64)
            counts[values] = weights.astype(np.uint64)                  # (at least 1: the code has every value)
            data = rng.choice(values, n, p=weights / weights.sum()).astype(np.uint8).tobytes()
            jobs.append((data, counts, len(jobs) % 16, (len(jobs) // 16 + len(jobs)) % 4))
        if n >= S and (n % 7 == 0 or n > 2 * S + 2):
            data = np.where(rng.random(n) < 0.9, 0, rng.integers(0, 256, n)).astype(np.uint8).tobytes()
            jobs.append((data, long_code, len(jobs) % 16, (len(jobs) // 16 + len(jobs)) % 4))
    return jobs


def layout_trace(code, data, dst_start):
    """what the walk's description says of a member, restated: (is stored, prefix bits, the bit at which every lane behind the first one
    with bytes begins, the bit behind the padding of the block)"""
    n = len(data)
    coded = G.coded_bytes(code, data)
    stored = coded is None or coded > 5 + n
    width = (lambda b: 8) if stored else (lambda b: code.len[b])
    prefix = 144 + (40 if stored else code.header_bits)
    gap = G.B - n                                                        # the block lies right-aligned in 64 spans of S bytes
    begins, at, seen_first = [], prefix, False
    for lane in range(64):
        lo, hi = max(lane * G.S - gap, 0), max((lane + 1) * G.S - gap, 0)
        if hi:
            if seen_first:
                begins.append(at)
            seen_first = True
            at += sum(width(b) for b in data[lo:hi])
    end = at + (0 if stored else code.len[256])
    return stored, prefix, begins, (end + 7) // 8 * 8


@pytest.mark.parametrize("sanitize", [None, "address,undefined"])
def test_wave64_sweep_equals_the_plain_encoder(tmp_path, sanitize):
    exe = G.build_program(sanitize)
    jobs = sweep_jobs()
    built = iter(G.codes_of(exe, str(tmp_path), [c for _, c, _, _ in jobs if not isinstance(c, G.Code)]))
    codes = [c if isinstance(c, G.Code) else next(built) for _, c, _, _ in jobs]
    got = G.run_program(exe, str(tmp_path), jobs)
    census = {"prefix_mod_32": set(), "inner_on_word": 0, "inner_off_word": 0, "padding_ends_on_word": 0, "padding_ends_off_word": 0, "pw_40": 0,
              "dst_coded": set(), "dst_stored": set(), "starts": set()}
    for (data, _, start, dst_start), code, (members, blocks) in zip(jobs, codes, got):
        want = G.ref_members(code, data)
        where = "%d bytes at %d to %d, header of %d bits" % (len(data), start, dst_start, code.header_bits)
        assert members == want, where
        stored, prefix, begins, end = layout_trace(code, data, dst_start)
        assert blocks == [(len(data), len(want), stored)] and G.ref_is_stored(want) == stored and len(want) == end // 8 + 8, where
        census["starts"].add(start)
        census["dst_stored" if stored else "dst_coded"].add(dst_start % 4)
        if not stored:
            census["prefix_mod_32"].add(prefix % 32)
            census["inner_on_word"] += sum(b % 32 == 0 for b in begins)
            census["inner_off_word"] += sum(b % 32 != 0 for b in begins)
            census["padding_ends_on_word" if end % 32 == 0 else "padding_ends_off_word"] += 1
            census["pw_40"] += prefix // 32 >= 40 and len(begins) > 0
    print({k: sorted(v) if isinstance(v, set) else v for k, v in census.items()})
    assert census["prefix_mod_32"] == set(range(32))
    assert census["inner_on_word"] >= 10 and census["inner_off_word"] >= 10
    assert census["padding_ends_on_word"] >= 10 and census["padding_ends_off_word"] >= 10
    assert census["pw_40"] >= 10
    assert census["dst_coded"] == census["dst_stored"] == {0, 1, 2, 3} and census["starts"] == set(range(16))


# inputs under the Fibonacci code (header 219 bits; value 100 and end-of-block 15 bits, value 139 2 bits): a times 100, b times 139 make a
# dynamic block of 219 + 15 a + 2 b + 15 bits against the 8 (5 + a + b) of the stored one.  (a, b, the bits the dynamic block has more,
# its bytes less those of the stored block): found by a search over a and b; the block is stored only when it is LONGER in bytes
TIES = [(4, 37, 0, 0), (3, 37, -7, 0), (1, 34, -3, 0), (5, 38, 1, 1), (1, 33, 3, 1), (2, 36, -8, -1), (1, 35, -9, -1)]


def test_wave64_stored_or_coded_at_equal_size(tmp_path):
    exe = G.build_program()
    counts = G.fib_counts()
    code, = G.codes_of(exe, str(tmp_path), [counts])
    assert (code.header_bits, code.len[100], code.len[139], code.len[256]) == (219, 15, 2, 15)
    inputs = [bytes([100]) * a + bytes([139]) * b for a, b, _, _ in TIES]
    got = G.run_program(exe, str(tmp_path), [(data, counts, 0) for data in inputs])
    for (a, b, more_bits, more_bytes), data, (members, blocks) in zip(TIES, inputs, got):
        assert 219 + 15 * a + 2 * b + 15 - 8 * (5 + a + b) == more_bits, (a, b)
        assert G.coded_bytes(code, data) - (5 + len(data)) == more_bytes, (a, b)
        want = G.ref_member(code, data)
        assert G.ref_is_stored(want) == (more_bytes > 0) and members == want, (a, b)
        assert blocks == [(len(data), len(want), more_bytes > 0)], (a, b)


@pytest.mark.parametrize("sanitize", [None, "address,undefined"])
def test_wave64_member_of_another_size_stores_nothing(tmp_path, sanitize):
    """gz_member with a size that is not the member's (the path behind the mismatch counter of k_gz_emit): it answers the true size and
    leaves every byte of its destination as it was"""
    exe = G.build_program(sanitize)
    jobs = [G.make_input(kind, n) + (start,) for kind in G.KINDS for n, start in ((1, 0), (4, 1), (G.S + 1, 2), (63 * G.S + 1, 3), (G.B, 15))]
    jobs.append((bytes(G.B - 5), G.long_header_code(), 1))
    codes = G.codes_of(G.build_program(), str(tmp_path), [c for _, c, _ in jobs[:-1]]) + [jobs[-1][1]]
    lines = []
    for k, (data, counts, start) in enumerate(jobs):
        pi, pc = (tmp_path / ("bad_%s%d.bin" % (x, k)) for x in ("in", "code"))
        pi.write_bytes(data); pc.write_bytes(G.counts_payload(counts))
        lines.append("%s %s %d\n" % (pi, pc, start))
    out = G.run_mode(exe, "badsize", str(tmp_path), "".join(lines).encode(), "badsize.txt").splitlines()
    assert len(out) == len(jobs)
    for k, ((data, _, _), code, ln) in enumerate(zip(jobs, codes, out)):
        true = len(G.ref_member(code, data))
        assert [int(x) for x in ln.split()] == [k, true, true, true, 0], ln


def blocks_by_scan(cuts):
    out = []
    for lo, hi in zip(cuts, cuts[1:]):
        for at in range(lo, hi, G.B):
            out.append((at, min(G.B, hi - at)))
    return out


def test_block_at_equals_a_linear_scan(tmp_path):
    """gz_block_at, the binary search of the kernels for the range of a block: empty ranges in front, in the middle, behind and three in a
    row; ranges of 1, B - 1, B, B + 1 and 2 B bytes; one range and 200"""
    B = G.B
    rng = np.random.default_rng(3)
    sizes = {
        "one": [5 * B + 3], "one_byte": [1], "one_block": [B],
        "empty_in_front": [0, B + 1, 7], "empty_in_the_middle": [B, 0, 1], "empty_behind": [B - 1, 2 * B, 0],
        "three_empty_in_a_row": [3, 0, 0, 0, B + 1, 0, 0, 0], "three_empty_in_front": [0, 0, 0, 2 * B, 1],
        "edges": [1, B - 1, B, B + 1, 2 * B, 1, 2 * B, B + 1, B, B - 1],
        "two_hundred": [int(x) for x in rng.choice([0, 0, 1, 77, B - 1, B, B + 1, 2 * B, 3 * B + 5], 200)],
        "two_hundred_single_bytes": [1] * 200,
    }
    exe = G.build_program()
    for name, s in sizes.items():
        for base in (0, 12345):                                         # (cuts[0] need not be 0)
            cuts = [base + int(x) for x in np.cumsum([0] + s)]
            out = G.run_mode(exe, "blocks", str(tmp_path), np.asarray(cuts, dtype="<u8").tobytes())
            got = [tuple(int(x) for x in ln.split()) for ln in out.splitlines()]
            assert got == [(g, off, n) for g, (off, n) in enumerate(blocks_by_scan(cuts))], name
