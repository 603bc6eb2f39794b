"""The block walk of the compressed output at 64 lanes without a GPU ("BGZF output"): nanosim_amd/csrc/ns_gz.h compiled for
the host on the lock-step wavefront of tests/wave64_host.h (tests/gz_wave_host.cpp: 64 host threads, every collective a rendezvous).  The
stand-alone program writes whole members; it runs as a child process, built plain, under -fsanitize=address,undefined (the input in a
buffer of exactly its size at byte 0, 1 and 15 of a 16-aligned allocation, the members in a buffer of exactly their sum) and under
-fsanitize=thread (every word of the staging image and every byte of a member is stored by one lane; what another lane wrote is read
behind the fence only).  Nothing is loaded into Python under a sanitizer.

Every output must gunzip to its input, and the BGZF walk of characterize/bam.py must accept every member."""
import numpy as np
import pytest

from tests import gz_lib as G

JOBS = [(kind, n, start) for kind in G.KINDS for n in G.LENGTHS for start in G.STARTS]


def run_all(exe, tmp_path):
    inputs = {(kind, n): G.make_input(kind, n) for kind in G.KINDS for n in G.LENGTHS}
    got = G.run_program(exe, str(tmp_path), [inputs[kind, n] + (start,) for kind, n, start in JOBS])
    first = {}
    for (kind, n, start), (members, blocks) in zip(JOBS, got):
        data = inputs[kind, n][0]
        where = "%s, %d bytes at %d" % (kind, n, start)
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
