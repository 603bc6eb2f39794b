"""The BAM-to-SAM walks at 64 lanes without a GPU ("BAM input"): nanosim_amd/csrc/ns_bam.h compiled for the host on the
lock-step wavefront of tests/wave64_host.h (tests/bam_host.cpp with -DBAM_HOST_LANES=64: 64 host threads, every collective a
rendezvous) behind the signature of ns_bam_to_sam.  With one lane `i = base + lane` never lies past n inside a `base < n` loop, a
round of ops is one op and the bulk fields have one strider, so the `i < n` guards of the *_text loops, the lane striding of bam_bulk
and bam_strlen and the one-writer-per-byte rule of the small fields ran on the GPU alone, never under a sanitizer and never under the
mutation audit.  Here the check_* functions of tests/test_bam.py run on that build, and the stand-alone program of it runs as a child
process under -fsanitize=address,undefined (every record on a copy of exactly its size, every line in a buffer of exactly its length)
and under -fsanitize=thread (no two lanes store to one byte of a line).  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from tests import bam_lib, test_bam as T

ROOT = T.ROOT


@pytest.fixture(scope="module")
def wave():
    return T.build_host(64)


def test_wave64_writer_and_decoder_against_a_record_packed_by_hand(wave, tmp_path):
    T.test_writer_and_decoder_against_a_record_packed_by_hand(wave, tmp_path)
    assert [wave.constant(i) for i in range(6)] == [T.ROUND_OPS, T.LANE_BYTES, T.SLICE_BASES, T.STRLEN_BYTES, T.FLOAT_SLOT, T.FLOAT_CHARS]


def test_wave64_corner_cases(wave):
    T.check_corner_cases(wave)


def test_wave64_sizes_around_the_constants(wave):
    T.check_sized_records(wave)


def test_wave64_batches_with_and_without_floats(wave):
    T.check_floats_many_and_none(wave)


def test_wave64_malformed_records(wave):
    T.check_malformed(wave)


def test_wave64_batches_cut_at_every_byte(wave):
    T.check_batching(wave)


def test_wave64_edges_of_the_rounds(wave):
    assert T.check_edge_cases(wave) > 25
    T.check_no_references(wave)
    T.check_store_guards(wave)


def program(sanitize: str, name: str):
    exe = os.path.join(ROOT, "tests", "_tmp", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-DBAM_HOST_MAIN",
                           "-DBAM_HOST_LANES=64", "-o", exe, os.path.join(ROOT, "tests", "bam_host.cpp")])
    return exe


def run_program(exe, tmp_path, data, final=1):
    p = os.path.join(str(tmp_path), "records.bin")
    with open(p, "wb") as f:
        f.write(data)
    done = subprocess.run([exe, p, str(final)] + [n for n, _ in T.REFS], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-3000:]
    a, b = done.stdout.strip().split("\n")
    return [int(x) for x in a.split()], int(b)


def checksum(text, line_off):
    s = 0
    for c in text:
        s = (s * 31 + c) & (2 ** 64 - 1)
    for o in line_off:
        s = (s * 31 + o) & (2 ** 64 - 1)
    return s


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_wave64_program_is_clean_under_the_sanitizers(tmp_path, sanitize):
    """the stand-alone program of the 64-lane build, started as a child process: every malformed record gives its reason and reads
    nothing outside its copy, the corner cases, the edges of the rounds and about 50 records sized around the constants give their text
    (the number of records, the bytes of text and the checksum of the text and the offsets, from the expected lines)"""
    exe = program(sanitize, "bam_host64_" + sanitize.split(",")[0])
    for name, data, reason, index, offset in T.malformed() + T.edge_malformed():
        assert run_program(exe, tmp_path, data) == ([0, 0, 0, index, offset, reason], 0), name
    cases = T.corner_cases() + T.edge_cases()
    sized = T.sized_sam_text()
    _, _, recs = bam_lib.parse_sam(sized)
    lines = [x.encode() for x in sized.splitlines(True) if not x.startswith("@")]
    pick = [k for k in range(len(recs)) if len(recs[k]) < 3000][::3][:50]
    assert len(pick) == 50
    cases += [(recs[k], lines[k]) for k in pick]
    data, text = b"".join(r for r, _ in cases), b"".join(l for _, l in cases)
    offs = np.cumsum([0] + [len(l) for _, l in cases]).tolist()
    assert run_program(exe, tmp_path, data) == ([len(cases), len(text), len(data), -1, -1, 0], checksum(text, offs))
    assert run_program(exe, tmp_path, data[:-1], 0) == ([len(cases) - 1, offs[-2], len(data) - len(cases[-1][0]), -1, -1, 0], checksum(text[:offs[-2]], offs[:-1]))
    assert run_program(exe, tmp_path, b"") == ([0, 0, 0, -1, -1, 0], 0)
