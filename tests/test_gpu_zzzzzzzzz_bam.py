"""GPU parity of the training side's BAM input ("BAM input"): ns_bam_to_sam (the k_bam_* kernels of csrc/ns_train.h) against
the same walks compiled for the host with one lane (tests/bam_host.cpp) and against the expected lines of tests/test_bam.py: the
project's SAM texts, the corner cases, records sized around every constant of ns_bam.h at every offset modulo 16, batches with and
without floats, the call repeated and between other training calls, the malformed records (which pass the sanitizer program of
tests/test_bam.py first), and a genome prefix trained once from SAM text and once from the BAM file of the same records."""
import gzip
import json
import os

import numpy as np
import pytest

from nanosim_amd import characterize, model
from nanosim_amd import engine as EN
from tests import bam_lib
from tests.test_bam import (build_host, check_batching, check_corner_cases, check_floats_many_and_none, check_malformed, check_project_texts,
                            check_sized_records, check_stage_equality, corner_cases, malformed, raw, sized_sam_text, write_bam)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    return build_host()


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0)
    yield e
    e.close()


def same(a, b):
    for k in ("text", "line_off", "n", "consumed", "first_bad", "first_bad_offset", "reason"):
        assert a[k] == b[k], k


def test_gpu_project_texts_and_every_reader(eng, host, tmp_path):
    done = check_project_texts(eng, tmp_path)
    for name, (text, path) in done.items():                          # text and line_off == the host build's
        _, _, recs = bam_lib.parse_sam(text)
        data = b"".join(recs)
        got = raw(eng, data)
        same(got, raw(host, data))
        assert got["ms_kernel"] > 0
    check_stage_equality(eng, tmp_path)


def test_gpu_corner_cases_and_batches_cut_at_every_byte(eng, host):
    check_corner_cases(eng)
    check_batching(eng)
    data = b"".join(r for r, _ in corner_cases())
    same(raw(eng, data), raw(host, data))


def test_gpu_sizes_around_the_constants_at_every_offset(eng, host):
    text = check_sized_records(eng)
    _, _, recs = bam_lib.parse_sam(sized_sam_text())
    data = b"".join(recs)
    got = raw(eng, data)
    same(got, raw(host, data))
    assert got["text"] == text
    print("ms_kernel %.3f for %d records, %d bytes of text" % (got["ms_kernel"], got["n"], len(text)))


def test_gpu_batches_with_and_without_floats(eng):
    check_floats_many_and_none(eng)


def test_gpu_twice_on_one_engine_and_between_other_calls(eng, host):
    """scratch and result reuse: the same call after itself, after a smaller one and between count_maf and ns_maf_besthit calls"""
    data = b"".join(r for r, _ in corner_cases()) * 3
    want = raw(host, data)
    first = raw(eng, data)
    same(first, want)
    pairs = [("ACGT-ACGTTT", "ACGTAAC-TTT"), ("AAAA", "AAAT")]
    hist = characterize.count_maf(eng, pairs)
    maf = np.frombuffer(b"s ref 5 4 + 100 ACGT\ns only 0 4 + 4 ACGT\n", dtype=np.uint8)
    best = characterize.besthit_call(eng, maf, [b"only"])
    small = raw(eng, corner_cases()[0][0])
    assert small["text"] == corner_cases()[0][1]
    for _ in range(2):
        same(raw(eng, data), want)
        assert np.array_equal(characterize.count_maf(eng, pairs)["dic"], hist["dic"])
        again = characterize.besthit_call(eng, maf, [b"only"])
        assert again["found"].tolist() == best["found"].tolist() == [True] and np.array_equal(again["lines"], best["lines"])


def test_gpu_malformed_records_as_the_host_build_and_a_good_file_afterwards(eng, host):
    check_malformed(eng)
    for name, data, reason, index, offset in malformed():
        same(raw(eng, data), raw(host, data))
    data = b"".join(r for r, _ in corner_cases())
    same(raw(eng, data), raw(host, data))


def test_gpu_a_prefix_trains_from_bam_as_from_sam(eng, tmp_path):
    """the genome prefix of test_gpu_zzzz_read_lengths' end-to-end case, once from the SAM files and once from read_bam of the same
    records: every file the two runs write is equal byte for byte, and model.load_model opens the second"""
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_read_len.json.gz"), "rt") as f:
        fx = json.load(f)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_hist.json.gz"), "rt") as f:
        cs = json.load(f)["cs"]
    refs, recs, _, _ = characterize.primary_and_unaligned(_written(tmp_path, "all.sam", fx["sam"]))
    primary = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "".join(
        "%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t*\t*\tcs:Z:%s\n" % (tuple(r) + (cs[i % len(cs)],)) for i, r in enumerate(recs))
    sources = {"sam": (_written(tmp_path, "training.sam", fx["sam"]), _written(tmp_path, "training_primary.sam", primary)),
               "bam": (characterize.read_bam(write_bam(tmp_path, "training.bam", fx["sam"]), eng),
                       characterize.read_bam(write_bam(tmp_path, "training_primary.bam", primary), eng))}
    files = {}
    for kind, (all_records, primary_records) in sources.items():
        os.makedirs(str(tmp_path / kind))
        prefix = str(tmp_path / kind / "training")
        refs, recs, unaligned_len, strandness = characterize.primary_and_unaligned(all_records)
        assert recs == [tuple(r) for r in fx["primary"]]
        characterize.hist(prefix, characterize.cs_from_sam(primary_records), eng)
        characterize.model_fitting(prefix, eng)
        characterize.read_lengths(prefix, refs, recs, eng, unaligned_len, strandness)
        files[kind] = {n: open(os.path.join(str(tmp_path / kind), n), "rb").read() for n in sorted(os.listdir(str(tmp_path / kind)))}
    assert sorted(files["sam"]) == sorted(files["bam"]) and len(files["sam"]) >= 8
    for n in files["sam"]:
        assert files["sam"][n] == files["bam"][n], n
    m = model.load_model(str(tmp_path / "bam" / "training"))
    assert m.strandness_rate == round(fx["strandness"], 3)


def _written(tmp_path, name, text):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    return path
