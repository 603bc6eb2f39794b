"""GPU parity of the cs / MD stage ("cs and MD from the reference"): ns_calmd (the k_calmd_* kernels of csrc/ns_train.h, a
wavefront of 64 lanes per record) against the independent column-by-column writer, the generator's truth and the same walks compiled
for the host with one lane (tests/calmd_host.cpp) — the hand-written cases, the 2 000 generated records, the bad records (which pass the
sanitizer program of tests/test_calmd.py first) —, a sequence of calls on one engine, the Python side, and three stages trained from
input without tags: as SAM text, as BAM and with = / X ops."""
import ctypes as C

import numpy as np
import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as EN
from tests.test_calmd import (REF, bad_cases, build_host, check_bad_records, check_hand_cases, check_random_records, check_tagged_text,
                              check_tagged_text_errors, check_training_from_stripped_input, hand_cases, random_records, seq_bytes, tags)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    h = build_host()
    h.set_reference(REF)
    return h


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0)
    e.set_reference(REF)
    yield e
    e.close()


def same(eng, host, records):
    a = characterize.calmd_raw(eng, [r[0] for r in records], [r[1] for r in records], [r[2] for r in records], [r[3] for r in records])
    b = characterize.calmd_raw(host, [r[0] for r in records], [r[1] for r in records], [r[2] for r in records], [r[3] for r in records])
    for k in ("md", "cs", "n_bad", "first_bad", "bad_reason"):
        assert a[k] == b[k], k
    assert a["md_off"].tolist() == b["md_off"].tolist() and a["cs_off"].tolist() == b["cs_off"].tolist()
    return a


def test_gpu_hand_written_cases(eng, host):
    check_hand_cases(eng)
    same(eng, host, [(c[1], c[2], c[3], c[4]) for c in hand_cases()])


def test_gpu_random_records_three_ways(eng, host):
    check_random_records(eng)
    recs = random_records()["records"]
    r = same(eng, host, [(x["cigar"], x["seq"], x["chrom"], x["pos"]) for x in recs])
    assert r["ms_kernel"] > 0
    print("ms_kernel %.3f for %d records, %d + %d bytes of text" % (r["ms_kernel"], len(recs), len(r["md"]), len(r["cs"])))


def test_gpu_bad_records_as_the_host_build(eng, host):
    check_bad_records(eng)
    cases = bad_cases()
    good = [(c[1], c[2], c[3], c[4]) for c in hand_cases()[:10]]
    mixed = good + [(c[1], seq_bytes(c[2]), c[3], c[4]) for c in cases] + good
    r = same(eng, host, mixed)
    assert (r["n_bad"], r["first_bad"], r["bad_reason"]) == (len(cases), len(good), cases[0][5])
    assert tags(eng, good) == tags(host, good)


def test_gpu_a_sequence_of_calls_with_growing_and_shrinking_n(eng):
    """scratch and result reuse: the same engine, n up and down, n == 0 in between, another training call in between"""
    fx = random_records()
    recs, truth = fx["records"], [(r["md"], r["cs"]) for r in fx["records"]]
    pairs = [("ACGT-ACGTTT", "ACGTAAC-TTT"), ("AAAA", "AAAT")]
    hist = characterize.count_maf(eng, pairs)
    for n in (1, 7, 300, 2000, 300, 0, 65, 2, 1):
        at = (n * 13) % (len(recs) - n + 1)
        assert tags(eng, [(r["cigar"], r["seq"], r["chrom"], r["pos"]) for r in recs[at:at + n]]) == truth[at:at + n], n
        if n == 300:
            assert np.array_equal(characterize.count_maf(eng, pairs)["dic"], hist["dic"])


def test_gpu_no_reference_and_bad_arguments():
    e = EN.Engine(0)
    try:
        with pytest.raises(EN.EngineError, match="no reference set") as err:
            characterize.calmd_raw(e, ["5M"], ["ACGTA"], [0], [1])
        assert err.value.code == EN.NS_EINVAL
        e.set_reference(REF)
        assert characterize.calmd_raw(e, ["5M"], ["ACGTA"], [0], [1])["n_bad"] == 0
        out = characterize.NsCalmdResult()
        cg, cg_off = characterize._pack(["5M"])
        sq, sq_off = characterize._pack(["ACGTA"])
        one, down = np.ones(1, dtype=np.uint32), cg_off[::-1].copy()
        for args in ((cg.ctypes.data, None, sq.ctypes.data, sq_off.ctypes.data, one.ctypes.data, one.ctypes.data),
                     (cg.ctypes.data, cg_off.ctypes.data, sq.ctypes.data, sq_off.ctypes.data, None, one.ctypes.data),
                     (cg.ctypes.data, down.ctypes.data, sq.ctypes.data, sq_off.ctypes.data, one.ctypes.data, one.ctypes.data)):
            assert e.L.ns_calmd(e.ctx, *args, 1, C.addressof(out)) == EN.NS_EINVAL
    finally:
        e.close()


def test_gpu_tagged_text_and_its_errors(eng, tmp_path):
    (tmp_path / "text").mkdir()
    (tmp_path / "errors").mkdir()
    check_tagged_text(eng, tmp_path / "text")
    check_tagged_text_errors(eng, tmp_path / "errors")
    eng.set_reference(REF)


def test_gpu_three_stages_train_from_input_without_tags(eng, tmp_path):
    check_training_from_stripped_input(eng, tmp_path, hist=True)
    eng.set_reference(REF)
