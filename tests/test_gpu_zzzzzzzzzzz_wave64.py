"""GPU parity of the cross-lane cases of the two walks that are written against an abstract wavefront ("cs and MD from the
reference" and "BAM input"): ns_calmd and ns_bam_to_sam on the records tests/test_calmd.py and tests/test_bam.py add for the rounds of
64 CIGAR bytes, the steps of 64 columns, the clip order across rounds, two errors in one CIGAR, the 2^31 sums, the neighbour's first
byte, and the guards of the op, element and NUL-search rounds — against the Python references first (write_tags, bad_reason, the
expected SAM lines), and against the same walks on the host at 64 lanes in lock step second (tests/wave64_host.h).  Short records
only; nothing here is compiled for the GPU."""
import time

import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as EN
from tests import test_bam as B
from tests import test_calmd as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0)
    e.set_reference(T.REF)
    yield e
    e.close()


@pytest.fixture(scope="module")
def wave_calmd():
    h = T.build_host(64)
    h.set_reference(T.REF)
    return h


@pytest.fixture(scope="module")
def wave_bam():
    return B.build_host(64)


def same_tags(eng, host, records):
    a = characterize.calmd_raw(eng, [r[0] for r in records], [r[1] for r in records], [r[2] for r in records], [r[3] for r in records])
    b = characterize.calmd_raw(host, [r[0] for r in records], [r[1] for r in records], [r[2] for r in records], [r[3] for r in records])
    for k in ("md", "cs", "n_bad", "first_bad", "bad_reason"):
        assert a[k] == b[k], k
    assert a["md_off"].tolist() == b["md_off"].tolist() and a["cs_off"].tolist() == b["cs_off"].tolist()
    return a


def same_lines(a, b):
    for k in ("text", "line_off", "n", "consumed", "first_bad", "first_bad_offset", "reason"):
        assert a[k] == b[k], k


def test_gpu_calmd_cross_lane_cases(eng, wave_calmd):
    t0 = time.time()
    assert T.check_wave_cases(eng) > 90
    print("check_wave_cases on the GPU: %.2f s" % (time.time() - t0))
    same_tags(eng, wave_calmd, [(c[1], T.seq_bytes(c[2]), c[3], c[4]) for c in T.wave_cases()])


def test_gpu_calmd_the_neighbour_first_byte(eng):
    T.check_neighbours(eng)


def test_gpu_calmd_corrupted_records_in_one_call(eng, wave_calmd):
    t0 = time.time()
    fx = T.check_corrupted_records(eng, alone=10)
    print("check_corrupted_records on the GPU: %.2f s" % (time.time() - t0))
    r = same_tags(eng, wave_calmd, [(x["cigar"], x["seq"], x["chrom"], x["pos"]) for x in fx["records"]])
    assert r["ms_kernel"] > 0
    print("ms_kernel %.3f for %d corrupted records" % (r["ms_kernel"], len(fx["records"])))


def test_gpu_bam_edges_of_the_rounds(eng, wave_bam):
    t0 = time.time()
    assert B.check_edge_cases(eng) > 25
    print("check_edge_cases on the GPU: %.2f s" % (time.time() - t0))
    data = b"".join(r for r, _ in B.edge_cases())
    same_lines(B.raw(eng, data), B.raw(wave_bam, data))
    for name, data, reason, index, offset in B.edge_malformed():
        same_lines(B.raw(eng, data), B.raw(wave_bam, data))
    B.check_no_references(eng)
    data = b"".join(r for r, _ in B.corner_cases())                  # ... and a good file afterwards
    same_lines(B.raw(eng, data), B.raw(wave_bam, data))
