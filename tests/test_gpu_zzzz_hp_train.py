"""GPU parity of the training side's homopolymer-length model: ns_hp_histograms (k_hp_count + k_hp_records, csrc/ns_train.h) against what the
REAL src/model_homopolymer_lengths.py collected and wrote (tests/golden/reference_hp_train.json.gz) and against the same walk compiled
for the host.  (The file sorts behind every other -m gpu file: these are the newest kernels of the engine — and for the same reason it
runs in a CHILD pytest first, like tests/test_gpu_zzz_basequal.py: a device fault or a hang there fails this file with the child's
output, not the whole -m gpu run.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as E
from tests.test_hp_train import KS, build_host_walk, expected_columns, expected_table, load_fixture, spans_of, write_files

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


@pytest.fixture(scope="module")
def child_ok():
    if os.environ.get("NS_HP_CHILD"):
        return
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT,
                           env=dict(os.environ, NS_HP_CHILD="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    except subprocess.TimeoutExpired as ex:
        pytest.fail("the child run of this file did not finish in 300 s:\n" + str(ex.stdout or "")[-3000:])
    if r.returncode != 0:
        pytest.fail("the child run of this file failed (exit %d):\n%s" % (r.returncode, r.stdout[-4000:]))


@pytest.fixture(scope="module")
def eng(child_ok):
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host_counts(fx, host):
    """the host walk's result per k, computed once"""
    return {k: characterize.count_homopolymers(host, fx["records"], k, records=True) for k in KS}


def same(a, b):
    return (a["table"].shape == b["table"].shape and np.array_equal(a["table"], b["table"]) and np.array_equal(a["columns"], b["columns"])
            and a["n_hp"] == b["n_hp"] and np.array_equal(a["records"], b["records"]))


@pytest.mark.parametrize("k", KS)
def test_gpu_counts_equal_the_reference_and_the_host_walk(fx, eng, host_counts, k):
    """414 alignments: the order by length, two workgroups, the LDS corner, the global table beyond it and beyond the first caps"""
    assert len(fx["records"]) > 256 + 64
    t = characterize.count_homopolymers(eng, fx["records"], k, records=True)
    assert np.array_equal(t["table"], expected_table(fx, k)) and t["columns"].tolist() == expected_columns(fx, k) and t["ms_kernel"] > 0
    assert spans_of(fx, t["records"]) == fx["k"][str(k)]["spans"]
    assert same(t, host_counts[k])


@pytest.mark.parametrize("k", KS)
def test_gpu_first_40_alignments_in_index_order(fx, eng, host, k):
    some = fx["records"][:40]
    assert same(characterize.count_homopolymers(eng, some, k, records=True), characterize.count_homopolymers(host, some, k, records=True))


def raw_call(eng, fx, k, cap_ref, cap_read, cap_records):
    rb = np.frombuffer(b"".join(r[2].encode() for r in fx["records"]) + b"\0", dtype=np.uint8)
    qb = np.frombuffer(b"".join(r[3].encode() for r in fx["records"]) + b"\0", dtype=np.uint8)
    off = np.cumsum([0] + [len(r[2]) for r in fx["records"]]).astype(np.uint64)
    h = characterize.NsHpHist()
    table = np.full((2, cap_ref, cap_read), 7, dtype=np.uint64)
    rec = np.zeros(max(cap_records, 1), dtype=characterize.HP_RECORD_DTYPE)
    h.cap_ref, h.cap_read, h.table, h.records, h.cap_records = cap_ref, cap_read, table.ctypes.data, rec.ctypes.data, cap_records
    rc = eng.L.ns_hp_histograms(eng.ctx, rb.ctypes.data, qb.ctypes.data, int(off[-1]), off.ctypes.data, len(off) - 1, k, C.byref(h))
    return rc, h, table, rec


def test_gpu_small_caps_report_the_overflow_and_the_retry_gives_the_same(fx, eng, host_counts):
    full = host_counts[3]
    rc, h, table, rec = raw_call(eng, fx, 3, 5, 7, 100)
    assert rc == 0 and np.array_equal(table, full["table"][:, :5, :7])
    assert h.n_overflow == int(full["table"].sum() - full["table"][:, :5, :7].sum()) > 0
    assert (h.max_ref, h.max_read, h.n_hp) == (full["table"].shape[1] - 1, full["table"].shape[2] - 1, full["n_hp"])
    assert h.columns[:] == full["columns"].tolist()
    assert not rec.view(np.uint32).any()                                      # more homopolymers than cap_records: none is written
    rc, h, table, rec = raw_call(eng, fx, 3, 100, 100, full["n_hp"])          # inside the corner's caps no longer, records: exactly enough
    assert rc == 0 and h.n_overflow == 1 and np.array_equal(table, full["table"][:, :100, :100])
    assert np.array_equal(rec["start"], full["records"][:, 1]) and np.array_equal(rec["read_base"] >> 2, full["records"][:, 3])
    t = characterize.count_homopolymers(eng, fx["records"], 3, records=True, cap_ref=2, cap_read=3, cap_records=5)
    assert same(t, full)


def test_gpu_writes_both_files(fx, eng, host, tmp_path):
    for k in (5, 1):
        params, lengths = write_files(eng, fx, k, tmp_path, "gpu%d" % k)
        assert lengths == fx["k"][str(k)]["lengths_file"]
        assert params == write_files(host, fx, k, tmp_path, "host%d" % k)[0]


def test_gpu_no_alignments_empty_lines_and_argument_checks(eng):
    for pairs in ([], [("", "")] * 3, [("", "")] * 70):
        t = characterize.count_homopolymers(eng, pairs, 5, records=True)
        assert t["table"].shape == (2, 1, 1) and not t["table"].any() and not t["columns"].any() and t["n_hp"] == 0 and t["records"].shape == (0, 5)
    h = characterize.NsHpHist()
    table = np.zeros((2, 8, 8), dtype=np.uint64)
    h.cap_ref, h.cap_read, h.table = 8, 8, table.ctypes.data
    ref = np.frombuffer(b"AAAAA\0", dtype=np.uint8)
    off = np.array([0, 5], dtype=np.uint64)

    def call(r=ref.ctypes.data, q=ref.ctypes.data, n=5, o=off, k=5, out=C.byref(h)):
        return eng.L.ns_hp_histograms(eng.ctx, r, q, n, o.ctypes.data if o is not None else None, 1, k, out)
    assert call() == 0 and table[0, 5, 5] == 1 and table.sum() == 1 and h.columns[:] == [0, 0, 0, 5]
    for kw in (dict(out=None), dict(o=None), dict(r=None), dict(q=None), dict(k=0), dict(o=np.array([3, 2], dtype=np.uint64)),
               dict(o=np.array([0, 6], dtype=np.uint64))):
        assert call(**kw) == E.NS_EINVAL, kw
        assert b"ns_hp_histograms" in eng.L.ns_last_error(eng.ctx)
    h.cap_ref = 0
    assert call() == E.NS_EINVAL
    h.cap_ref, h.table = 8, None
    assert call() == E.NS_EINVAL
