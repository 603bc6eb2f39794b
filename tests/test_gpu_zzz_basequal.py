"""GPU parity of the training side's base-quality model: ns_qual_histograms (k_qual_mark + k_qual_count, csrc/ns_train.h) against what the
REAL src/model_base_qualities.py collected and wrote (tests/golden/reference_basequal.json.gz), against the same walk compiled for the
host and against the per-base expansion of tests/test_basequal.py.  (The file sorts behind every other -m gpu file: these are the
newest kernels of the engine — and for the same reason it runs in a CHILD pytest first, like tests/test_gpu_zz_characterize.py: a
device fault or a hang there fails this file with the child's output, not the whole -m gpu run.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as E
from tests.test_basequal import CORNERS, brute_force, build_host_walk, check_offset_entries, fixture_entries, load_fixture, raw_counts, same_file

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
    if os.environ.get("NS_BQ_CHILD"):
        return
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT,
                           env=dict(os.environ, NS_BQ_CHILD="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    except subprocess.TimeoutExpired as ex:
        pytest.fail("the child run of this file did not finish in 300 s:\n" + str(ex.stdout or "")[-3000:])
    if r.returncode != 0:
        pytest.fail("the child run of this file failed (exit %d):\n%s" % (r.returncode, r.stdout[-4000:]))


@pytest.fixture(scope="module")
def eng(child_ok):
    e = E.Engine(0)
    yield e
    e.close()


def test_gpu_counts_equal_the_reference_and_the_host_walk(fx, eng, host, tmp_path):
    t = characterize.count_qualities(eng, fx["alignments"], fx["unmapped"])
    assert np.array_equal(t["hist"], fx["hist"]) and t["ms_kernel"] > 0
    assert np.array_equal(raw_counts(eng, fixture_entries(fx))[0], raw_counts(host, fixture_entries(fx))[0])
    prefix = str(tmp_path / "training")
    characterize.base_qualities(prefix, fx["alignments"], fx["unmapped"], eng)
    same_file(open(prefix + "_base_qualities_model_parameters.tsv").read(), fx["file"])


def small_shapes(rng):
    """quality strings of 0, 1, 15, 16, 17, 63, 64 and 65 bytes: marks in the first and the last aligned byte, an insertion run across
    16-byte boundaries, clips that leave nothing, clips around the marks, unmapped strings"""
    out = []
    qual = lambda n: "".join(chr(33 + int(v)) for v in rng.integers(0, 94, n))
    for n in (0, 1, 15, 16, 17, 63, 64, 65):
        ends = "" if n == 0 else "*ag" if n == 1 else "*ag:%d*ct" % (n - 2)
        out.append((ends, qual(n), 0, 0, 0))
        out.append((ends, qual(n + 5), 2, 3, 0))
        out.append((":%d" % n, qual(n), n // 2, n - n // 2, 0))                       # head + tail = the whole string
        out.append(("", qual(n), 0, 0, 1))
        if n >= 15:
            out.append((":9+%s:%d" % ("acgt" * 9, n), qual(n), 0, 0, 0))              # cut inside the insertion (n < 45) or behind it
            out.append(("+%s" % ("a" * n), qual(n + 1), 1, 0, 0))
    return out


def test_gpu_small_shapes_back_to_back(eng, host):
    rng = np.random.default_rng(21)
    shapes = small_shapes(rng)
    assert len(shapes) <= 64                                                          # index order; the longer lists below are sorted by length
    for entries in (shapes, [shapes[i] for i in rng.permutation(len(shapes))], [shapes[i] for i in rng.integers(0, len(shapes), 300)],
                    [shapes[0]], [shapes[3]] * 3, [shapes[-1]]):
        got = raw_counts(eng, entries)
        exp, exp_short = brute_force(entries)
        assert got[1] == exp_short == 0 and got[2] == 0
        assert np.array_equal(got[0], exp)
        assert np.array_equal(got[0], raw_counts(host, entries)[0])


def test_gpu_corners_and_cs_strings_at_every_offset_and_length(eng):
    """the per-base expansion on the device for the corners of tests/test_basequal.py (items left over exactly at the aligned length among
    them: a mark taken there would land on the next alignment's first base) and for cs strings at every offset mod 8 and every length
    0 .. 17 of the packed bytes (CsBytes reads them through aligned 8-byte windows)"""
    rng = np.random.default_rng(11)
    corners = [(cs, "".join(chr(33 + int(v)) for v in rng.integers(1, 94, n)), 0, 0, 0) for cs, n in CORNERS]
    corners += [(cs, "".join(chr(33 + int(v)) for v in rng.integers(1, 94, 3 + n + 2)), 3, 2, 0) for cs, n in CORNERS]
    for entries in (corners, [e for e in corners if e[1]][::-1]):
        got = raw_counts(eng, entries)
        exp, exp_short = brute_force(entries)
        assert got[1] == exp_short and got[2] == 0 and np.array_equal(got[0], exp)
    check_offset_entries(eng)


def test_gpu_short_cs_bad_bytes_and_no_alignments(eng, host):
    entries = [(":20", "I" * 20, 0, 0, 0), (":4*ag:4", "5" * 13, 2, 1, 0), ("", "+" * 7, 0, 0, 1)]        # the 2nd covers 9 of 10 aligned bases
    assert raw_counts(eng, entries)[1] == 1
    with pytest.raises(ValueError, match="fewer query bases"):
        characterize.count_qualities(eng, [e[:4] for e in entries[:2]])
    entries = [(":3", "I I", 0, 0, 0), ("", "\x1f!~\x7f", 0, 0, 1), (":2", "II", 0, 0, 0)]                # a byte below '!', one above '~'
    got = raw_counts(eng, entries)
    assert got[2] == 3 and got[1] == 0 and np.array_equal(got[0], raw_counts(host, entries)[0]) and got[0].sum() == 6
    with pytest.raises(ValueError, match="outside"):
        characterize.count_qualities(eng, [(":3", "I I", 0, 0)])
    t = characterize.count_qualities(eng, [])
    assert t["hist"].shape == (5, 94) and t["hist"].sum() == 0 and t["ms_kernel"] == 0


def test_gpu_argument_checks(eng):
    h = characterize.NsQualHist()
    cs = np.frombuffer(b":4\0", dtype=np.uint8)
    q = np.frombuffer(b"IIII\0", dtype=np.uint8)
    cs_off = np.array([0, 2], dtype=np.uint64)
    q_off = np.array([0, 4], dtype=np.uint64)
    aln = np.zeros(1, dtype=characterize.QUAL_ALN_DTYPE)

    def call(cs_p=cs.ctypes.data, cs_n=2, cs_o=cs_off, q_p=q.ctypes.data, q_n=4, q_o=q_off, a=aln, out=C.byref(h)):
        return eng.L.ns_qual_histograms(eng.ctx, cs_p, cs_n, cs_o.ctypes.data if cs_o is not None else None, q_p, q_n,
                                        q_o.ctypes.data if q_o is not None else None, a.ctypes.data if a is not None else None, 1, out)
    assert call() == 0 and h.hist[2][ord("I") - 33] == 4
    for kw in (dict(out=None), dict(cs_o=None), dict(q_o=None), dict(a=None), dict(cs_p=None), dict(q_p=None),
               dict(q_o=np.array([3, 2], dtype=np.uint64)), dict(q_o=np.array([0, 5], dtype=np.uint64)), dict(cs_o=np.array([0, 3], dtype=np.uint64)),
               dict(a=np.array([(3, 2, 0, 0)], dtype=characterize.QUAL_ALN_DTYPE))):
        assert call(**kw) == E.NS_EINVAL, kw
        assert b"ns_qual_histograms" in eng.L.ns_last_error(eng.ctx)
    assert call(a=np.array([(2, 2, 0, 0)], dtype=characterize.QUAL_ALN_DTYPE)) == 0 and h.hist[3][ord("I") - 33] == 4


def test_gpu_many_alignments_several_workgroups(fx, eng):
    """the fixture 20 times, shuffled: ~10 MB of qualities — several workgroups per kernel, several tiles per workgroup, the flush"""
    entries = fixture_entries(fx)
    rng = np.random.default_rng(5)
    many = [entries[i] for _ in range(20) for i in rng.permutation(len(entries))]
    hist, n_short, n_bad = raw_counts(eng, many)
    assert n_short == 0 and n_bad == 0
    assert np.array_equal(hist, 20 * fx["hist"])
