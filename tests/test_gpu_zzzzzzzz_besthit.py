"""GPU parity of the training side's MAF input ("MAF input: the best hit per read"): ns_maf_besthit (the k_maf_* kernels of
csrc/ns_train.h) against what the REAL src/get_besthit_maf.py wrote and returned (tests/golden/reference_besthit.json.gz), on the raw
file, on its `s` lines alone and at sizes around the span of the line kernels; twice on one engine and between other training calls;
on a synthetic file of 70 000 pairs against a restatement of G:14-39 written out here; and a genome prefix trained end to end."""
import numpy as np
import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as EN
from tests.test_besthit import (check_carriage_returns, check_fixture, check_tiny, check_training, check_value_errors, load_fixture, raw)

pytestmark = pytest.mark.gpu
SPAN = 16384                        # MAF_LINE_SPAN (tests/test_besthit.py checks the number against the header)


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0)
    yield e
    e.close()


def test_gpu_fixture_equals_the_reference(fx, eng, tmp_path):
    got = check_fixture(eng, fx, tmp_path)
    assert got["ms_kernel"] > 0
    print("ms_kernel %.3f" % got["ms_kernel"])


def test_gpu_lines_only_and_sizes_around_the_span(fx, eng, tmp_path):
    maf = fx["maf"]
    check_fixture(eng, fx, tmp_path, "".join(x for x in maf.splitlines(True) if x.startswith("s ") or x.startswith("s\t")))
    start = maf.index("\ns ", 20 * SPAN) + 1
    for pad in [(d - len(maf)) % SPAN + SPAN for d in (-1, 0, 1)] + [(d - start) % SPAN + SPAN for d in (0, 1, SPAN - 1)]:
        check_fixture(eng, fx, tmp_path, "#" + "x" * (pad - 2) + "\n" + maf)


def test_gpu_tiny_tables_empty_input_carriage_returns_and_value_errors(eng, tmp_path):
    check_tiny(eng)
    check_carriage_returns(eng, tmp_path)
    check_value_errors(eng, tmp_path)


def test_gpu_twice_on_one_engine_and_between_other_calls(fx, eng):
    """scratch reuse: the same call after itself, after a smaller one and after count_maf gives the same arrays"""
    names = [b"hot", b"never000", b"chrOnlyRef", b"read1", b"read1y"]
    first, counts = raw(eng, fx["maf"], names)
    pairs = [(fx["maf"][a:a + n], fx["maf"][b:b + n]) for _, a, b, _, n, _, _ in first["records"].tolist()[:200]]
    hist = characterize.count_maf(eng, pairs)
    small, _ = raw(eng, "s ref 5 4 + 100 ACGT\ns only 0 4 + 4 ACGT\n", [b"only"])
    assert small["found"].tolist() == [True]
    for _ in range(2):
        again, counts2 = raw(eng, fx["maf"], names)
        assert counts2 == counts == (2 * fx["n_pairs"], fx["n_pairs"], fx["n_names"], 794)
        for k in ("lines", "records", "figure_rows", "found"):
            assert np.array_equal(again[k], first[k]), k
        assert again["found"].tolist() == [True, False, False, True, False]
        assert np.array_equal(characterize.count_maf(eng, pairs)["dic"], hist["dic"])


def test_gpu_seventy_thousand_pairs_equal_the_restated_choice(eng):
    """70 000 pairs over 20 000 names (274 workgroups of pairs, a table of 2^18 slots, about 70 spans of text), sizes from a small
    range so that most names have ties; against G:14-39 restated"""
    rng = np.random.default_rng(20261020)
    n = 70000
    name_id = rng.integers(0, 20000, n)
    size = rng.integers(0, 40, n)
    strand = rng.integers(0, 2, n)
    parts = []
    for i in range(n):
        parts.append("s c%d %d 3 + 999 ACG\ns q%x %d %d %s 50 ACG\n" % (i % 7, i, int(name_id[i]), i % 5, int(size[i]), "+-"[int(strand[i])]))
    text = "".join(parts)
    # G:14-39: the largest size per name, replaced on strictly greater only; then the first pair that has it
    best = {}
    for i in range(n):
        if name_id[i] not in best or best[name_id[i]] < size[i]:
            best[name_id[i]] = size[i]
    kept, done, pos = [], set(), 0
    for i in range(n):
        if best[name_id[i]] == size[i] and name_id[i] not in done:
            done.add(name_id[i])
            kept.append(i)
            pos += int(strand[i] == 0)
    r, counts = raw(eng, text, [b"q0", b"q4e1f", b"q4e20", b"c1", b"q"])
    assert counts == (2 * n, n, len(kept), pos)
    off = np.cumsum([0] + [len(p) for p in parts])
    assert r["lines"]["ref_begin"].tolist() == off[kept].tolist() and r["lines"]["qry_end"].tolist() == off[np.array(kept) + 1].tolist()
    assert r["records"]["ref_start"].tolist() == kept and r["figure_rows"]["ht"].tolist() == [50 - int(size[i]) for i in kept]
    ids = set(name_id.tolist())
    assert r["found"].tolist() == [0 in ids, 0x4e1f in ids, False, False, False]
    print("ms_kernel %.3f for %d pairs, %d bytes" % (r["raw"].ms_kernel, n, len(text)))


def test_gpu_a_prefix_trains_from_a_maf_file_and_opens(fx, eng, tmp_path):
    check_training(eng, fx, tmp_path)
