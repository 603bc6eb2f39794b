"""GPU parity of the index of a SAM text ("SAM text: one indexed pass and the CLI"): ns_sam_index (the k_sam_sep_*, k_sam_tags
and k_sam_rows kernels of csrc/ns_train.h) against the restatement of tests/test_sam_index.py on the project's texts, on the hand-written
text and at the borders of the spans; near misses of the four prefixes, records that end with their FLAG or POS, texts of nothing but
separators at the sizes of a chunk, a wavefront's load, a load and a span, two separators at every pair of seams (what the ranking of
k_sam_sep_count / k_sam_sep_write, which has no host build, is decided by); characterize.SamTable's readers against the path readers, returns and ValueErrors; twice on one
engine and between other training calls; and a synthetic text of 20 000 records against the restatement and the path readers.  Every
malformed input here is one the call answers with a status or a bit."""
import os

import numpy as np
import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as EN
from tests import test_besthit
from tests.test_sam_index import (HAND, as_bytes, check_arrays, check_boundaries, check_dense, check_errors, check_near_prefixes, check_readers, check_rows,
                                  check_same_outcome, check_seam_pairs, check_short_records, check_tag_dense, check_texts, composed_texts, restate)

pytestmark = pytest.mark.gpu
SPAN = 16384                        # SAM_SPAN (tests/test_sam_index.py checks the number against the header)


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0)
    yield e
    e.close()


def test_gpu_rows_equal_the_restatement(eng):
    check_texts(eng)
    r = characterize.sam_index_call(eng, as_bytes(composed_texts()[0]))
    assert r["raw"].ms_kernel > 0
    print("ms_kernel %.3f" % r["raw"].ms_kernel)


def test_gpu_sizes_and_separators_at_the_borders_of_the_spans(eng):
    check_boundaries(eng, SPAN)


def test_gpu_a_near_miss_of_a_prefix_is_no_tag(eng, tmp_path):
    check_near_prefixes(eng, tmp_path)


def test_gpu_records_that_end_with_their_flag_or_their_pos(eng):
    check_short_records(eng)


def test_gpu_texts_of_nothing_but_separators(eng):
    check_dense(eng, SPAN)
    r = characterize.sam_index_call(eng, np.full(2 * SPAN + 1, 10, dtype=np.uint8))
    assert int(r["raw"].n_records) == 2 * SPAN + 1
    print("ms_kernel %.3f for %d bytes, all of them line ends" % (r["raw"].ms_kernel, 2 * SPAN + 1))


def test_gpu_tag_dense_lines_at_every_chunk_offset(eng):
    check_tag_dense(eng, SPAN)


def test_gpu_two_separators_at_every_pair_of_seams(eng):
    assert check_seam_pairs(eng, SPAN) == 1860


def test_gpu_the_spare_bytes_behind_the_text_are_no_text(eng):
    """the last chunk's load reaches into the 16 spare bytes behind the text, which no copy writes: a text that ends 1 .. 15 bytes into a
    chunk, each indexed directly behind a call whose text was line ends up to and beyond that place, is one record of one field.  Best
    effort: whether the allocator hands the second call the memory of the first is its own business, and nothing here asserts that it
    did; the host build decides the same thing with bytes it fills in itself (tests/sam_index_host.cpp)."""
    L = SPAN + 32
    line_ends = np.full(L, 10, dtype=np.uint8)
    assert int(characterize.sam_index_call(eng, line_ends)["raw"].n_records) == L
    for k in range(1, 16):
        assert int(characterize.sam_index_call(eng, line_ends)["raw"].n_records) == L
        r = check_arrays(eng, b"x" * (L - k), "%d bytes behind %d line ends" % (L - k, L))
        assert len(r["rows"]) == 1 and len(r["header"]) == 0 and int(r["raw"].n_odd) == 0
        assert (int(r["rows"][0]["n_fields"]), int(r["rows"][0]["begin"]), int(r["rows"][0]["end"])) == (1, 0, L - k)


def test_gpu_every_table_reader_equals_its_path_reader(eng, tmp_path):
    check_readers(eng, tmp_path)


def test_gpu_every_value_error_of_the_path_readers_and_the_texts_turned_away(eng, tmp_path):
    check_errors(eng, tmp_path)


def test_gpu_twice_on_one_engine_and_between_other_calls(eng):
    """scratch reuse: the same call after itself, after a smaller text and between count_maf and ns_maf_besthit gives the same arrays"""
    fx = test_besthit.load_fixture()
    chim, pairs = composed_texts()
    big = as_bytes(pairs + chim[chim.index("\n", chim.rindex("\n@")) + 1:])
    first = characterize.sam_index_call(eng, big)
    maf, counts = test_besthit.raw(eng, fx["maf"], [b"hot"])
    hist = characterize.count_maf(eng, [(fx["maf"][a:a + n], fx["maf"][b:b + n]) for _, a, b, _, n, _, _ in maf["records"].tolist()[:200]])
    small = characterize.sam_index_call(eng, as_bytes(HAND))
    for _ in range(2):
        again = characterize.sam_index_call(eng, big)
        for k in ("rows", "header"):
            assert again[k].tobytes() == first[k].tobytes(), k
        assert [int(getattr(again["raw"], k)) for k in ("n_records", "n_header", "n_odd", "n_cs", "n_md")] == \
            [int(getattr(first["raw"], k)) for k in ("n_records", "n_header", "n_odd", "n_cs", "n_md")]
        assert test_besthit.raw(eng, fx["maf"], [b"hot"])[1] == counts
        assert characterize.sam_index_call(eng, as_bytes(HAND))["rows"].tobytes() == small["rows"].tobytes()
        assert np.array_equal(characterize.count_maf(eng, [(fx["maf"][a:a + n], fx["maf"][b:b + n]) for _, a, b, _, n, _, _ in maf["records"].tolist()[:200]])["dic"],
                              hist["dic"])


def synthetic(n: int = 20000, seed: int = 20261021) -> str:
    """n records under a header, header lines in between: SEQ / QUAL of 0 (`*`) .. 3 SPAN bytes (most of them short, one in a hundred
    long: the text stays at some 20 MB), 0-6 other tags in random order around the four that are looked for, each of which is absent,
    present or given twice on the unmapped records; a mapped record has cs, MD and NM once or twice, so that the readers return"""
    rng = np.random.default_rng(seed)
    refs = ["chr%d" % k for k in range(1, 6)]
    out = ["@HD\tVN:1.6\n"] + ["@SQ\tSN:%s\tLN:100000000\n" % r for r in refs]
    kind = rng.integers(0, 100, n)
    length = np.where(kind < 90, rng.integers(2, 200, n), np.where(kind < 99, rng.integers(200, SPAN // 4, n), rng.integers(SPAN // 4, 3 * SPAN + 1, n)))
    length[rng.integers(0, n, 8)] = 3 * SPAN
    flags = rng.choice([0, 16, 4, 256, 2048, 2064], n, p=[0.35, 0.35, 0.1, 0.07, 0.07, 0.06])
    flags[0] = 0
    others = ["AS:i:%d", "ms:i:%d", "nn:i:%d", "tp:Z:P%d","de:f:0.01%d", "rl:i:%d", "cm:i:%d", "s1:i:%d", "XS:Z:cs:Z:%d", "ZZ:Z:%d"]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(n):
        flag, ln = int(flags[i]), int(length[i])
        if flag in (4, 256) and i % 3 == 0:
            ln = 0
        seq = letters[rng.integers(0, 4, ln)].tobytes().decode() if ln else "*"
        qual = (rng.integers(33, 127, ln).astype(np.uint8).tobytes().decode()) if ln else "*"
        times = rng.integers(0, 3, 4) if flag == 4 else np.concatenate([rng.integers(1, 3, 3), rng.integers(0, 3, 1)])
        tags = [others[k] % i for k in rng.choice(len(others), int(rng.integers(0, 7)), replace=False)]
        for g, t in enumerate(times.tolist()):
            for d in range(t):
                tags.append(("cs:Z::%d" % (ln or 10), "MD:Z:%d" % (ln or 10), "NM:i:%d" % (i % 50 + d), "SA:Z:chr2,%d,+,5S%dM,60,%d;" % (i + 1, ln or 10, d))[g])
        tags = [tags[k] for k in rng.permutation(len(tags))]
        cigar = "*" if flag == 4 else "%dM" % (ln or 10)
        out.append("\t".join(["read%d" % i, str(flag), "*" if flag == 4 else refs[i % 5], str(0 if flag == 4 else i + 1), "60", cigar, "*", "0", "0", seq, qual] + tags) + "\n")
        if i % 997 == 5:
            out.append("@CO\tcomment %d\tcs:Z:no\n" % i)
    return "".join(out)


def test_gpu_twenty_thousand_records_equal_the_restatement_and_the_path_readers(eng, tmp_path):
    text = synthetic()
    r = check_rows(eng, text)
    rows, header = restate(text)
    assert len(rows) == 20000 and len(header) > 20 and max(x[4][9] - x[4][8] - 1 for x in rows) == 3 * SPAN
    assert {x[3] >> 4 for x in rows} == set(range(16)) and len(text) > 100 * SPAN
    path = os.path.join(str(tmp_path), "synthetic.sam")
    with open(path, "w") as f:
        f.write(text)
    table = characterize.SamTable(path, eng)
    assert table.rows.tobytes() == r["rows"].tobytes() and table.n_cs == int(r["raw"].n_cs)
    seen = check_same_outcome(table, path)
    assert all(what[0] == "returns" for what in seen.values()), {k: v[1:] for k, v in seen.items() if v[0] != "returns"}
    halves = characterize.SamTable(path, eng, batch_bytes=len(text) // 3)
    assert halves.rows.tobytes() == table.rows.tobytes() and halves.header.tobytes() == table.header.tobytes()
    print("ms_kernel %.3f for %d records, %d bytes" % (r["raw"].ms_kernel, len(rows), len(text)))
