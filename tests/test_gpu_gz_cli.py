"""`--gzip` of the simulator CLI on the GPU ("BGZF output"): a run with the flag and a run without it at the same seed; gunzip of
every .gz file — or of cat $(cat <file>.subfiles) — is the plain run's file, byte for byte, and every file is BGZF to the walk of
characterize/bam.py (BC/BSIZE, CRC32, ISIZE, the end-of-file block last and only there).  The plain runs are the ones tests/test_gpu_cli.py
holds against the oracle."""
import gzip
import os

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import simulator
from nanosim_amd.characterize import bam
from tests import gz_lib as G
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PREFIX = os.path.join(GOLDEN, "model_small", "training")
GENOME = ["genome", "-rg", os.path.join(GOLDEN, "genome_small.fa"), "-c", PREFIX, "-n", "3000", "--seed", "20261021"]
META = ["metagenome", "-gl", os.path.join(GOLDEN, "meta", "genome_list.tsv"), "-a", os.path.join(GOLDEN, "meta", "abundance.tsv"),
        "-dl", os.path.join(GOLDEN, "meta", "dna_type_list.tsv"), "-c", PREFIX, "--seed", "777", "--chimeric", "--fastq"]
TRX = ["transcriptome", "-rt", os.path.join(GOLDEN, "trx", "transcripts.fa"), "-e", os.path.join(GOLDEN, "trx", "expression.tsv"), "--polya",
       os.path.join(GOLDEN, "trx", "polya.txt"), "-b", "guppy", "-c", PREFIX, "-n", "1500", "--seed", "4242", "--no_model_ir", "--uracil", "--fastq"]
CASES = {
    "fasta_t1": GENOME + ["--chimeric", "-t", "1"],
    "fastq_t3_keep": GENOME + ["--chimeric", "--fastq", "-t", "3", "--no-merge"],
    "perfect": GENOME + ["--perfect"],
    "metagenome": META,
    "transcriptome": TRX,
}


def cat_parts(path):
    lst = path + ".subfiles"
    names = [x for x in open(lst).read().split("\n") if x] if os.path.exists(lst) else [path]
    return b"".join(open(x, "rb").read() for x in names), names


def outputs_of(d):
    """the outputs of a run in directory d: what is neither a part nor a list of parts, and what the lists stand for"""
    names = set()
    for f in os.listdir(d):
        if f.endswith(".subfiles"):
            names.add(f[:-len(".subfiles")])
    parts = {os.path.basename(x) for n in names for x in cat_parts(os.path.join(d, n))[1]}
    return sorted(names | {f for f in os.listdir(d) if not f.endswith(".subfiles") and f not in parts})


@pytest.mark.parametrize("case", sorted(CASES))
def test_gunzip_of_a_gzip_run_is_the_plain_run(case, tmp_path, monkeypatch):
    monkeypatch.chdir(ROOT)                                  # (the metagenome's genome list holds paths relative to the repository root)
    monkeypatch.setattr(simulator, "BATCH_READS", 1100)     # several batches per phase: both result slots carry a compressed image
    for k in ("NS_SERIAL", "NS_TWO_ENGINES", "NS_CLI_DROP_OUTPUT"):
        monkeypatch.delenv(k, raising=False)
    plain, gz = str(tmp_path / "plain"), str(tmp_path / "gz")
    monkeypatch.setenv("NS_KEEP_SUBFILES", "0")             # (set, so that what --no-merge writes into the environment is undone with the test)
    simulator.main(CASES[case] + ["-o", os.path.join(plain, "sim")])
    monkeypatch.setenv("NS_KEEP_SUBFILES", "0")
    simulator.main(CASES[case] + ["-o", os.path.join(gz, "sim"), "--gzip"])
    want = outputs_of(plain)
    assert outputs_of(gz) == [f + ".gz" for f in want] and len(want) == (6 if case == "metagenome" else len(want)) >= 2
    for f in want:
        data, _ = cat_parts(os.path.join(plain, f))
        members, names = cat_parts(os.path.join(gz, f + ".gz"))
        assert len(data) > 0 or "unaligned" in f, f
        assert gzip.decompress(members) == data, f
        whole = tmp_path / "whole.gz"
        whole.write_bytes(members)
        blocks = list(bam.bgzf_blocks(str(whole)))
        assert b"".join(bam._inflate(str(whole), b) for b in blocks) == data, f
        assert all(b[2] <= E.NS_GZ_BLOCK_BYTES for b in blocks)
        assert members.endswith(E.BGZF_EOF) and members.count(E.BGZF_EOF) == 1
        assert len(names) == (1 if case != "fastq_t3_keep" else len(cat_parts(os.path.join(plain, f))[1]))
        if "error_profile" in f:
            assert bam._inflate(str(whole), blocks[0]) == simulator.ERR_HEADER
        if len(data) > 100000 and "reads.fasta" in f:
            assert len(members) < 0.5 * len(data), f        # five values: at most log2(5) + 1 bits a byte under a Huffman code, names aside; 8 if stored


def test_two_batches_on_one_engine_fill_both_slots(small_model, small_ref, tmp_path):
    """the API under the CLI: two consecutive batches whose compressed images are queued for one file each, the code of the first batch
    serving the second; the second batch is generated while the first one's copies may still be under way"""
    eng = E.Engine(0)
    try:
        eng.set_reference(small_ref)
        eng.load_model(small_model)
        fd = os.open(tmp_path / "reads.gz", os.O_WRONLY | os.O_CREAT, 0o644)
        fe = os.open(tmp_path / "errors.gz", os.O_WRONLY | os.O_CREAT, 0o644)
        sr, se = eng.sink(fd), eng.sink(fe)
        want_r, want_e, codes = [], [], {}
        for k, n in enumerate((900, 1300, 700)):
            p = E.make_params(seed=7, first_read=1000 * k, n_reads=n, fastq=True, chimeric=True, max_len=small_ref.max_chrom, emit_errlog=True)
            b = eng.generate(p)
            exp = O.generate(small_model, small_ref, p)
            want_r.append(exp["records"].tobytes()); want_e.append(exp["errlog"].tobytes())
            for which, sink, size in ((E.NS_BUF_RECORDS, sr, int(b.info.record_bytes)), (E.NS_BUF_ERRLOG, se, int(b.info.errlog_bytes))):
                if which not in codes:
                    h = b.gz_histogram(which)
                    assert h.tolist() == np.bincount(np.frombuffer((want_r if which == E.NS_BUF_RECORDS else want_e)[-1], dtype=np.uint8), minlength=256).tolist()
                    codes[which] = E.build_gz_code(h)
                cuts = [0, size // 3, size // 3, size]
                off = b.gz(which, cuts, codes[which])
                assert off[0] == 0 and off[1] == off[2] and off[3] <= eng.L.ns_gz_bound(size, 3)
                got = b.copy_range(E.GZ_OF[which], 0, np.empty(int(off[3]), dtype=np.uint8), int(off[3])).tobytes()
                plain = (want_r if which == E.NS_BUF_RECORDS else want_e)[-1]
                assert gzip.decompress(got[:int(off[1])]) == plain[:size // 3] and gzip.decompress(got[int(off[2]):]) == plain[size // 3:]
                sink.write(E.GZ_OF[which])
        sr.close(); se.close()
        os.close(fd); os.close(fe)
    finally:
        eng.close()
    assert gzip.decompress((tmp_path / "reads.gz").read_bytes()) == b"".join(want_r)
    assert gzip.decompress((tmp_path / "errors.gz").read_bytes()) == b"".join(want_e)


def test_images_under_codes_that_do_not_fit_equal_the_plain_encoder(small_model, small_ref):
    """ns_gz_result on the images of two batches, held byte for byte against gz_lib.ref_members over the oracle's bytes: under the code
    of the image's own counts; under that code without the newline, so that every block with a line end is stored; under the code of a flat histogram; with cuts at 1, 2 and 3 modulo 4 and an empty range; and twice on one batch with other
    cuts, where the second image takes the place of the first.  The device's counts are numpy's for both images of both batches."""
    eng = E.Engine(0)
    try:
        eng.set_reference(small_ref)
        eng.load_model(small_model)
        for k, n in enumerate((110, 170)):
            p = E.make_params(seed=11, first_read=1000 * k, n_reads=n, fastq=True, chimeric=True, max_len=small_ref.max_chrom, emit_errlog=True)
            b = eng.generate(p)
            exp = O.generate(small_model, small_ref, p)
            for which, plain in ((E.NS_BUF_RECORDS, exp["records"].tobytes()), (E.NS_BUF_ERRLOG, exp["errlog"].tobytes())):
                size = len(plain)
                assert size == int(b.info.record_bytes if which == E.NS_BUF_RECORDS else b.info.errlog_bytes) > 4 * G.B
                counts = np.bincount(np.frombuffer(plain, dtype=np.uint8), minlength=256).astype(np.uint64)
                assert b.gz_histogram(which).tolist() == counts.tolist() and counts[10] > 0
                no_newline = counts.copy()
                no_newline[10] = 0
                third = size // 3
                cut_sets = [[0, third - third % 4 + 1, 2 * third - (2 * third) % 4 + 2, size - size % 4 - 1, size - size % 4 - 1, size],
                            [0, size], [3, 2 * G.B + 2, size - 5]]
                assert [c % 4 for c in cut_sets[0][1:4]] == [1, 2, 3]
                saw, ref = set(), {}
                for name, handed in (("own", E.build_gz_code(counts)), ("no_newline", E.build_gz_code(no_newline)),
                                     ("flat", E.build_gz_code(np.full(256, 1000, dtype=np.uint64))), ("counted", None)):
                    code = G.plain_code(handed if handed is not None else E.build_gz_code(counts))
                    for cuts in cut_sets:                       # (every call on this batch replaces the image of the call before)
                        off = b.gz(which, cuts, handed)
                        got = b.copy_range(E.GZ_OF[which], 0, np.empty(int(off[-1]), dtype=np.uint8), int(off[-1])).tobytes()
                        assert off[0] == 0 and len(got) == int(off[-1]) <= eng.L.ns_gz_bound(size, len(cuts) - 1)
                        for i in range(len(cuts) - 1):
                            key = (G.code_bytes(code), cuts[i], cuts[i + 1])       # ("own" and "counted" must be one code)
                            if key not in ref:
                                ref[key] = G.ref_members(code, plain[cuts[i]:cuts[i + 1]])
                            want = ref[key]
                            assert got[int(off[i]):int(off[i + 1])] == want, (name, which, cuts, i)
                        if name == "no_newline" and len(cuts) == 2:         # every block with a line end is a stored one
                            at = 0
                            for lo in range(0, size, G.B):
                                m = G.ref_member(code, plain[lo:lo + G.B])
                                assert got[at:at + len(m)] == m
                                if b"\n" in plain[lo:lo + G.B]:
                                    assert got[at + 18] == 1 and len(m) == 31 + len(plain[lo:lo + G.B])
                                    saw.add(True)
                                at += len(m)
                assert saw == {True}
    finally:
        eng.close()
