"""`--gzip` of the simulator CLI on the CPU ("BGZF output"): the layout of the files, on a recording stand-in for engine.Engine
whose Batch.gz makes real BGZF members on the host (zlib) — so the files of a run can be read back with gzip and with the BGZF walk of
characterize/bam.py, and the log of the engine's calls says what the flag adds.  The stand-in is this file's own; tests/fake_engine.py is
the plain one it extends."""
import gzip
import os
import sys
import threading

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import shard, simulator
from nanosim_amd.characterize import bam
from tests.fake_engine import RecordingEngine, _FakeBatch, _FakeSink

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = "tests/golden/model_small/training"
GENOME = ["genome", "-rg", "tests/golden/genome_small.fa", "-n", "3000"]
META = ["metagenome", "-gl", "tests/golden/meta/genome_list.tsv", "-a", "tests/golden/meta/abundance.tsv", "-dl", "tests/golden/meta/dna_type_list.tsv"]
BATCH = 700


class GzBatch(_FakeBatch):
    def __init__(self, log, first, n, with_err):
        super().__init__(first, n, with_err)
        self.log, self.gz_img = log, {}

    def image(self, which):
        return b"".join(self.rec if which == E.NS_BUF_RECORDS else self.err)

    def record_offsets(self, cuts):
        self.log.append(("record_offsets", tuple(int(c) for c in cuts)))
        return super().record_offsets(cuts)

    def gz_histogram(self, which):
        self.log.append(("gz_histogram", which))
        return np.bincount(np.frombuffer(self.image(which), dtype=np.uint8), minlength=256).astype(np.uint64)

    def gz(self, which, cuts, code=None):
        cuts = [int(c) for c in cuts]
        self.log.append(("gz", which, tuple(cuts), None if code is None else bytes(code.len)))
        img, parts = self.image(which), []
        assert cuts == sorted(cuts) and cuts[-1] <= len(img)
        for lo, hi in zip(cuts, cuts[1:]):
            parts.append(E.gz_header_member(img[lo:hi]))
        self.gz_img[E.GZ_OF[which]] = b"".join(parts)
        return np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)


class GzSink(_FakeSink):
    def put(self, data):
        self.eng.log.append(("put", self.name, bytes(data)))
        super().put(data)

    def write(self, which, offset=0, nbytes=None):
        self.eng.log.append(("write", self.name, which, int(offset), None if nbytes is None else int(nbytes)))
        if which in (E.NS_BUF_RECORDS_GZ, E.NS_BUF_ERRLOG_GZ):
            img = self.eng.last.gz_img[which]
            os.write(self.fd, img[offset:] if nbytes is None else img[offset:offset + nbytes])
        else:
            super().write(0 if which == E.NS_BUF_RECORDS else 1, offset, nbytes)


class GzEngine(RecordingEngine):
    def __init__(self, world, owner=None):
        super().__init__(world, owner=owner)
        self.log = world.log

    def _serve(self, p):
        self.log.append(("generate", int(p.first_read), int(p.n_reads)))
        self.requests.append((int(p.first_read), int(p.n_reads)))
        self.last = GzBatch(self.log, int(p.first_read), int(p.n_reads), bool(p.emit_errlog))
        return self.last

    def sink(self, fd):
        s = GzSink(self, fd)
        s.name = os.path.basename(os.readlink("/proc/self/fd/%d" % fd))
        self.log.append(("sink", s.name))
        self.sinks.append(s)
        return s


class GzWorld:
    def __init__(self):
        self.created, self.closed, self.lock, self.log = [], [], threading.Lock(), []

    def __call__(self, device=0):
        return GzEngine(self)


def run(argv, tmp_path, monkeypatch, name):
    world = GzWorld()
    monkeypatch.setattr(E, "Engine", world)
    monkeypatch.setattr(simulator, "BATCH_READS", BATCH)
    monkeypatch.setattr(sys, "argv", ["simulator"])
    for k in ("NS_TWO_ENGINES", "NS_CLI_TRACE", "NS_CLI_DROP_OUTPUT", "NS_FORCE_DIST", "RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NS_SERIAL", "1")
    monkeypatch.setenv("NS_KEEP_SUBFILES", "0")             # (set, so that what --no-merge writes into the environment is undone with the test)
    monkeypatch.chdir(ROOT)
    out = tmp_path / name
    simulator.main(argv + ["-c", PREFIX, "-o", str(out / "sim"), "--seed", "31"])
    return world, out


def cat_parts(path):
    """the bytes of an output: the file itself, or cat $(cat <file>.subfiles)"""
    lst = str(path) + ".subfiles"
    names = [x for x in open(lst).read().split("\n") if x] if os.path.exists(lst) else [str(path)]
    return b"".join(open(x, "rb").read() for x in names), names


def walk(path, tmp_path):
    """the file through the BGZF walk of characterize/bam.py (which insists on the end-of-file block at the end): the inflated blocks"""
    data, _ = cat_parts(path)
    whole = tmp_path / "whole.gz"
    whole.write_bytes(data)
    blocks = [bam._inflate(str(whole), b) for b in bam.bgzf_blocks(str(whole))]
    assert data.endswith(E.BGZF_EOF) and data.count(E.BGZF_EOF) == 1
    return blocks


def plain_log(log):
    """a --gzip run's log without what the flag adds: no gz calls, the plain buffer ids, no byte counts (they are the compressed ones)"""
    back = {E.NS_BUF_RECORDS_GZ: E.NS_BUF_RECORDS, E.NS_BUF_ERRLOG_GZ: E.NS_BUF_ERRLOG}
    out = []
    for c in log:
        if c[0] in ("gz", "gz_histogram"):
            continue
        if c[0] == "write":
            c = ("write", c[1].replace(".gz", ""), back.get(c[2], c[2]))
        elif c[0] == "put":
            c = ("put", c[1].replace(".gz", ""))
        elif c[0] == "sink":
            c = ("sink", c[1].replace(".gz", ""))
        out.append(c)
    return out


@pytest.mark.parametrize("case", ["fasta_t1", "fastq_t3", "fastq_t3_keep", "perfect"])
def test_gzip_run_holds_the_plain_runs_bytes(case, tmp_path, monkeypatch):
    argv = GENOME + {"fasta_t1": [], "fastq_t3": ["--fastq", "-t", "3"], "fastq_t3_keep": ["--fastq", "-t", "3", "--no-merge"], "perfect": ["--perfect"]}[case]
    ext = ".fastq" if "--fastq" in argv else ".fasta"
    w_plain, d_plain = run(argv, tmp_path, monkeypatch, "plain")
    w_gz, d_gz = run(argv + ["--gzip"], tmp_path, monkeypatch, "gz")
    outputs = ["sim_aligned_reads" + ext, "sim_aligned_error_profile"] + ([] if case == "perfect" else ["sim_unaligned_reads" + ext])
    keep = case == "fastq_t3_keep"
    # names: every file of the plain run has its .gz twin and nothing else is there (a list of parts keeps its own suffix last)
    twin = lambda f: f[:-len(".subfiles")] + ".gz.subfiles" if f.endswith(".subfiles") else f + ".gz"
    assert sorted(os.listdir(d_gz)) == sorted(twin(f) for f in os.listdir(d_plain))
    assert set(outputs) <= set(os.listdir(d_plain)) or keep
    for o in outputs:
        want, plain_names = cat_parts(d_plain / o)
        got, gz_names = cat_parts(d_gz / (o + ".gz"))
        assert gzip.decompress(got) == want, o
        assert b"".join(walk(d_gz / (o + ".gz"), tmp_path)) == want, o
        # .subfiles order: part for part the plain run's, and only the last one ends the file
        assert [os.path.basename(x) for x in gz_names] == [twin(os.path.basename(x)) for x in plain_names]
        for k, (g, p) in enumerate(zip(gz_names, plain_names)):
            data = open(g, "rb").read()
            assert gzip.decompress(data) == open(p, "rb").read(), g
            assert data.endswith(E.BGZF_EOF) == (k == len(gz_names) - 1), g
    # the header line of the error profile is the first member, on its own
    first = walk(d_gz / "sim_aligned_error_profile.gz", tmp_path)[0]
    assert first == simulator.ERR_HEADER
    puts = [c for c in w_gz.log if c[0] == "put"]
    assert len(puts) == 1 and puts[0][2] == E.gz_header_member(simulator.ERR_HEADER)
    # a run without the flag makes no call the flag adds, and the flag adds calls only
    assert not [c for c in w_plain.log if c[0] in ("gz", "gz_histogram") or (c[0] == "write" and c[2] not in (E.NS_BUF_RECORDS, E.NS_BUF_ERRLOG))]
    strip = lambda log: [c[:3] if c[0] == "write" else c[:2] if c[0] == "put" else c for c in log]
    assert plain_log(w_gz.log) == strip(w_plain.log)


def test_cuts_map_to_ranges_and_the_code_is_built_once(tmp_path, monkeypatch):
    w, d = run(GENOME + ["--fastq", "-t", "3", "--gzip"], tmp_path, monkeypatch, "gz")
    log = w.log
    # one histogram per output stream of the run: records and error profile of the aligned phase, records of the unaligned one
    assert [c[1] for c in log if c[0] == "gz_histogram"] == [E.NS_BUF_RECORDS, E.NS_BUF_ERRLOG, E.NS_BUF_RECORDS]
    codes = {}
    for k, c in enumerate(log):
        if c[0] != "generate":
            continue
        n = c[2]
        nxt = [x for x in log[k + 1:]]
        end = next((i for i, x in enumerate(nxt) if x[0] == "generate"), len(nxt))
        calls = nxt[:end]
        ro = [x for x in calls if x[0] == "record_offsets"]
        assert len(ro) == 1 and ro[0][1] == tuple(sorted({j * n // 3 for j in range(4)}))
        b = _FakeBatch(c[1], n, True)
        rec_cuts = tuple(int(v) for v in _FakeBatch.record_offsets(b, ro[0][1])[0])
        gz = [x for x in calls if x[0] == "gz"]
        assert gz[0][1] == E.NS_BUF_RECORDS and gz[0][2] == rec_cuts            # the cuts of record_offsets, as they are
        for x in gz:
            assert x[3] is not None
            phase = (x[1], c[1] >= 2850)                                        # (the unaligned reads follow the 2850 aligned ones)
            assert codes.setdefault(phase, x[3]) == x[3]                        # one code per stream, whatever the batch
        writes = [x for x in calls if x[0] == "write"]
        assert all(x[2] in (E.NS_BUF_RECORDS_GZ, E.NS_BUF_ERRLOG_GZ) for x in writes)
        assert len(writes) == len(gz) * (len(ro[0][1]) - 1)
    assert len(codes) == 3


def test_metagenome_samples_take_the_same_path(tmp_path, monkeypatch):
    w_plain, d_plain = run(META, tmp_path, monkeypatch, "plain")
    w_gz, d_gz = run(META + ["--gzip"], tmp_path, monkeypatch, "gz")
    assert sorted(os.listdir(d_gz)) == sorted(f + ".gz" for f in os.listdir(d_plain))
    assert len(os.listdir(d_gz)) == 6                                           # two samples, three outputs each
    for f in os.listdir(d_plain):
        assert gzip.decompress((d_gz / (f + ".gz")).read_bytes()) == (d_plain / f).read_bytes()
        walk(d_gz / (f + ".gz"), tmp_path)


def test_subfile_names_keep_gz_last():
    assert shard.subfile_path("o/sim_aligned_reads.fastq.gz", 2) == "o/sim_aligned_reads2.fastq.gz"
    assert shard.subfile_path("o/sim_aligned_error_profile.gz", "1_0") == "o/sim_error_profile1_0.gz"
    assert shard.subfile_path("o/sim_unaligned_reads.fasta", 0) == "o/sim_unaligned_reads0.fasta"
