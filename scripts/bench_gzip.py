#!/usr/bin/env python3
"""What --gzip costs and saves ("BGZF output"), on BASELINE configs[1]: E. coli-like reference, hg002-like model.

  sizes   compressed / plain per stream (FASTA records, FASTQ records, error profile) over 3 steps of 10^6 reads after one untimed step,
          and, on the first 64 MB of each stream, next to zlib with Z_HUFFMAN_ONLY — the best a literal-only code with per-block tables does;
  kernel  the time of ns_gz_result per step by event pair (its first kernel to its last; NS_GZ_TRACE=1 prints it);
  cli     reads/s of the whole CLI with and without --gzip, alternating, same process, same box: into /dev/null (-t 1, NS_CLI_DROP_OUTPUT=1)
          and into tmpfs (-t 16 --no-merge).  Model and reference loading are inside the time, as in scripts/bench_cli.py.

Prints one JSON object."""
import argparse
import json
import os
import re
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanosim_amd import engine as E, model as M, simulator, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--cli-reads", type=int, default=1_000_000)
ap.add_argument("--cli-repeats", type=int, default=2)
ap.add_argument("--dir", default="/dev/shm")
ap.add_argument("--no-cli", action="store_true")
a = ap.parse_args()
SAMPLE = 64 << 20
d = tempfile.mkdtemp(prefix="nsgz_", dir=a.dir)
out = {}
try:
    prefix = os.path.join(d, "training")
    synth.write_model(prefix, synth.SynthModelSpec(n_train=1_000_000, seed=1), write_pkl=False)
    fa = os.path.join(d, "ecoli_like.fa")
    synth.write_fasta(fa, [("ecoli-like", synth.synth_sequence(synth.ECOLI_LEN, 1, n_frac=0.0005, iupac_frac=0.0002, lower_frac=0.02, hp_boost=0.005))])
    ref = M.read_fasta(fa, "circular")
    trace = os.path.join(d, "gz_trace.txt")
    os.environ["NS_GZ_TRACE"] = "1"
    for fastq in (False, True):
        mdl = M.load_model(prefix, fastq=fastq)
        n_al, _ = mdl.split_counts(a.reads)
        eng = E.Engine(0)
        eng.set_reference(ref)
        eng.load_model(mdl)
        streams = {E.NS_BUF_RECORDS: "fastq" if fastq else "fasta"}
        if not fastq:
            streams[E.NS_BUF_ERRLOG] = "error_profile"
        codes, tot = {}, {k: [0, 0] for k in streams}
        sys.stderr.flush()
        saved = os.dup(2)
        fd = os.open(trace, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.dup2(fd, 2)                                   # the library's trace lines
        try:
            for step in range(a.steps + 1):
                p = E.make_params(seed=1, first_read=step * a.reads, n_reads=n_al, fastq=fastq, max_len=ref.max_chrom, emit_errlog=not fastq)
                b = eng.generate(p)
                for which, name in streams.items():
                    size = int(b.info.record_bytes if which == E.NS_BUF_RECORDS else b.info.errlog_bytes)
                    if which not in codes:
                        codes[which] = E.build_gz_code(b.gz_histogram(which))
                    off = b.gz(which, [0, size], codes[which])
                    if step:
                        tot[which][0] += size
                        tot[which][1] += int(off[-1])
                    if step == a.steps:                  # the yardstick, on the same bytes
                        n = min(size, SAMPLE)
                        plain = b.copy_range(which, 0, np.empty(n, dtype=np.uint8), n)
                        ours, _ = eng.gz_bytes(plain, code=codes[which])
                        z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
                        ref_bytes = len(z.compress(plain.tobytes())) + len(z.flush())
                        out.setdefault("sizes", {})[name] = dict(plain_bytes_per_step=size, sample_bytes=n, ours_over_plain_sample=len(ours) / n,
                                                                zlib_huffman_only_over_plain_sample=ref_bytes / n, gap=len(ours) / ref_bytes - 1.0)
        finally:
            os.dup2(saved, 2)
            os.close(fd); os.close(saved)
        eng.close()
        ms = {}
        for ln in open(trace):
            m = re.match(r"\[gz\] buffer (\d+): (\d+) -> (\d+) bytes, (\d+) blocks, ([0-9.]+) ms", ln)
            if m:
                ms.setdefault(int(m.group(1)), []).append(float(m.group(5)))
        for which, name in streams.items():
            out["sizes"][name]["compressed_over_plain"] = tot[which][1] / tot[which][0]
            out.setdefault("kernel_ms_per_step", {})[name] = ms.get(which, [])[1:]       # (without the untimed step)
    os.environ.pop("NS_GZ_TRACE", None)

    if not a.no_cli:
        def cli(gz, dest):
            o = os.path.join(d, "run")
            os.makedirs(o, exist_ok=True)
            argv = ["genome", "-rg", fa, "-c", prefix, "-o", os.path.join(o, "sim"), "-n", str(a.cli_reads), "--seed", "1", "-dna_type", "circular"]
            argv += ["-t", "1"] if dest == "null" else ["-t", "16", "--no-merge"]
            os.environ["NS_CLI_DROP_OUTPUT"] = "1" if dest == "null" else "0"
            so, sys.stdout = sys.stdout, open(os.devnull, "w")
            t0 = time.perf_counter()
            try:
                simulator.main(argv + (["--gzip"] if gz else []))
            finally:
                sys.stdout = so
            dt = time.perf_counter() - t0
            size = sum(os.path.getsize(os.path.join(o, f)) for f in os.listdir(o))
            shutil.rmtree(o, ignore_errors=True)
            os.environ.pop("NS_KEEP_SUBFILES", None)
            return dict(reads_per_s=a.cli_reads / dt, seconds=dt, file_bytes=size)
        out["cli"] = {dest: {"plain": [], "gzip": []} for dest in ("null", "tmpfs")}
        for dest in ("null", "tmpfs"):
            for _ in range(a.cli_repeats):
                for gz in (False, True):
                    out["cli"][dest]["gzip" if gz else "plain"].append(cli(gz, dest))
finally:
    shutil.rmtree(d, ignore_errors=True)
print(json.dumps(out))
