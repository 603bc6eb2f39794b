#!/usr/bin/env python
"""Drop-in for the simulation stage of NanoSim: same sub-commands, flags, model files and output files as
``src/simulator.py`` of bcgsc/NanoSim v3.2.2 (CLI: S:2070-2218, genome driver: S:2226-2320), with the per-read
loop running on MI355X through the C-ABI (include/nanosim_amd.h).

    python -m nanosim_amd.simulator genome -rg ref.fa -c model/training -o out/simulated -n 100000 [--fastq] ...

Differences a user can see: ``--seed`` is honoured (the reference re-seeds from the OS in
``simulation()``, S:1591-1592, so its --seed has no effect); read numbers are the read's index (no gaps);
``-t K`` keeps the reference's meaning for the OUTPUT (K sub-files written side by side, then concatenated, S:1588-1639) while GPUs,
not processes, do the work (run under ``torch.distributed.run`` for several GPUs).  ``--gzip`` (not in the reference) writes every
output as a BGZF ``.gz`` file whose bytes are deflated on the GPU before they are copied ("BGZF output").
"""
from __future__ import annotations

import argparse
import contextlib
import os
import sys
import time
from textwrap import dedent
from time import strftime

import numpy as np

from . import engine as E
from . import model as M
from . import shard

VERSION = "3.2.2"
BATCH_READS = 1_000_000
ERR_HEADER = b"Seq_name\tSeq_pos\terror_type\terror_length\tref_base\tseq_base\n"      # S:1634


def log(msg):
    sys.stdout.write(strftime("%Y-%m-%d %H:%M:%S") + ": " + msg + "\n")
    sys.stdout.flush()


MERGE_HELP = ("Not in the reference: with several ranks (one process per GPU) concatenate every rank's sub-files into ONE file per output, "
              "as the reference's workers do (S:1626-1639).  Off by default when WORLD_SIZE > 1: rank 0 would append terabytes through one "
              "inode at 6-10 GB/s after minutes of GPU work; <file>.subfiles lists the parts in order (cat $(cat <file>.subfiles) = <file>)")
GZIP_HELP = ("Not in the reference: write BGZF-compressed outputs (<out>_aligned_reads.fasta.gz / .fastq.gz, <out>_unaligned_reads.*.gz, "
             "<out>_aligned_error_profile.gz; sub-files likewise).  The bytes are deflated on the GPU before they cross PCIe; zcat, gzip, bgzip and "
             "htslib read the files, and cat of the parts listed in <file>.subfiles is again one valid file")
NO_MERGE_HELP = ("Not in the reference: with -t K > 1 (or several ranks) keep the sub-files the workers wrote side by side and list them in "
                 "<file>.subfiles (cat $(cat <file>.subfiles) = <file>) instead of concatenating them into one file as the reference does "
                 "(S:1626-1639).  Writes into ONE inode serialise in the kernel (5.7 GB/s on the measured box): the merge, not the GPU, sets "
                 "the wall clock of a large run.  NS_KEEP_SUBFILES=1 does the same")


def build_parser():
    parser = argparse.ArgumentParser(
        description=dedent('''
        Simulation step
        -----------------------------------------------------------
        Given error profiles, reference genome, metagenome,
        and/or transcriptome, simulate ONT DNA or RNA reads
        '''), formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('-v', '--version', action='version', version='NanoSim ' + VERSION + ' (nanosim_amd, MI355X)')
    sub = parser.add_subparsers(help="You may run the simulator on genome, transcriptome, or metagenome mode.", dest='mode')

    g = sub.add_parser('genome', help="Run the simulator on genome mode")
    g.add_argument('-rg', '--ref_g', help='Input reference genome', required=True)
    g.add_argument('-c', '--model_prefix', default="training",
                   help='Location and prefix of error profiles generated from characterization step (Default = training)')
    g.add_argument('-o', '--output', default="simulated", help='Output location and prefix for simulated reads (Default = simulated)')
    g.add_argument('-n', '--number', type=int, default=20000, help='Number of reads to be simulated (Default = 20000)')
    g.add_argument('-x', '--coverage', type=float, default=None,
                   help='Coverage of the simulated reads, Note: Coverage will override the number of reads')
    g.add_argument('-max', '--max_len', type=int, default=float("inf"), help='The maximum length for simulated reads (Default = Infinity)')
    g.add_argument('-min', '--min_len', type=int, default=50, help='The minimum length for simulated reads (Default = 50)')
    g.add_argument('-med', '--median_len', type=int, default=None, help='The median read length (Default = None)')
    g.add_argument('-sd', '--sd_len', type=float, default=None, help='The standard deviation of read length in log scale (Default = None)')
    g.add_argument('--seed', type=int, default=None, help='Manually seeds the pseudo-random number generator')
    g.add_argument('-hp', '--homopolymer', action='store_true', default=False, help='Simulate homopolymer lengths (Default = False)')
    g.add_argument('-k', '--KmerBias', type=int, default=None,
                   help='Minimum homopolymer length to simulate homopolymer contraction and expansion events in, a typical k is 5')
    g.add_argument('-s', '--strandness', type=float, default=None,
                   help='Proportion of sense sequences. Overrides the value profiled in characterization stage.')
    g.add_argument('-dna_type', choices=["linear", "circular"], default="linear", help='Specify the dna type: circular OR linear (Default = linear)')
    g.add_argument('--perfect', action='store_true', default=False, help='Ignore error profiles and simulate perfect reads')
    g.add_argument('--fastq', action='store_true', default=False, help='Output fastq files instead of fasta files')
    g.add_argument('--chimeric', action='store_true', default=False, help='Simulate chimeric reads')
    g.add_argument('-t', '--num_threads', type=int, default=1, help='Number of threads for simulation (Default = 1)')
    g.add_argument('--no-merge', dest='no_merge', action='store_true', default=False, help=NO_MERGE_HELP)
    g.add_argument('--merge', dest='merge', action='store_true', default=False, help=MERGE_HELP)
    g.add_argument('--gzip', dest='gzip', action='store_true', default=False, help=GZIP_HELP)

    t = sub.add_parser('transcriptome', help="Run the simulator on transcriptome mode")
    t.add_argument('-rt', '--ref_t', required=True)
    t.add_argument('-rg', '--ref_g', default='')
    t.add_argument('-e', '--exp', required=True)
    t.add_argument('-c', '--model_prefix', default="training")
    t.add_argument('-o', '--output', default="simulated")
    t.add_argument('-n', '--number', type=int, default=20000)
    t.add_argument('-x', '--coverage', type=float, default=None)
    t.add_argument('-max', '--max_len', type=int, default=float("inf"))
    t.add_argument('-min', '--min_len', type=int, default=50)
    t.add_argument('--seed', type=int, default=None)
    t.add_argument('-hp', '--homopolymer', action='store_true', default=False)
    t.add_argument('-k', '--KmerBias', type=int, default=None)
    t.add_argument('-b', '--basecaller', choices=["albacore", "guppy"], default=None)
    t.add_argument('-s', '--strandness', type=float, default=None)
    t.add_argument('--no_model_ir', action='store_false', default=True)
    t.add_argument('--perfect', action='store_true', default=False)
    t.add_argument('--polya', default=None)
    t.add_argument('--fastq', action='store_true', default=False)
    t.add_argument('-t', '--num_threads', type=int, default=1)
    t.add_argument('--no-merge', dest='no_merge', action='store_true', default=False, help=NO_MERGE_HELP)
    t.add_argument('--merge', dest='merge', action='store_true', default=False, help=MERGE_HELP)
    t.add_argument('--gzip', dest='gzip', action='store_true', default=False, help=GZIP_HELP)
    t.add_argument('--uracil', action='store_true', default=False)

    mg = sub.add_parser('metagenome', help="Run the simulator on metagenome mode")
    mg.add_argument('-gl', '--genome_list', required=True)
    mg.add_argument('-a', '--abun', required=True)
    mg.add_argument('-dl', '--dna_type_list', required=True)
    mg.add_argument('-c', '--model_prefix', default="training")
    mg.add_argument('-o', '--output', default="simulated")
    mg.add_argument('-max', '--max_len', type=int, default=float("inf"))
    mg.add_argument('-min', '--min_len', type=int, default=50)
    mg.add_argument('-med', '--median_len', type=int, default=None)
    mg.add_argument('-sd', '--sd_len', type=float, default=None)
    mg.add_argument('--seed', type=int, default=None)
    mg.add_argument('-hp', '--homopolymer', action='store_true', default=False)
    mg.add_argument('-k', '--KmerBias', type=int, default=None)
    mg.add_argument('-s', '--strandness', type=float, default=None)
    mg.add_argument('--perfect', action='store_true', default=False)
    mg.add_argument('--abun_var', nargs='+', type=float, default=None)
    mg.add_argument('--fastq', action='store_true', default=False)
    mg.add_argument('--chimeric', action='store_true', default=False)
    mg.add_argument('-t', '--num_threads', type=int, default=1)
    mg.add_argument('--no-merge', dest='no_merge', action='store_true', default=False, help=NO_MERGE_HELP)
    mg.add_argument('--merge', dest='merge', action='store_true', default=False, help=MERGE_HELP)
    mg.add_argument('--gzip', dest='gzip', action='store_true', default=False, help=GZIP_HELP)
    return parser, g, mg, t


def calculate_read_number_from_coverage(ref: M.Reference, model_prefix: str, coverage: float) -> int:
    """S:2024-2068.  The reference estimates the mean read length with 10^7 KDE samples; a Gaussian KDE sample has
    the mean of its training vector, so the expectation is taken directly."""
    rate = None
    with open(model_prefix + "_reads_alignment_rate") as f:
        rate = float(f.readline().strip().split('\t')[1])
    npz = np.load(model_prefix + "_kde.npz") if os.path.exists(model_prefix + "_kde.npz") else None
    al = M._load_kde(model_prefix, "aligned_reads", npz)[0]
    un = M._load_kde(model_prefix, "unaligned_length", npz)[0]
    n_est = 10000000
    n_al = int(n_est * rate / (rate + 1))
    mean = (n_al * float(al.mean()) + (n_est - n_al) * float(un.mean())) / n_est
    return int(ref.genome_len / mean * coverage)


def validate_genome_args(a, parser_mode):
    """For all three modes, despite its name: the checks of a mode's branch of main(), before anything is opened (genome S:2251-2280,
    transcriptome S:2350-2374, metagenome S:2438-2467): same messages in the same order, usage on stderr, exit code 1.  The
    transcriptome parser has no read-length distribution and no --chimeric, the other two no intron retention and no polyA tails: a
    flag a mode lacks counts as not given."""
    def die(msg, to_err=True):
        (sys.stderr if to_err else sys.stdout).write("\n" + msg + "\n")
        parser_mode.print_help(sys.stderr)
        sys.exit(1)
    median_len, sd_len, chimeric = (getattr(a, k, None) for k in ("median_len", "sd_len", "chimeric"))
    if a.homopolymer and (a.KmerBias is None or a.KmerBias < 0):
        die("Please input proper kmer bias value >= 0 to simulate homopolymer contraction and expansion events from", False)
    if a.strandness and (a.strandness < 0 or a.strandness > 1):
        die("Please input proper strandness value between 0 and 1", False)
    if (median_len and not sd_len) or (sd_len and not median_len):
        die("Please provide both mean and standard deviation of read length!")
    if median_len and sd_len and chimeric:
        die("Lognormal distributed reads cannot be chimeric!")
    if a.max_len < a.min_len:
        die("Maximum read length must be longer than Minimum read length!")
    if a.perfect and chimeric:
        die("Perfect reads cannot be chimeric", False)
    if getattr(a, "no_model_ir", False) and a.ref_g == '':                                      # (store_false: True unless --no_model_ir)
        die("Please provide a reference genome to simulate intron retention events!")
    if getattr(a, "polya", None) and a.basecaller is None:
        die("Please input basecaller to simulate polyA tails from.", False)
    if a.KmerBias and not a.homopolymer:                                                       # not in the reference
        sys.stderr.write("\n-k/--KmerBias needs -hp (the reference crashes on the missing homopolymer parameters, S:504,639)\n")
        sys.exit(1)


def _cap_stripes(stripes: int, n_outputs: int) -> int:
    """-t K opens 2 x K descriptors per output (two batches in flight): K is capped at 64 and by RLIMIT_NOFILE"""
    k = max(1, min(int(stripes), 64))
    try:
        import resource
        soft = resource.getrlimit(resource.RLIMIT_NOFILE)[0]
        if soft != resource.RLIM_INFINITY:
            k = max(1, min(k, (int(soft) - 64) // max(1, 4 * n_outputs)))
    except (ImportError, ValueError, OSError):
        pass
    return k


def _step_batches(n_al: int, n_un: int) -> tuple[int, int]:
    """reads per worker call of the two phases: one STEP of BATCH_READS reads = an aligned call on its share and an unaligned call on
    the rest (950 000 + 50 000 at the usual 19:1), so that the two contexts of _run_phases work through the run in lockstep — the step
    bench.py times — instead of the unaligned phase racing ahead in one big batch"""
    tot = max(1, n_al + n_un)
    al = max(1000, min(BATCH_READS, int(round(BATCH_READS * n_al / tot))))
    return al, max(1000, BATCH_READS - al)


def _serial_schedule() -> bool:
    """NS_SERIAL=1: aligned and unaligned worker calls one after the other on ONE engine context (A/B runs, GPUs short of memory)"""
    return os.environ.get("NS_SERIAL", "0") != "0"


def _background_engine(device, setup, owner=None):
    """Where the unaligned worker calls of this GPU run, NEXT TO the aligned ones: by default the step companion of `owner`
    (Engine.step_engine: it shares the owner's reference, model and mode tables, nothing is uploaded twice; the library runs it from
    its own worker thread, ns_generate_step); NS_TWO_ENGINES=1: a second engine context of its own (the schedule of rounds 2-4: `setup`
    installs reference, mode tables and model on it).  Returns (engine of the unaligned calls, owner of a StepPair or None)."""
    if owner is not None and os.environ.get("NS_TWO_ENGINES", "0") == "0":
        return owner.step_engine(), owner
    eng = E.Engine(device)
    try:
        eng.set_background(True)
        setup(eng)
    except BaseException:
        eng.close()
        raise
    return eng, None


class StepPair:
    """Pairs the worker calls of the two phases of a run into steps: when the aligned phase asks for its next batch and the unaligned
    phase is waiting with one, both go into ONE ns_generate_step call (include/nanosim_amd.h) — the aligned call on the engine, the
    unaligned one on its step companion, side by side on the GPU; a phase whose partner has nothing to run (it is done, or busy
    queueing its files) calls on its own.  The unaligned phase posts its next request only when it has queued the last batch for its
    files, so the companion's buffers are never written under it."""

    def __init__(self, eng):
        import threading
        self.eng, self.un_eng = eng, eng.step_engine()
        self.cv = threading.Condition()
        self.pending = None          # parameters of an unaligned call waiting for its step
        self.result = None           # ("ok", Batch) | ("alone", None) for the waiting unaligned call
        self.al_done = False
        self.steps = self.alone = 0

    def aligned(self, p):
        with self.cv:
            pu, self.pending = self.pending, None
        if pu is None:
            self.alone += 1
            return self.eng.generate(p)
        try:
            b_al, b_un = self.eng.generate_step(p, pu)
        except BaseException as ex:
            with self.cv:            # the unaligned call repeats on its own (and reports its own error, if it was its error)
                self.result = ("alone", None)
                self.cv.notify_all()
            b_al = getattr(ex, "aligned_batch", None)
            if b_al is None:
                raise
            return b_al              # only the unaligned half failed: the aligned batch is good and its phase keeps its batch size
        with self.cv:
            self.result = ("ok", b_un)
            self.cv.notify_all()
        self.steps += 1
        return b_al

    def unaligned(self, p):
        with self.cv:
            if not self.al_done:
                self.pending = p
                while self.result is None and not (self.al_done and self.pending is not None):
                    self.cv.wait()
                if self.result is not None:
                    kind, b = self.result
                    self.result = None
                    if kind == "ok":
                        return b
                else:
                    self.pending = None          # the aligned phase ended without taking it
        return self.un_eng.generate(p)

    def finish_aligned(self):
        with self.cv:
            self.al_done = True
            self.cv.notify_all()


def _run_phases(aligned, unaligned, rank, n_done, step_owner=None):
    """simulation() (S:1588-1672) starts the unaligned workers once the aligned ones are joined.  That order constrains the FILES only —
    the two phases write different files and a read is a function of (seed, read index) — so here `unaligned` runs in a second host
    thread NEXT TO `aligned`: one GPU, the schedule bench.py times.  step_owner (an Engine): the two phases take their batches through a
    StepPair of it — `aligned(gen)` / `unaligned(gen)` are then called with the pair's generate functions (one ns_generate_step per step);
    None: they are called without arguments (closures over two engine contexts of their own).
    unaligned is None: nothing to run (--perfect).  The log keeps the reference's order."""
    import threading
    err = []
    pair = StepPair(step_owner) if (step_owner is not None and unaligned is not None) else None

    def bg():
        try:
            unaligned(pair.unaligned) if pair else unaligned()
        except BaseException as ex:                      # (SystemExit of a failed merge included: threading would swallow it)
            err.append(ex)
    t = None
    if unaligned is not None:
        t = threading.Thread(target=bg, name="ns-unaligned")
        t.start()
    try:
        aligned(pair.aligned) if pair else aligned()
    finally:
        if pair:
            pair.finish_aligned()
        if t is not None:
            if rank == 0:
                log("Start simulation of random reads")
            t.join()
    if err:
        raise err[0]
    if pair and os.environ.get("NS_CLI_TRACE") is not None:
        sys.stderr.write("[cli] %d steps through ns_generate_step, %d aligned worker calls on their own\n" % (pair.steps, pair.alone))
    if t is not None and rank == 0:
        sys.stdout.write(strftime("%Y-%m-%d %H:%M:%S") + ": Number of reads simulated >> " + str(n_done) + "\n")
        sys.stdout.flush()


def _gz_end_of_file(path, keep):
    """--gzip, rank 0, once every part of `path` is in place: the 28-byte BGZF end-of-file block behind the last byte — of the merged
    file, or of the last part that <path>.subfiles lists"""
    last = path
    if keep and os.path.exists(path + ".subfiles"):
        names = [x for x in open(path + ".subfiles").read().split("\n") if x]
        last = names[-1] if names else path
    with open(last, "ab") as f:
        f.write(E.BGZF_EOF)


def _write_batches(eng, out_path, err_path, params, *, first, count, err_header=b"", dist=None, stripes=1, quiet=False, tag="",
                   batch_reads=None, gen=None, gz=False):
    """Reads [first, first + count) of this rank into out_path (and their error-profile rows into err_path), through the engine's output
    sinks (include/nanosim_amd.h: ns_sink_*): the images of batch i leave the GPU and reach the files while batch i + 1 is generated.
    params: what every worker call of the phase has in common, as keywords of E.make_params (seed, kind, lengths, mode flags).

    stripes == 1: rank 0 writes the final files front to back, every other rank one sub-file per output.
    stripes > 1 (-t K; the reference's workers write K sub-files that are concatenated afterwards, S:1588-1639): every batch is cut at read
    boundaries into K sub-files `<out>_aligned_reads<i>.fasta` / `<out>_error_profile<i>` / `<out>_unaligned_reads<i>.fasta` that are written in
    parallel — writes into ONE file serialise on its inode, K files do not — and appended to the final file at the end, in order.
    NS_KEEP_SUBFILES=1 skips that merge: the sub-files stay and `<file>.subfiles` lists them in order (cat $(cat x.subfiles) = x).
    Several ranks: a rank that is done publishes the list of its sub-files (shard.publish_parts); rank 0 appends them in rank order as they
    appear (shard.collect_parts) — no collective, and a rank that fails leaves a marker instead of a hanging peer.
    quiet: no progress line on stdout (the worker call that runs on the background context, _run_phases).
    gen: what generates a batch from its parameters (StepPair.aligned / .unaligned); None: eng.generate.
    gz (--gzip; the paths end in .gz): every range that would be queued is deflated on the GPU into whole BGZF members first (Batch.gz, with
    the cuts of record_offsets) and the ranges of the compressed images are queued instead.  The code of an output is built once, from the
    byte counts of the first batch that has bytes, and serves every later batch: a block it fits badly, or that has a byte it lacks, is
    stored.  The error profile's header line is a member of its own, made on the host; rank 0 ends every file with the end-of-file block."""
    rank = dist.get_rank() if dist is not None else 0
    stripes = _cap_stripes(stripes, len([p for p in (out_path, err_path) if p]))
    world = dist.get_world_size() if dist is not None else 1
    trace = os.environ.get("NS_CLI_TRACE") is not None       # per-batch host timing on stderr
    keep = os.environ.get("NS_KEEP_SUBFILES", "0") != "0"      # (--no-merge sets it: main)
    batch = min(getattr(eng, "_batch_reads", BATCH_READS), batch_reads or BATCH_READS)
    paths = [p for p in (out_path, err_path) if p]
    which = {out_path: E.NS_BUF_RECORDS, err_path: E.NS_BUF_ERRLOG}
    codes = {}                                               # gz: the code of each output
    if gz and err_header:
        err_header = E.gz_header_member(err_header)

    def gz_offsets(b, p, cuts):
        """the compressed image of output p's plain one, cut at the byte offsets `cuts`: where the members of every range begin"""
        if p not in codes:
            h = b.gz_histogram(which[p])
            if h.any():
                codes[p] = E.build_gz_code(h)
        return b.gz(which[p], cuts, codes.get(p))
    files = {p: [] for p in paths}                           # what holds this rank's bytes of p, in order
    open_now, prev = [], []                                  # (sink, fd) of the batch being queued / of the batch before it
    single = {}                                              # stripes == 1: the one sink per output
    done = n_sub = 0

    def close_all(lst):
        """every (sink, fd) of the list is closed exactly once, whatever fails on the way; the first error is raised at the end"""
        first_err = None
        while lst:
            sk, fd = lst.pop(0)
            try:
                sk.close()                               # waits for the file writes; raises on ENOSPC & co
            except Exception as ex:
                first_err = first_err or ex
            finally:
                try:
                    os.close(fd)
                except OSError as ex:
                    first_err = first_err or ex
        if first_err is not None:
            raise first_err
    try:
        if stripes == 1:
            for p in paths:
                name = shard.part_path(p, rank)
                fd = os.open(name, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                if os.environ.get("NS_CLI_DROP_OUTPUT", "0") != "0":       # measurement aid: the bytes cross PCIe and are dropped (empty files)
                    os.close(fd)
                    fd = os.open("/dev/null", os.O_WRONLY)
                single[p] = eng.sink(fd)
                open_now.append((single[p], fd))
                files[p].append(name)
            if err_path and err_header and rank == 0:   # rank 0 opens the error profile with the column header (S:1634)
                single[err_path].put(err_header)
        while done < count:
            n = min(batch, count - done)
            t0 = time.perf_counter()
            try:
                b = (gen or eng.generate)(E.make_params(first_read=first + done, n_reads=n, emit_errlog=err_path is not None, **params))
            except E.EngineError as ex:              # not enough free HBM for this batch size (shared GPU): halve it and go on
                if getattr(ex, "code", 0) != E.NS_ENOMEM or n <= 1000 or params.get("meta"):
                    raise                            # (metagenome workers: the batches are part of the result)
                batch = eng._batch_reads = max(1000, n // 2)
                continue
            t1 = time.perf_counter()
            sizes = {out_path: int(b.info.record_bytes), err_path: int(b.info.errlog_bytes)}
            if stripes == 1:
                for p in paths:
                    if gz:
                        sizes[p] = int(gz_offsets(b, p, [0, sizes[p]])[-1])
                        single[p].write(E.GZ_OF[which[p]])
                    else:
                        single[p].write(which[p])
            else:
                cuts = sorted({k * n // stripes for k in range(stripes + 1)})
                offs = dict(zip(paths, b.record_offsets(cuts)))
                buf = which
                if gz:
                    offs = {p: gz_offsets(b, p, offs[p]) for p in paths}
                    buf = {p: E.GZ_OF[which[p]] for p in paths}
                    sizes = {p: int(offs[p][-1]) for p in paths}
                for lo, hi in zip(range(len(cuts) - 1), range(1, len(cuts))):
                    for p in paths:
                        name = shard.subfile_path(p, n_sub if world == 1 else "%d_%d" % (rank, n_sub))
                        fd = os.open(name, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                        sk = eng.sink(fd)
                        open_now.append((sk, fd))
                        files[p].append(name)
                        if p == err_path and err_header and rank == 0 and n_sub == 0:
                            sk.put(err_header)
                        sk.write(buf[p], int(offs[p][lo]), int(offs[p][hi] - offs[p][lo]))
                    n_sub += 1
                close_all(prev)                      # the batch before this one is in its files; this one's copies are under way
                prev, open_now = open_now, []
            if trace:
                c = eng.io_counters()
                # device: first to last event of the worker call — it includes what the HOST does in between (the first-use hipMalloc of a result
                # slot, the wait for a slot whose last batch is still crossing PCIe); kernels: the sum of the kernel phases alone
                sys.stderr.write("[cli%s] batch %d reads: generate %.1f ms (device %.1f, kernels %.1f), %.2f GB queued; so far %.2f GB copied at %s GB/s (DMA), copier waited "
                                 "%.2f s for staging, writers %.2f s in pwrite\n"
                                 % (tag, n, (t1 - t0) * 1e3, b.info.ms_total, sum(float(x) for x in b.info.ms_kernel), sum(sizes[p] for p in paths) / 1e9, c["bytes"] / 1e9,
                                    "%.1f" % c["d2h_gbs"] if c["d2h_gbs"] else "-", c["wait_staging_s"], c["write_s"]))
            done += n
            if rank == 0 and not quiet:
                sys.stdout.write(strftime("%Y-%m-%d %H:%M:%S") + ": Number of reads simulated >> " + str(first + done) + "\r")
                sys.stdout.flush()
        close_all(prev)
        close_all(open_now)
        if stripes > 1 and err_path and err_header and rank == 0 and not files[err_path]:     # no reads at all: the header alone
            name = shard.subfile_path(err_path, 0 if world == 1 else "0_0")
            with open(name, "wb") as f:
                f.write(err_header)
            files[err_path].append(name)
        if rank:
            for p in paths:
                shard.publish_parts(p, rank, files[p])
    except BaseException as ex:
        for lst in (prev, open_now):
            try:
                close_all(lst)
            except Exception:
                pass
        if world > 1:
            for p in paths:
                shard.mark_failed(p, rank, repr(ex))
        raise
    if rank == 0:
        if not quiet:
            sys.stdout.write('\n')
        for p in paths:
            shard.collect_parts(p, world, files[p], keep=keep)
            if gz:
                _gz_end_of_file(p, keep)


class _Run:
    """What the three modes share of a run: where it runs (rank, world, dist, device of the broadcast), the engine of the aligned worker
    calls and the one of the unaligned calls, seed, file extension and -t; and the procedure around a mode's own steps — prologue here,
    then broadcast(), `with scope(outputs)`: load_model(), set_up(), simulate() once (metagenome: once per sample)."""

    def __init__(self, a, shown):
        """the process group, the parameter print (`shown`, in the reference's order: the name of a flag, or (label, value)), the output
        directory, the seed"""
        self.a = a
        self.rank, self.device, self.world, self.dist, self.bdev = shard.init_dist()
        if self.rank == 0:
            print("\nrunning the code with following parameters:\n")
            for x in shown:
                print(*((x, getattr(a, x)) if isinstance(x, str) else x))
            log(' '.join(sys.argv))
        d = os.path.dirname(a.output)
        if d:
            os.makedirs(d, exist_ok=True)
        self.ext = ".fastq" if a.fastq else ".fasta"
        self.seed = a.seed if a.seed is not None else int.from_bytes(os.urandom(8), "little") >> 1
        self.stripes = max(a.num_threads, 1)
        self.eng = self.eng_un = self.step_owner = None           # (the mode opens self.eng where it did before: E.Engine(self.device))
        self.keep = None                                          # the broadcast bases on this GPU, while an engine may still copy them

    def outputs(self, base):
        gz = ".gz" if getattr(self.a, "gzip", False) else ""
        return [base + "_aligned_reads" + self.ext + gz, base + "_aligned_error_profile" + gz, base + "_unaligned_reads" + self.ext + gz]

    def broadcast(self, ref, extra=None, outputs=(), error=None):
        """Rank 0's reference, its seed and the mode's small tables `extra` (a dict) for every rank: returns (ref, extra).  error: rank
        0's failed check — every rank leaves together (the verdict travels in the header of the broadcast).  outputs: whose sub-files of
        an earlier run to remove first.  One rank without a process group: nothing travels."""
        if self.dist is None:
            shard.agree(None, error is None, error or "")
            return ref, extra
        shard.clean_parts(outputs, self.rank)
        ref, self.keep, extra = shard.broadcast_reference(ref, self.dist, device=self.bdev, error=error,
                                                          extra=dict(extra or {}, seed=self.seed) if self.rank == 0 else None)
        self.seed = extra["seed"]                                 # rank 0's: a read is a function of (seed, read index)
        if self.bdev is None:                                     # (gloo: the bases arrived in host memory)
            ref = M.Reference(ref.names, self.keep.numpy(), ref.chrom_off, ref.circular)
            self.keep = None
        return ref, extra

    def dev_ptr(self):
        """where the broadcast left the bases on this GPU; None: they are in ref.bases"""
        return self.keep.data_ptr() if self.keep is not None else None

    @contextlib.contextmanager
    def scope(self, outputs):
        """everything after the broadcast: a failure leaves a marker for every output (shard.failure_markers), both engines are closed
        whatever happens, and the run ends as the reference's does"""
        with shard.failure_markers(outputs, self.rank, self.world):
            try:
                yield
            finally:
                if self.eng_un is not None and self.eng_un is not self.eng:
                    self.eng_un.close()
                self.eng.close()
        if self.dist is not None:
            self.dist.destroy_process_group()
        if self.rank == 0:
            log("Finished!")

    def load_model(self, **mode):
        a = self.a
        if self.rank == 0:
            log("Read error profile" if not a.perfect else "Read KDF of aligned reads")
        return M.load_model(a.model_prefix, perfect=a.perfect, strandness=a.strandness, homopolymer=a.homopolymer, fastq=a.fastq, **mode)

    def set_up(self, setup, setup_unaligned=None):
        """setup(engine) installs reference, mode tables and model; then the choice of where the unaligned worker calls run: on the same
        engine (--perfect has none, NS_SERIAL=1 runs them afterwards) or next to the aligned ones (_background_engine; a second engine
        of its own is set up by setup_unaligned, default `setup`)"""
        setup(self.eng)
        self.eng_un = self.eng
        if not self.a.perfect and not _serial_schedule():
            self.eng_un, self.step_owner = _background_engine(self.device, setup_unaligned or setup, self.eng)

    def read_number(self, ref):
        """-n, or what -x makes of it (S:2247-2249, 2346-2348); the note comes from rank 0, as every other line of the run does"""
        if self.a.coverage is None:
            return self.a.number
        if self.rank == 0:
            print("\nCalculating the number of reads to be simulated based on the coverage, if you specified the number of reads "
                  "concurrently with the coverage, coverage will override number of reads.\n")
        return calculate_read_number_from_coverage(ref, self.a.model_prefix, self.a.coverage)

    def simulate(self, base, first, n_al, n_un, common, aligned_only):
        """simulation() (S:1568-1672) for a genome, a transcriptome or one metagenome sample: reads [first, first + n_al) are the aligned
        ones (<base>_aligned_reads, <base>_aligned_error_profile), the n_un after them the unaligned ones (<base>_unaligned_reads);
        this rank writes its share of both.  common / aligned_only: keywords of E.make_params for every worker call / for the aligned
        ones (seed and kind are set here)."""
        a, rank = self.a, self.rank
        if rank == 0:
            log("Start simulation of aligned reads")
        lo, hi = shard.partition(n_al, self.world)[rank]
        ulo, uhi = shard.partition(n_un, self.world)[rank]
        side_by_side = self.eng_un is not self.eng
        out_al, out_err, out_un = self.outputs(base)
        common = dict(common, seed=self.seed)
        meta = bool(common.get("meta"))
        stripes = 1 if meta else self.stripes      # -t has no effect in metagenome mode: not a decision, kept as it has always been
        # deliberate: a metagenome worker call keeps its own species quotas, so its batches are part of the result, never the step's shares
        b_al, b_un = _step_batches(n_al, n_un) if side_by_side and not meta else (None, None)

        def aligned(gen=None):
            _write_batches(self.eng, out_al, out_err, dict(common, kind=E.NS_KIND_PERFECT if a.perfect else E.NS_KIND_ALIGNED, **aligned_only),
                           first=first + lo, count=hi - lo, err_header=ERR_HEADER, dist=self.dist, stripes=stripes, tag=" aligned",
                           batch_reads=b_al, gen=gen, gz=getattr(a, "gzip", False))

        def unaligned(gen=None, quiet=True):                                                    # S:1642-1672
            _write_batches(self.eng_un, out_un, None, dict(common, kind=E.NS_KIND_UNALIGNED), first=first + n_al + ulo, count=uhi - ulo,
                           dist=self.dist, stripes=stripes, quiet=quiet, tag=" unaligned", batch_reads=b_un, gen=gen, gz=getattr(a, "gzip", False))
        if a.perfect:
            aligned()
        elif not side_by_side:
            aligned()
            if rank == 0:
                log("Start simulation of random reads")
            unaligned(quiet=False)
        else:
            _run_phases(aligned, unaligned, rank, first + n_al + uhi, self.step_owner)


def run_genome(a, parser_g):
    validate_genome_args(a, parser_g)
    run = _Run(a, ["ref_g", "model_prefix", ("out", a.output), ("number", [a.number]), "coverage", "perfect", "homopolymer", "dna_type",
                   "strandness", "sd_len", "median_len", "max_len", "min_len", "fastq", "chimeric", ("num_threads", max(a.num_threads, 1))])
    rank = run.rank
    if rank == 0:
        log("Read in reference ")
    run.eng = E.Engine(run.device)
    ref = M.read_fasta(a.ref_g, a.dna_type) if rank == 0 else None
    bad = None
    if rank == 0 and len(ref.names) > 1 and a.dna_type == "circular":                         # S:354-356
        bad = "Do not choose circular if there is more than one chromosome in the genome!\n"
    outputs = run.outputs(a.output)
    ref, _ = run.broadcast(ref, outputs=outputs, error=bad)
    with run.scope(outputs):
        mdl = run.load_model(chimeric=a.chimeric)

        def setup(e):
            if run.dev_ptr() is not None:
                e.set_reference_device(run.dev_ptr(), ref)
            else:
                e.set_reference(ref)
            e.load_model(mdl)
        run.set_up(setup)
        n_al, n_un = mdl.split_counts(run.read_number(ref))
        if rank == 0 and a.median_len and a.sd_len:
            log("Simulating read length with log-normal distribution")
        max_len = int(min(a.max_len, ref.max_chrom))                                            # S:2318
        run.simulate(a.output, 0, n_al, n_un,
                     dict(fastq=a.fastq, min_len=a.min_len, max_len=max_len, median_len=a.median_len, sd_len=a.sd_len),
                     dict(chimeric=a.chimeric, kmer_bias=a.KmerBias or 0))


def run_metagenome(a, parser_mg):
    """The metagenome branch of main() (S:2416-2527) + simulation("metagenome") (S:1568-1672).  One ns_generate call plays
    one worker of the reference: it keeps its own per-species base quota (S:835) and numbers its reads consecutively."""
    from . import metagenome as MG
    validate_genome_args(a, parser_mg)
    run = _Run(a, ["genome_list", "abun", "dna_type_list", "model_prefix", ("out", a.output), "perfect", "strandness", "sd_len", "median_len",
                   "max_len", "min_len", "abun_var", "fastq", "chimeric", ("num_threads", max(a.num_threads, 1))])
    rank = run.rank
    run.eng = E.Engine(run.device)
    mref = info = None
    if rank == 0:
        log("Read in reference ")
        mref = MG.read_metagenome(a.genome_list, a.dna_type_list)
        numbers, samples = MG.read_abundance(a.abun, mref.species)
        info = dict(species=mref.species, off=mref.species_chrom_off.tolist(), keys=mref.chrom_names, numbers=numbers, samples=samples)
    if run.dist is not None:
        # sub-files of every sample this rank may write: the sample count is only known after the broadcast, so by pattern and not by
        # shard.clean_parts — ".part<rank>" followed by the end of the name or a dot, so that rank 1 does not take rank 10's files
        import glob
        import re
        tail = re.compile(r"\.part%d(\.|$)" % rank)
        for q in glob.glob(glob.escape(a.output) + "_sample*.part%d*" % rank) if rank else ():
            if tail.search(q):
                os.unlink(q)
        ref, info = run.broadcast(mref.ref if rank == 0 else None, info)
        mref = MG.MetaReference(ref, info["species"], np.array(info["off"], dtype=np.uint32), info["keys"])
        numbers, samples = info["numbers"], info["samples"]
    with run.scope([p for s in range(len(samples)) for p in run.outputs(a.output + "_sample%d" % s)]):
        mdl = run.load_model(chimeric=a.chimeric)

        def setup(e):
            e.set_metagenome(mref, dev_ptr=run.dev_ptr())
            e.load_model(mdl)
        run.set_up(setup)                         # (unaligned reads and gaps take any species: a second engine needs no abundances, S:1708)
        max_len = a.max_len
        total_len = mref.total_len()
        first = 0
        for s, abun in enumerate(samples):
            sample = "sample" + str(s)
            if a.abun_var:                                                                  # S:2497-2506: the species of THIS sample
                sample_len = {sp: total_len[sp] for sp in abun}
                u = np.random.default_rng([run.seed & 0xffffffff, run.seed >> 32, s]).random(len(sample_len))
                abun = MG.add_abundance_var(abun, sample_len, float(a.abun_var[0]), float(a.abun_var[1]), iter(u.tolist()))
            infl = {sp: MG.inflate_abun(abun, sp, mdl.abun_inflation) for sp in abun} if a.chimeric else None   # S:2510-2514
            run.eng.set_abundance(mref, abun, infl)
            if rank == 0:
                log("Simulating sample " + sample)
                if a.median_len and a.sd_len:
                    log("Simulating read length from log-normal distribution")
            n_al, n_un = mdl.split_counts(numbers[s])
            max_len = int(min(max_len, mref.max_chrom))                                     # S:2525
            run.simulate(a.output + "_" + sample, first, n_al, n_un,
                         dict(fastq=a.fastq, min_len=a.min_len, max_len=max_len, median_len=a.median_len, sd_len=a.sd_len, meta=True),
                         dict(chimeric=a.chimeric, kmer_bias=0 if a.perfect else (a.KmerBias or 0)))
            first += n_al + n_un                # samples draw from disjoint read-index ranges of the same seed


def run_transcriptome(a, parser_t):
    """The transcriptome branch of main() (S:2322-2414) + simulation("transcriptome") (S:1568-1672)."""
    from . import intron_retention as IR
    from . import transcriptome as TR
    validate_genome_args(a, parser_t)
    model_ir = a.no_model_ir                                                                  # store_false: True unless --no_model_ir
    run = _Run(a, ["ref_g", "ref_t", "exp", "model_prefix", ("out", a.output), ("number", [a.number]), "coverage", "perfect", "homopolymer",
                   ("model_ir", model_ir), ("dna_type", "transcriptome"), "strandness", "max_len", "min_len", "uracil", "polya"]
               + (["basecaller"] if a.polya else []) + ["fastq", ("num_threads", max(a.num_threads, 1))])
    rank = run.rank
    run.eng = E.Engine(run.device)
    tr = info = None
    if rank == 0:
        log("Read in reference ")
        tr = TR.read_transcriptome(a.ref_t, a.exp, a.polya, a.basecaller)
        info = dict(ec=tr.expr_chrom, cum=tr.expr_cum, w=tr.expr_weight, pa=tr.polya, sc=tr.polya_scale)
    outputs = run.outputs(a.output)
    if run.dist is not None:
        ref, info = run.broadcast(tr.ref if rank == 0 else None, info, outputs)
        tr = TR.TranscriptomeReference(ref, info["ec"], info["cum"], info["w"], info["pa"], info["sc"])
    ir = None
    if model_ir:                                                                              # S:403-452
        if rank == 0:
            log("Read in reference genome, IR markov model and GFF3 annotation file")
        ir = IR.load(a.model_prefix, a.ref_g, tr.ref)
        tr = TR.restrict_expression(tr, ir.eligible)                                          # S:1093-1099
    with run.scope(outputs):
        mdl = run.load_model(transcriptome=True)

        def setup(e, with_ir=True):
            e.set_transcriptome(tr, dev_ptr=run.dev_ptr())
            if ir is not None and with_ir:
                e.set_intron_retention(ir)
            e.load_model(mdl)
        run.set_up(setup, lambda e: setup(e, with_ir=False))                                  # (S:1156: unaligned reads are never spliced)
        n_al, n_un = mdl.split_counts(run.read_number(tr.ref))
        max_len = int(min(a.max_len, tr.ref.max_chrom))                                         # S:2411
        run.simulate(a.output, 0, n_al, n_un, dict(fastq=a.fastq, min_len=a.min_len, max_len=max_len, trx=True, uracil=a.uracil),
                     dict(kmer_bias=a.KmerBias or 0, model_ir=model_ir))


def main(argv=None):
    parser, parser_g, parser_mg, parser_t = build_parser()
    if len(sys.argv if argv is None else argv) == (1 if argv is None else 0):
        parser.print_help(sys.stderr)
        sys.exit(1)
    a = parser.parse_args(argv)
    if getattr(a, "no_merge", False) and getattr(a, "merge", False):
        sys.stderr.write("--merge and --no-merge exclude each other\n")
        sys.exit(1)
    world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    if getattr(a, "no_merge", False):
        os.environ["NS_KEEP_SUBFILES"] = "1"
    elif world > 1 and not getattr(a, "merge", False) and "NS_KEEP_SUBFILES" not in os.environ:
        # several ranks: the parts stay where the ranks wrote them unless --merge asks for the reference's single files (MERGE_HELP)
        os.environ["NS_KEEP_SUBFILES"] = "1"
    if a.mode == "genome":
        run_genome(a, parser_g)
    elif a.mode == "metagenome":
        run_metagenome(a, parser_mg)
    elif a.mode == "transcriptome":
        run_transcriptome(a, parser_t)
    else:
        parser.print_help(sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
