"""simulator.main end to end on the CPU, every mode under every schedule, with a recording stand-in for engine.Engine: which tables each
engine context gets, which worker calls it serves, what reaches which file, what the log says, and that every engine is closed once.
The expectations are worked out here from mdl.split_counts, shard.partition and _step_batches — what the three run_* functions have
in common must not change what any of them does."""
import os
import re
import sys

import pytest

from nanosim_amd import engine as E
from nanosim_amd import model as M
from nanosim_amd import shard, simulator
from tests.fake_engine import EngineWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = "tests/golden/model_small/training"                # (relative: every run has its cwd at the repository root)
META = ["-gl", "tests/golden/meta/genome_list.tsv", "-a", "tests/golden/meta/abundance.tsv", "-dl", "tests/golden/meta/dna_type_list.tsv"]
TRX = ["-rt", "tests/golden/trx/transcripts.fa", "-e", "tests/golden/trx/expression.tsv"]
N = 16000                                                   # 15 200 + 800 reads: both phases span several batches of 700
BATCH = 700

CASES = {
    "genome": ["genome", "-rg", "tests/golden/genome_small.fa", "-n", str(N), "--chimeric", "-t", "3"],
    "genome_perfect": ["genome", "-rg", "tests/golden/genome_small.fa", "-n", str(N), "--perfect"],
    "metagenome": ["metagenome"] + META + ["--chimeric", "--fastq", "-t", "3"],
    "transcriptome": ["transcriptome"] + TRX + ["-n", str(N), "--no_model_ir", "--uracil", "--fastq", "--polya", "tests/golden/trx/polya.txt",
                                                "-b", "guppy"],
    "transcriptome_ir": ["transcriptome"] + TRX + ["-n", str(N), "-rg", "tests/golden/trx/genome.fa"],
    # what --perfect does with -k differs between the modes (genome hands it on, the metagenome worker gets 0)
    "genome_perfect_k": ["genome", "-rg", "tests/golden/genome_small.fa", "-n", "1500", "--perfect", "-hp", "-k", "5"],
    "metagenome_perfect_k": ["metagenome"] + META + ["--perfect", "-hp", "-k", "5"],
}
SCHEDULES = {"step": {}, "serial": {"NS_SERIAL": "1"}, "two_engines": {"NS_TWO_ENGINES": "1"}}


def _run(argv, tmp_path, monkeypatch, schedule="serial", world=None, batch=BATCH):
    """main(argv + -c, -o, --seed) with its cwd at the repository root; returns (the engines' world, output directory, names given to
    shard.subfile_path)"""
    world = world or EngineWorld()
    sub_files = []
    real_subfile_path = shard.subfile_path
    monkeypatch.setattr(E, "Engine", world)
    monkeypatch.setattr(shard, "subfile_path", lambda p, tag: sub_files.append(real_subfile_path(p, tag)) or sub_files[-1])
    monkeypatch.setattr(simulator, "BATCH_READS", batch)
    monkeypatch.setattr(sys, "argv", ["simulator"])
    for k in ("NS_SERIAL", "NS_TWO_ENGINES", "NS_KEEP_SUBFILES", "NS_CLI_TRACE", "NS_CLI_DROP_OUTPUT", "NS_FORCE_DIST", "RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in SCHEDULES[schedule].items():
        monkeypatch.setenv(k, v)
    monkeypatch.chdir(ROOT)
    simulator.main(argv + ["-c", PREFIX, "-o", str(tmp_path / "run" / "sim"), "--seed", "31"])
    return world, tmp_path / "run", sub_files


def _expected(case):
    """per sample of the run: (output base, first read, n_al, n_un); and the fields every request of the run shares"""
    argv = CASES[case]
    perfect, fastq = "--perfect" in argv, "--fastq" in argv
    kw = dict(perfect=perfect, fastq=fastq, homopolymer="-hp" in argv)
    if argv[0] == "genome":
        mdl = M.load_model(PREFIX, chimeric="--chimeric" in argv, **kw)
        max_len = M.read_fasta("tests/golden/genome_small.fa", "linear").max_chrom
        numbers = [int(argv[argv.index("-n") + 1])]
    elif argv[0] == "metagenome":
        from nanosim_amd import metagenome as MG
        mdl = M.load_model(PREFIX, chimeric="--chimeric" in argv, **kw)
        mref = MG.read_metagenome(META[1], META[5])
        max_len = mref.max_chrom
        numbers = MG.read_abundance(META[3], mref.species)[0]
        assert list(numbers) == [3000, 500]
    else:
        from nanosim_amd import transcriptome as TR
        mdl = M.load_model(PREFIX, transcriptome=True, **kw)
        max_len = TR.read_transcriptome(TRX[1], TRX[3], None, None).ref.max_chrom
        numbers = [N]
    samples, first = [], 0
    for s, number in enumerate(numbers):
        n_al, n_un = mdl.split_counts(number)
        samples.append(("sim_sample%d" % s if argv[0] == "metagenome" else "sim", first, n_al, n_un))
        first += n_al + n_un
    meta, trx = argv[0] == "metagenome", argv[0] == "transcriptome"
    common = dict(fastq=int(fastq), min_len=50, max_len=int(max_len), meta=int(meta), trx=int(trx), uracil=int("--uracil" in argv))
    aligned = dict(common, kind=E.NS_KIND_PERFECT if perfect else E.NS_KIND_ALIGNED, chimeric=int("--chimeric" in argv), emit_errlog=1,
                   kmer_bias=5 if "-k" in argv and not (meta and perfect) else 0, model_ir=int(trx and "--no_model_ir" not in argv))
    unaligned = dict(common, kind=E.NS_KIND_UNALIGNED, chimeric=0, emit_errlog=0, kmer_bias=0, model_ir=0)
    return samples, aligned, unaligned, ".fastq" if fastq else ".fasta"


def _requests(fields, first, count, batch):
    """the worker calls of one phase of one rank: reads [first, first + count) in calls of `batch`"""
    from tests.fake_engine import REQUEST_FIELDS
    out, done = [], 0
    while done < count:
        n = min(batch, count - done)
        out.append(tuple(dict(fields, first_read=first + done, n_reads=n)[f] for f in REQUEST_FIELDS))
        done += n
    return out


def _phase_requests(case, schedule, batch=BATCH):
    """per sample of the run: (aligned requests, unaligned requests), each in order; world size 1"""
    samples, aligned, unaligned, _ = _expected(case)
    perfect = "--perfect" in CASES[case]
    out = []
    for _, first, n_al, n_un in samples:
        b_al = b_un = batch
        if schedule != "serial" and not perfect and CASES[case][0] != "metagenome":      # a metagenome worker call keeps its own quotas:
            b_al, b_un = (min(batch, b) for b in simulator._step_batches(n_al, n_un))      # its batches are never the step's shares
        lo, hi = shard.partition(n_al, 1)[0]
        ulo, uhi = shard.partition(n_un, 1)[0]
        out.append((_requests(aligned, first + lo, hi - lo, b_al),
                    [] if perfect else _requests(unaligned, first + n_al + ulo, uhi - ulo, b_un)))
    return out


def _setup_calls(case, schedule):
    """(setup of the first engine, setup of the second engine or None, setup of the companion or None)"""
    argv = CASES[case]
    perfect = "--perfect" in argv
    mode = {"genome": [("set_reference", ())], "metagenome": [("set_metagenome", ("dev_ptr",))],
            "transcriptome": [("set_transcriptome", ("dev_ptr",))]}[argv[0]]
    ir = [("set_intron_retention", ())] if argv[0] == "transcriptome" and "--no_model_ir" not in argv else []
    model = [("load_model", ())]
    n_samples = 2 if argv[0] == "metagenome" else 1
    step = schedule == "step" and not perfect
    first = mode + ir + model + ([("step_engine", ())] if step else [])          # (_background_engine asks for the companion)
    for _ in range(n_samples):
        if argv[0] == "metagenome":
            first.append(("set_abundance", ()))                                 # once per sample, on the owner only
        if step:
            first.append(("step_engine", ()))                                   # (the StepPair of this sample's phases)
    second = [("set_background", ())] + mode + model if schedule == "two_engines" and not perfect else None    # no intron retention
    return first, second, [] if step else None


def _file_bytes(lo, hi, err=False):
    return b"".join((b"read_%d\t0\tmis\t1\tA\tC\n" if err else b">read_%d\nACGT\n") % i for i in range(lo, hi))


def _check_run(case, schedule, world, out_dir, sub_files):
    samples, _, _, ext = _expected(case)
    perfect = "--perfect" in CASES[case]
    per_sample = _phase_requests(case, schedule)
    al, un = sum((x for x, _ in per_sample), []), sum((x for _, x in per_sample), [])
    first, second, companion = _setup_calls(case, schedule)
    engines = world.created
    assert len(engines) == 1 + (second is not None) + (companion is not None)
    assert engines[0].setup == first and engines[0].background is None
    if schedule == "serial" or perfect:
        assert engines[0].requests == sum((x + y for x, y in per_sample), [])        # sample after sample, each aligned then unaligned
    else:
        other = engines[1]
        assert other.setup == (second if second is not None else companion)
        assert other.background is (True if second is not None else None)
        assert (other.owner is engines[0]) == (companion is not None)
        # each phase in its order on its own context (a step: its aligned request here, its unaligned one on the companion); how the
        # requests of the two phases interleave depends on timing and is not part of the result
        assert engines[0].requests == al and other.requests == un
    # every engine and companion closed once, the one of the unaligned calls before the first
    assert world.closed == engines[::-1]
    # the files: exactly the requested read ranges, in order
    names = []
    for base, f0, n_al, n_un in samples:
        names += [base + "_aligned_error_profile", base + "_aligned_reads" + ext] + ([] if perfect else [base + "_unaligned_reads" + ext])
        assert (out_dir / (base + "_aligned_reads" + ext)).read_bytes() == _file_bytes(f0, f0 + n_al)
        assert (out_dir / (base + "_aligned_error_profile")).read_bytes() == simulator.ERR_HEADER + _file_bytes(f0, f0 + n_al, err=True)
        if not perfect:
            assert (out_dir / (base + "_unaligned_reads" + ext)).read_bytes() == _file_bytes(f0 + n_al, f0 + n_al + n_un)
    assert sorted(os.listdir(out_dir)) == sorted(names)
    # -t 3: genome and transcriptome batches go through three sub-files per output, a metagenome run creates none
    if "-t" in CASES[case] and CASES[case][0] != "metagenome":
        assert len(sub_files) == 3 * (2 * len(al) + len(un))
    else:
        assert sub_files == []


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("case", [c for c in CASES if not c.endswith("_k")])
def test_mode_under_schedule(case, schedule, tmp_path, monkeypatch):
    _check_run(case, schedule, *_run(CASES[case], tmp_path, monkeypatch, schedule))


@pytest.mark.parametrize("case", [c for c in CASES if c.endswith("_k")])
def test_perfect_with_kmer_bias(case, tmp_path, monkeypatch):
    world, out_dir, sub_files = _run(CASES[case], tmp_path, monkeypatch)
    _check_run(case, "serial", world, out_dir, sub_files)
    assert {r[5] for r in world.created[0].requests} == {5 if case.startswith("genome") else 0}      # kmer_bias


def test_metagenome_batches_are_not_the_step_shares(tmp_path, monkeypatch):
    """at 700 reads _step_batches' floor of 1000 hides the difference; at 2500 a step's aligned share would be 2375 reads, and a
    metagenome worker call still takes 2500: it keeps its own species quotas, so the batches are part of the result"""
    monkeypatch.setattr(simulator, "BATCH_READS", 2500)
    assert simulator._step_batches(2850, 150) == (2375, 1000)
    world, _, _ = _run(CASES["metagenome"], tmp_path, monkeypatch, "step", batch=2500)
    (al0, un0), (al1, un1) = _phase_requests("metagenome", "step", batch=2500)
    al, un = al0 + al1, un0 + un1
    assert [r[:2] for r in al] == [(0, 2500), (2500, 350), (3000, 475)]
    assert world.created[0].requests == al and world.created[1].requests == un


def _progress(first, count):
    """the progress line of one phase: rewritten in place after every worker call"""
    return "".join("<t>: Number of reads simulated >> %d\r" % (first + min(done + BATCH, count)) for done in range(0, count, BATCH))


def _head(*fields):
    return ["", "running the code with following parameters:", ""] + list(fields) + ["<t>: simulator", "<t>: Read in reference "]


_GENOME = ("ref_g tests/golden/genome_small.fa", "model_prefix tests/golden/model_small/training", "out <tmp>/run/sim", "number [16000]",
           "coverage None")
_GENOME_TAIL = ("dna_type linear", "strandness None", "sd_len None", "median_len None", "max_len inf", "min_len 50", "fastq False")
_TRX = ("ref_t tests/golden/trx/transcripts.fa", "exp tests/golden/trx/expression.tsv", "model_prefix tests/golden/model_small/training",
        "out <tmp>/run/sim", "number [16000]", "coverage None", "perfect False", "homopolymer False")
_TWO_PHASES = ["<t>: Read error profile", "<t>: Start simulation of aligned reads", _progress(0, 15200), "<t>: Start simulation of random reads",
               _progress(15200, 800), "<t>: Finished!", ""]
LOGS = {
    "genome": _head(*_GENOME, "perfect False", "homopolymer False", *_GENOME_TAIL, "chimeric True", "num_threads 3") + _TWO_PHASES,
    "genome_perfect": _head(*_GENOME, "perfect True", "homopolymer False", *_GENOME_TAIL, "chimeric False", "num_threads 1") + [
        "<t>: Read KDF of aligned reads", "<t>: Start simulation of aligned reads", _progress(0, 16000), "<t>: Finished!", ""],
    "metagenome": _head("genome_list tests/golden/meta/genome_list.tsv", "abun tests/golden/meta/abundance.tsv",
                        "dna_type_list tests/golden/meta/dna_type_list.tsv", "model_prefix tests/golden/model_small/training",
                        "out <tmp>/run/sim", "perfect False", "strandness None", "sd_len None", "median_len None", "max_len inf", "min_len 50",
                        "abun_var None", "fastq True", "chimeric True", "num_threads 3") + [
        "<t>: Read error profile",
        "<t>: Simulating sample sample0", "<t>: Start simulation of aligned reads", _progress(0, 2850),
        "<t>: Start simulation of random reads", _progress(2850, 150),
        "<t>: Simulating sample sample1", "<t>: Start simulation of aligned reads", _progress(3000, 475),
        "<t>: Start simulation of random reads", _progress(3475, 25), "<t>: Finished!", ""],
    "transcriptome": _head("ref_g ", *_TRX, "model_ir False", "dna_type transcriptome", "strandness None", "max_len inf", "min_len 50",
                           "uracil True", "polya tests/golden/trx/polya.txt", "basecaller guppy", "fastq True", "num_threads 1") + _TWO_PHASES,
    "transcriptome_ir": _head("ref_g tests/golden/trx/genome.fa", *_TRX, "model_ir True", "dna_type transcriptome", "strandness None",
                              "max_len inf", "min_len 50", "uracil False", "polya None", "fastq False", "num_threads 1") + [
        "<t>: Read in reference genome, IR markov model and GFF3 annotation file"] + _TWO_PHASES,
}


@pytest.mark.parametrize("case", list(LOGS))
def test_serial_log(case, tmp_path, monkeypatch, capsys):
    _run(CASES[case], tmp_path, monkeypatch)
    out = capsys.readouterr().out.replace(str(tmp_path), "<tmp>")
    got = re.sub(r"\d{4}-\d\d-\d\d \d\d:\d\d:\d\d", "<t>", out).split("\n")
    assert got == LOGS[case]


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_failed_worker_call_closes_every_engine_and_leaves_main(schedule, tmp_path, monkeypatch):
    world = EngineWorld(fail_generate_at=2)
    with pytest.raises(RuntimeError, match="device lost"):
        _run(CASES["genome"], tmp_path, monkeypatch, schedule, world)
    assert len(world.created) == (1 if schedule == "serial" else 2) and world.closed == world.created[::-1]


K_MESSAGE = "\n-k/--KmerBias needs -hp (the reference crashes on the missing homopolymer parameters, S:504,639)\n"
EXITS = {
    "genome_k": (["genome", "-rg", "tests/golden/genome_small.fa", "-k", "5"], K_MESSAGE, ""),
    "metagenome_k": (["metagenome"] + META + ["-k", "5"], K_MESSAGE, ""),
    "transcriptome_k": (["transcriptome"] + TRX + ["--no_model_ir", "-k", "5"], K_MESSAGE, ""),
    "transcriptome_no_rg": (["transcriptome"] + TRX, "\nPlease provide a reference genome to simulate intron retention events!\nusage: ", ""),
    "transcriptome_polya": (["transcriptome"] + TRX + ["--no_model_ir", "--polya", "tests/golden/trx/polya.txt"], "usage: ",
                            "\nPlease input basecaller to simulate polyA tails from.\n"),
    "transcriptome_max_len": (["transcriptome"] + TRX + ["--no_model_ir", "-max", "40"],
                              "\nMaximum read length must be longer than Minimum read length!\nusage: ", ""),
}


@pytest.mark.parametrize("case", list(EXITS))
def test_early_exit_before_any_engine(case, tmp_path, monkeypatch, capsys):
    argv, err_start, out = EXITS[case]
    world = EngineWorld()
    with pytest.raises(SystemExit) as e:
        _run(argv, tmp_path, monkeypatch, world=world)
    assert e.value.code == 1 and world.created == []
    cap = capsys.readouterr()
    assert cap.err.startswith(err_start) and cap.out == out
    if err_start == K_MESSAGE:
        assert cap.err == K_MESSAGE
    assert not (tmp_path / "run").exists()
