"""`python -m nanosim_amd.read_analysis` on the GPU, every mode once, each in a fresh child process: the files the command writes equal
what the documented stage calls of characterize/__init__.py write when they are made by hand with the PATH readers (by_hand of
tests/test_training_modes.py, on this process's engine) — byte for byte, `_kde.npz` array by array.  The inputs are the composed ones
of tests/test_training_modes.py: a few hundred records with cs, MD, NM, SA, SEQ and QUAL."""
import os
import shutil
import subprocess
import sys

import pytest

from nanosim_amd import engine as EN
from nanosim_amd import model
from tests import test_besthit
from tests.test_training_modes import by_hand, genome_inputs, prefixes, same_files, transcriptome_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0)
    yield e
    e.close()


def cli(*args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "nanosim_amd.read_analysis"] + list(args), cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith(": Finished!")
    return r.stdout


def test_gpu_cli_chimeric_homopolymer_fastq_from_sam_and_from_bam(eng, tmp_path):
    inp = genome_inputs(tmp_path)
    got, want = prefixes(tmp_path)
    by_hand("genome -c -hp --fastq", want, eng, inp)
    for key in ("sam", "bam"):
        out = cli("genome", "-i", inp["reads"], "-ga", inp[key], "-o", got, "-c", "-hp", "--fastq", cwd=str(tmp_path))
        assert "Processing alignment file: " + key in out
        names = same_files(got, want)
        assert {"_primary.sam", "_kde.npz", "_chimeric_info", "_model_profile", "_base_qualities_model_parameters.tsv", "_processed.maf"} <= set(names)
        model.load_model(got, chimeric=True)
        shutil.rmtree(os.path.dirname(got))


def test_gpu_cli_without_chimeric_the_primary_lines_are_written(eng, tmp_path):
    inp = genome_inputs(tmp_path)
    got, want = prefixes(tmp_path)
    by_hand("genome", want, eng, inp)
    cli("genome", "-i", inp["reads"], "-ga", inp["sam"], "-o", got, cwd=str(tmp_path))
    same_files(got, want)
    lines = inp["text"].splitlines(True)
    with open(got + "_primary.sam") as f:
        assert f.read() == "".join(x for x in lines if x.startswith("@")) + "".join(x for x in lines if not x.startswith("@") and not int(x.split("\t")[1]) & 0x904)
    model.load_model(got)


def test_gpu_cli_a_maf_alignment(eng, tmp_path):
    fx = test_besthit.load_fixture()
    test_besthit.check_training(eng, fx, tmp_path)                              # (what the call in this process leaves under <tmp>/training)
    maf_path, reads_path = test_besthit.write_inputs(fx, tmp_path)
    os.makedirs(str(tmp_path / "got"))
    got = str(tmp_path / "got" / "training")
    shutil.copy(os.path.join(ROOT, "tests", "golden", "model_small", "training_model_profile"), got + "_model_profile")
    cli("genome", "-i", reads_path, "-ga", maf_path, "-o", got, "--no_model_fit", cwd=str(tmp_path))
    assert "_besthit.maf" in same_files(got, str(tmp_path / "training"))


def test_gpu_cli_metagenome_chimeric_quantification(eng, tmp_path):
    inp = genome_inputs(tmp_path)
    got, want = prefixes(tmp_path)
    by_hand("metagenome -c -q", want, eng, inp)
    cli("metagenome", "-i", inp["reads"], "-gl", inp["list"], "-ga", inp["sam"], "-o", got, "-c", "-q", cwd=str(tmp_path))
    assert "_quantification.tsv" in same_files(got, want)


@pytest.mark.parametrize("ir", [True, False])
def test_gpu_cli_transcriptome(eng, tmp_path, ir):
    inp = transcriptome_inputs(tmp_path)
    got, want = prefixes(tmp_path)
    by_hand("transcriptome" if ir else "transcriptome --no_intron_retention", want, eng, inp)
    out = cli("transcriptome", "-i", inp["reads"], "-rg", "g.fa", "-rt", "t.fa", "-annot", inp["annot"], "-ga", inp["g"], "-ta", inp["t"], "-o", got,
              *(() if ir else ("--no_intron_retention",)), cwd=str(tmp_path))
    assert ("_IR_markov_model" in same_files(got, want)) == ir
    stages = [x.split(": ", 1)[1] for x in out.splitlines() if x[:2] == "20" and ": " in x]
    assert stages == ["Read pre-process and unaligned reads analysis", "Processing transcriptome alignment file: sam", "Processing genome alignment file: sam"] + \
        (["Parse the annotation file (GTF/GFF3)", "Modeling Intron Retention"] if ir else []) + \
        ["Aligned reads analysis", "Unaligned reads analysis", "match and error models", "Model fitting", "Finished!"]


def test_gpu_cli_quantify_and_detect_ir(eng, tmp_path):
    inp = dict(genome_inputs(tmp_path), **{k: v for k, v in transcriptome_inputs(tmp_path).items() if k != "reads"})
    got, want = prefixes(tmp_path)
    by_hand("quantify -e meta", want, eng, inp)
    cli("quantify", "-e", "meta", "-i", inp["reads"], "-gl", inp["list"], "-ga", inp["sam"], "-o", got, cwd=str(tmp_path))
    assert same_files(got, want) == ["_quantification.tsv"]
    by_hand("quantify -e trans", want, eng, inp)
    cli("quantify", "-e", "trans", "-i", inp["reads"], "-ta", inp["sam"], "-o", got, cwd=str(tmp_path))
    assert same_files(got, want) == ["_quantification.tsv"]
    by_hand("detect_ir", want, eng, inp)
    cli("detect_ir", "-annot", inp["annot"], "-ga", inp["g"], "-ta", inp["t"], "-o", got, cwd=str(tmp_path))
    assert same_files(got, want) == ["_IR_info", "_IR_markov_model", "_added_intron_final.gff3", "_quantification.tsv"]
