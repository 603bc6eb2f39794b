"""`python -m nanosim_amd.read_analysis` without an engine: what the command line of src/read_analysis.py (R:251-892) does in front of
the work of a mode — the aligner it would have started where an alignment file is missing, its validity checks with their messages
and its parameter blocks, each run in a child process.  No run here comes to the point where an engine is made: the alignment files
of the valid command lines do not exist, which the command says and stops at."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*args, cwd=None):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "nanosim_amd.read_analysis"] + list(args), cwd=cwd or ROOT, env=env, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


def test_version_and_bare_command():
    rc, out, err = run("-v")
    assert rc == 0 and out.strip() == "NanoSim 3.2.2 (nanosim_amd, MI355X)"
    rc, out, err = run()
    assert rc == 1 and "There are five modes in read_analysis." in err
    for mode in ("genome", "transcriptome", "metagenome", "quantify", "detect_ir"):
        rc, out, err = run(mode, "-h")
        assert rc == 0 and out.startswith("usage:")


MINIMAP = "minimap2 --cs -ax %s -t %s %s %s | samtools view -b > %s"


@pytest.mark.parametrize("args, commands", [
    (("genome", "-i", "reads.fq", "-rg", "ref.fa"), [MINIMAP % ("map-ont", "1", "ref.fa", "reads.fq", "training_genome_alnm.bam")]),
    (("genome", "-i", "reads.fa", "-rg", "ref.fa", "-t", "8", "-o", "out/p"), [MINIMAP % ("map-ont", "8", "ref.fa", "reads.fa", "out/p_genome_alnm.bam")]),
    (("genome", "-i", "reads.fa", "-rg", "ref.fa", "-a", "LAST"), ["lastdb ref_genome ref.fa", "lastal -a 1 -P 1 ref_genome reads.fa > training_genome_alnm.maf"]),
    (("metagenome", "-i", "reads.fa", "-gl", "LIST"), [MINIMAP % ("map-ont", "1", "reference_metagenome.fasta", "reads.fa", "training_genome_alnm.bam")]),
    (("transcriptome", "-i", "reads.fa", "-rg", "g.fa", "-rt", "t.fa", "-annot", "a.gff3"),
     [MINIMAP % ("map-ont", "1", "t.fa", "reads.fa", "training_transcriptome_alnm.bam")]),
    (("transcriptome", "-i", "reads.fa", "-rg", "g.fa", "-rt", "t.fa", "-annot", "a.gff3", "-ta", "t.sam"),
     [MINIMAP % ("splice", "1", "g.fa", "reads.fa", "training_genome_alnm.bam")]),
    (("transcriptome", "-i", "reads.fa", "-rg", "g.fa", "-rt", "t.fa", "-annot", "a.gff3", "-a", "LAST"),
     ["lastdb ref_transcriptome t.fa", "lastal -a 1 -P 1 ref_transcriptome reads.fa > training_transcriptome_alnm.maf"]),
    (("quantify", "-e", "trans", "-i", "reads.fa", "-rt", "t.fa"), [MINIMAP % ("map-ont", "1", "t.fa", "reads.fa", "expression_transcriptome_alnm.bam")]),
    (("quantify", "-e", "meta", "-i", "reads.fa", "-gl", "LIST"), [MINIMAP % ("map-ont", "1", "reference_metagenome.fasta", "reads.fa", "expression_genome_alnm.bam")]),
    (("detect_ir", "-annot", "a.gff3", "-i", "reads.fa", "-rg", "g.fa", "-rt", "t.fa", "-ga", "g.sam"),
     [MINIMAP % ("map-ont", "1", "t.fa", "reads.fa", "ir_info_transcriptome_alnm.bam")]),
    (("detect_ir", "-annot", "a.gff3", "-i", "reads.fa", "-rg", "g.fa", "-rt", "t.fa", "-ta", "t.bam"),
     [MINIMAP % ("splice", "1", "g.fa", "reads.fa", "ir_info_genome_alnm.bam")]),
])
def test_a_missing_alignment_file_shows_the_aligner_command_and_stops(args, commands, tmp_path):
    if "LIST" in args:
        (tmp_path / "LIST").write_text("sp A\tspA.fa\t60\nspB\tspB.fa\t40\n")
    rc, out, err = run(*args, cwd=str(tmp_path))
    assert rc == 1 and "This build does not align reads" in out
    assert [x.strip() for x in out.splitlines()[-len(commands):]] == commands
    assert "Traceback" not in err and not any(x.endswith((".hist", ".npz", ".gz")) for x in os.listdir(str(tmp_path)))


FASTA_MSG = "\nFASTA file detected. Please supply reads in FASTQ format (.fastq/.fq/.fastq.gz/.fq.gz).\n\n"
HP_MSG = "\nPlease input proper min homopolymer length value (>= 0) to analyze\n\n"


@pytest.mark.parametrize("args, message, usage", [
    (("genome", "-i", "r.fa", "-ga", "a.txt"), "Please specify an acceptable alignment format! (.maf/.sam/.bam)\n\n", "genome"),
    (("genome", "-i", "r.fa"), "Please supply a reference genome or genome alignment file\n\n", "genome"),
    (("genome", "-i", "r.fa", "-ga", "a.sam", "-hp", "--min_homopolymer_len", "-1"), HP_MSG, "genome"),
    (("genome", "-i", "r.fa", "-ga", "a.sam", "--fastq"), FASTA_MSG, None),
    (("genome", "-i", "r.fasta.gz", "-ga", "a.sam", "--fastq"), FASTA_MSG, None),
    (("metagenome", "-i", "r.fa", "-gl", "l.tsv", "-ga", "a.maf"), "Please specify an acceptable alignment format! (.sam/.bam)\n\n", "genome"),
    (("metagenome", "-i", "r.fa", "-gl", "l.tsv", "-ga", "a.sam", "-hp", "--min_homopolymer_len", "-3"), HP_MSG, "genome"),
    (("metagenome", "-i", "r.fa", "-gl", "l.tsv", "-ga", "a.sam", "--fastq"), FASTA_MSG, None),
    (("transcriptome", "-i", "r.fa", "-rg", "g.fa", "-rt", "t.fa", "-ga", "g.sam", "-ta", "t.bam"),
     "\nPlease provide genome and transcriptome alignments in the same format: sam OR bam OR maf\n\n", "transcriptome"),
    (("transcriptome", "-i", "r.fa", "-rg", "g.fa", "-rt", "t.fa", "-ga", "g.txt", "-ta", "t.txt"),
     "\nPlease provide genome and transcriptome alignments in the same format: sam OR bam OR maf\n\n", "transcriptome"),
    (("transcriptome", "-i", "r.fa", "-rg", "g.fa", "-rt", "t.fa", "-annot", "a.gff3", "-ga", "g.maf", "-ta", "t.maf"),
     "\nThe intron retention only works with sam alignment files for now. Thanks\n\n", "transcriptome"),
    (("transcriptome", "-i", "r.fa", "-rg", "g.fa", "-rt", "t.fa", "-ga", "g.sam", "-ta", "t.sam"),
     "\nPlease also input reference genome and annotation file for Intron Retention modeling\n\n", "transcriptome"),
    (("transcriptome", "-i", "r.fa", "-rg", "g.fa", "-rt", "t.fa", "--no_intron_retention", "-ga", "g.sam", "-ta", "t.sam", "-hp", "--min_homopolymer_len", "-1"),
     HP_MSG, "genome"),
    (("transcriptome", "-i", "r.fa", "-rg", "g.fa", "-rt", "t.fa", "--no_intron_retention", "-ga", "g.sam", "-ta", "t.sam", "--fastq"), ".fa\n" + FASTA_MSG, None),
    (("quantify", "-e", "trans", "-i", "r.fa", "-ta", "t.maf"), None, "genome"),
    (("quantify", "-e", "meta", "-i", "r.fa", "-ga", "g.txt"), None, "genome"),
    (("detect_ir", "-annot", "a.gff3"), "Please supply a reference genome or genome alignment file\n\n", "detect_ir"),
    (("detect_ir", "-annot", "a.gff3", "-ga", "g.sam"), "Please supply a reference transcriptome or transcriptome alignment file\n\n", "detect_ir"),
    (("detect_ir", "-annot", "a.gff3", "-ga", "g.txt", "-ta", "t.sam"), "Please specify an acceptable alignment format! (.maf/.sam /.bam)\n\n", "detect_ir"),
    (("detect_ir", "-annot", "a.gff3", "-ga", "g.sam", "-ta", "t.txt"), "Please specify an acceptable alignment format! (.maf/.sam/.bam)\n\n", "detect_ir"),
])
def test_validity_checks_print_the_references_messages_and_exit_1(args, message, usage, tmp_path):
    rc, out, err = run(*args, cwd=str(tmp_path))
    assert rc == 1
    if message is None:                                     # (quantify checks behind its parameter block)
        assert out.endswith("Please specify an acceptable alignment format! (.sam/.bam)\n\n") and out.startswith("\nrunning the code with following parameters\n")
    else:
        assert out == message
    assert (("usage: read_analysis.py %s " % usage) in err.replace("__main__.py", "read_analysis.py").replace("python -m nanosim_amd.read_analysis", "read_analysis.py")) \
        if usage else err == ""
    assert os.listdir(str(tmp_path)) == []


def test_maf_with_fastq_stops_before_any_work(tmp_path):
    for args in (("genome", "-i", "r.fq", "-ga", "a.maf", "--fastq"), ("genome", "-i", "r.fastq.gz", "-ga", "a.maf")):
        rc, out, err = run(*args, cwd=str(tmp_path))
        assert rc == 1 and err == "Currently, base quality model parameter estimation cannot be performed on alignments in MAF format.\n"
        assert os.listdir(str(tmp_path)) == []


BLOCKS = {
    ("genome", "-i", "r.fq", "-rg", "g.fa", "-ga", "a.bam", "-c", "-hp", "--fastq", "-o", "d/p", "-t", "4"):
        ["", "Running the code with following parameters:", "", "infile r.fq", "ref_g g.fa", "aligner minimap2", "g_alnm a.bam", "prefix d/p", "num_threads 4",
         "model_fit True", "chimeric True", "homopolymer True", "min_homopolymer_len 5", "fastq True"],
    ("genome", "-i", "r.fa", "-ga", "a.sam", "--no_model_fit", "-a", "LAST"):
        ["", "Running the code with following parameters:", "", "infile r.fa", "ref_g ", "aligner LAST", "g_alnm a.sam", "prefix training", "num_threads 1",
         "model_fit False", "chimeric False", "homopolymer False", "fastq False"],
    ("metagenome", "-i", "r.fa", "-gl", "l.tsv", "-ga", "a.sam", "-c", "-q"):
        ["", "Running the code with following parameters:", "", "infile r.fa", "genome_list l.tsv", "g_alnm a.sam", "prefix training", "num_threads 1",
         "model_fit True", "chimeric True", "fastq False", "quantification True"],
    ("transcriptome", "-i", "r.fa", "-rg", "g.fa", "-rt", "t.fa", "-annot", "a.gff3", "-ga", "g.sam", "-ta", "t.sam", "-hp", "-q", "-n"):
        ["", "running the code with following parameters:", "", "infile r.fa", "ref_g g.fa", "ref_t t.fa", "annot a.gff3", "aligner minimap2", "g_alnm g.sam",
         "t_alnm t.sam", "prefix training", "num_threads 1", "model_fit True", "intron_retention True", "homopolymer True", "min_homopolymer_len 5", "fastq False",
         "quantification True", "normalize by transcript length True"],
    ("quantify", "-e", "trans", "-i", "r.fa", "-ta", "t.sam", "-n"):
        ["", "running the code with following parameters", "", "mode trans", "infile r.fa", "ref_t ", "genome_list ", "g_alnm ", "t_aln, t.sam", "prefix expression",
         "num_threads 1", "normalize by transcript length True"],
    ("detect_ir", "-annot", "a.gff3", "-ga", "g.sam", "-ta", "t.sam"):
        ["", "running the code with following parameters:", "", "annot a.gff3", "infile ", "aligner minimap2", "ref_g ", "ref_t ", "g_alnm g.sam", "t_alnm t.sam",
         "prefix ir_info"],
}


@pytest.mark.parametrize("args", list(BLOCKS))
def test_parameter_block_of_a_valid_command_line(args, tmp_path):
    if "l.tsv" in args:
        (tmp_path / "l.tsv").write_text("spA\tspA.fa\t60\nspB\tspB.fa\t40\n")
    rc, out, err = run(*args, cwd=str(tmp_path))
    lines = out.split("\n")
    assert lines[:len(BLOCKS[args])] == BLOCKS[args]
    assert rc == 1 and lines[-2].startswith("No such file: ") and "Traceback" not in err      # (the alignment file is not there: no engine is made)
    assert ("d" in os.listdir(str(tmp_path))) == ("d/p" in args)
