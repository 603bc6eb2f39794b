"""`python -m nanosim_amd.read_analysis`: the command line of the reference's read_analysis.py (src/read_analysis.py, R:251-892) over
the training side of this package — the same five modes, flags, defaults, help texts, validity checks and parameter blocks — for
alignments that exist: `-ga` / `-ta` name SAM, BAM or (genome mode) MAF files, and the work of a mode is one function of
nanosim_amd.characterize (train_genome, train_metagenome, train_transcriptome, quantify_reads, detect_ir).

Nothing is aligned.  Where the reference would start minimap2 or LAST because an alignment file is missing, this command
prints the command line the reference would have run and exits with status 1, before an engine exists.  The pre-processed copy of the
reads and the concatenated metagenome, which the reference writes only to align them, are not written.  `-t` and `-a` are accepted and
printed; `-a` otherwise only chooses the aligner command that is shown."""
import argparse
import os
import sys
from textwrap import dedent
from time import strftime

VERSION = "3.2.2"
READ_FORMATS = (".fastq", ".fq")

MSG_FORMAT_MSB = "Please specify an acceptable alignment format! (.maf/.sam/.bam)\n"
MSG_FORMAT_MSB_IR = "Please specify an acceptable alignment format! (.maf/.sam /.bam)\n"        # (the blank is the reference's, R:486)
MSG_FORMAT_SB = "Please specify an acceptable alignment format! (.sam/.bam)\n"
MSG_NEED_G = "Please supply a reference genome or genome alignment file\n"
MSG_NEED_T = "Please supply a reference transcriptome or transcriptome alignment file\n"
MSG_NEED_G_IR = "For intron retention function, please supply a reference genome or genome alignment file\n"
MSG_SAME_FORMAT = "\nPlease provide genome and transcriptome alignments in the same format: sam OR bam OR maf\n"
MSG_IR_MAF = "\nThe intron retention only works with sam alignment files for now. Thanks\n"
MSG_IR_NEEDS = "\nPlease also input reference genome and annotation file for Intron Retention modeling\n"
MSG_HP_LEN = "\nPlease input proper min homopolymer length value (>= 0) to analyze\n"
MSG_FASTA = "\nFASTA file detected. Please supply reads in FASTQ format (.fastq/.fq/.fastq.gz/.fq.gz).\n"
MSG_MAF_QUAL = "Currently, base quality model parameter estimation cannot be performed on alignments in MAF format.\n"
HELP_GENOME_LIST = ('Reference metagenome list, tsv file, the first column is species/strain name, the second column is the reference genome '
                    'fasta/fastq file directory, the third column is optional, if provided, it contains the expected abundance (sum up to 100)')
HELP_GA_META = 'Genome alignment file in sam format, the header of each species should match the metagenome list provided above (optional)'
HELP_THREADS_FIT = 'Number of threads for alignment and model fitting (Default = 1)'
HELP_OUTPUT = 'The location and prefix of outputting profiles (Default = training)'


def log(stage: str) -> None:
    sys.stdout.write(strftime("%Y-%m-%d %H:%M:%S") + ": " + stage + "\n")
    sys.stdout.flush()


def build_parser():
    """(the parser, {mode: its sub-parser}) with the reference's flags, defaults and help (R:252-381)"""
    parser = argparse.ArgumentParser(
        description=dedent('''
        Read characterization step
        -----------------------------------------------------------
        Given raw ONT reads, reference genome, metagenome, and/or
        transcriptome, learn read features and output error profiles
        '''),
        formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('-v', '--version', action='version', version='NanoSim ' + VERSION + ' (nanosim_amd, MI355X)')
    sub = parser.add_subparsers(dest='mode', description=dedent('''
        There are five modes in read_analysis.
        For detailed usage of each mode:
            read_analysis.py mode -h
        -------------------------------------------------------
        '''))
    flag = dict(action='store_true', default=False)
    off = dict(action='store_false', default=True)
    modes = {}

    g = modes["genome"] = sub.add_parser('genome', help="Run the simulator on genome mode")
    g.add_argument('-i', '--read', help='Input read for training', required=True)
    g.add_argument('-rg', '--ref_g', help='Reference genome, not required if genome alignment file is provided', default='')
    g.add_argument('-a', '--aligner', help='The aligner to be used, minimap2 or LAST (Default = minimap2)', choices=['minimap2', 'LAST'], default='minimap2')
    g.add_argument('-ga', '--g_alnm', help='Genome alignment file in SAM/BAM format (optional)', default='')
    g.add_argument('-o', '--output', help=HELP_OUTPUT, default='training')
    g.add_argument('-c', '--chimeric', help='Detect chimeric and split reads (Default = False)', **flag)
    g.add_argument('-hp', '--homopolymer', help='Analyze homopolymer lengths (Default = False)', **flag)
    g.add_argument('--min_homopolymer_len', help='Minimum length of homopolymers to analyze (Default = 5 bp)', default='5')
    g.add_argument('--fastq', help='Analyze base qualities (Default = False)', **flag)
    g.add_argument('--no_model_fit', help='Disable model fitting step', **off)
    g.add_argument('-t', '--num_threads', help=HELP_THREADS_FIT, default='1')

    t = modes["transcriptome"] = sub.add_parser('transcriptome', help="Run the simulator on transcriptome mode")
    t.add_argument('-i', '--read', help='Input read for training', required=True)
    t.add_argument('-rg', '--ref_g', help='Reference genome', required=True)
    t.add_argument('-rt', '--ref_t', help='Reference Transcriptome', required=True)
    t.add_argument('-annot', '--annotation', help='Annotation file in ensemble GTF/GFF formats, required for intron retention detection', default='')
    t.add_argument('-a', '--aligner', help='The aligner to be used: minimap2 or LAST (Default = minimap2)', choices=['minimap2', 'LAST'], default='minimap2')
    t.add_argument('-ga', '--g_alnm', help='Genome alignment file in SAM/BAM format (optional)', default='')
    t.add_argument('-ta', '--t_alnm', help='Transcriptome alignment file in SAM/BAM format (optional)', default='')
    t.add_argument('-o', '--output', help=HELP_OUTPUT, default='training')
    t.add_argument('--no_model_fit', help='Disable model fitting step', **off)
    t.add_argument('--no_intron_retention', help='Disable Intron Retention analysis', **off)
    t.add_argument('-t', '--num_threads', help=HELP_THREADS_FIT, default='1')
    t.add_argument('-c', '--chimeric', help=argparse.SUPPRESS, **flag)
    t.add_argument('-q', '--quantification', help='Perform abundance quantification (Default = False)', **flag)
    t.add_argument('-n', '--normalize', help='Normalize by transcript length', **flag)
    t.add_argument('-hp', '--homopolymer', help='Analyze homopolymer lengths (Default = False', **flag)
    t.add_argument('--min_homopolymer_len', help='Minimum length of homopolymers to analyze (Default = 5 bp)', default='5')
    t.add_argument('--fastq', help='Analyze base qualities (Default = False)', **flag)

    m = modes["metagenome"] = sub.add_parser('metagenome', help="Run the simulator on metagenome mode")
    m.add_argument('-i', '--read', help='Input read for training', required=True)
    m.add_argument('-gl', '--genome_list', help=HELP_GENOME_LIST, required=True)
    m.add_argument('-ga', '--g_alnm', help=HELP_GA_META, default='')
    m.add_argument('-o', '--output', help=HELP_OUTPUT, default='training')
    m.add_argument('-c', '--chimeric', help='Detect chimeric and split reads (Default = False)', **flag)
    m.add_argument('-q', '--quantification', help='Perform abundance quantification and compute the deviation between calculated abundance and '
                                                  'expected values (Default = False)', **flag)
    m.add_argument('-hp', '--homopolymer', help=argparse.SUPPRESS, **flag)
    m.add_argument('--min_homopolymer_len', help=argparse.SUPPRESS, default='5')
    m.add_argument('--fastq', help='Analyze base qualities (Default = False)', **flag)
    m.add_argument('--no_model_fit', help='Disable model fitting step', **off)
    m.add_argument('-t', '--num_threads', help=HELP_THREADS_FIT, default='1')

    e = modes["quantify"] = sub.add_parser('quantify', help="Quantify transcriptome expression or metagenome abundance")
    e.add_argument('-e', help='Select from (trans, meta)', default=None, required=True)
    e.add_argument('-i', '--read', help='Input reads for quantification', required=True)
    e.add_argument('-rt', '--ref_t', help='Reference Transcriptome', default='')
    e.add_argument('-gl', '--genome_list', help=HELP_GENOME_LIST, default='')
    e.add_argument('-ga', '--g_alnm', help=HELP_GA_META, default='')
    e.add_argument('-ta', '--t_alnm', help='Transcriptome alignment file in sam format(optional)', default='')
    e.add_argument('-o', '--output', help='The location and prefix of outputting profile (Default = expression)', default='expression')
    e.add_argument('-t', '--num_threads', help='Number of threads for alignment (Default = 1)', default='1')
    e.add_argument('-n', '--normalize', help='Normalize by transcript length', **flag)

    r = modes["detect_ir"] = sub.add_parser('detect_ir', help="Detect Intron Retention events using the alignment file")
    r.add_argument('-annot', '--annotation', help='Annotation file in ensemble GTF/GFF formats', required=True)
    r.add_argument('-i', '--read', help='Input read for training, not required if alignment files are provided', default='')
    r.add_argument('-rg', '--ref_g', help='Reference genome, not required if genome alignment file is provided', default='')
    r.add_argument('-rt', '--ref_t', help='Reference Transcriptome, not required if transcriptome alignment file is provided', default='')
    r.add_argument('-a', '--aligner', help='The aligner to be used: minimap2 or LAST (Default = minimap2)', choices=['minimap2', 'LAST'], default='minimap2')
    r.add_argument('-o', '--output', help='The output name and location', required=False, default='ir_info')
    r.add_argument('-ga', '--g_alnm', help='Genome alignment file in SAM/BAM format (optional)', default='')
    r.add_argument('-ta', '--t_alnm', help='Transcriptome alignment file in SAM/BAM format (optional)', default='')
    r.add_argument('-t', '--num_threads', help='Number of threads for alignment (Default = 1)', default='1')
    return parser, modes


def ext(path: str) -> str:
    return os.path.splitext(path)[1][1:]


def stop(message: str, usage=None) -> None:
    """a failed validity check: the message, the usage of the sub-parser the reference prints there, status 1"""
    print(message)
    if usage is not None:
        usage.print_help(sys.stderr)
    sys.exit(1)


def check_format(path: str, formats, message: str, usage) -> None:
    if path != '' and ext(path) not in formats:
        stop(message, usage)


def check_reads_are_fastq(infile: str, echo: bool = False) -> None:
    """--fastq: the reads file has to be named .fastq / .fq (.gz) (R:555-561; transcriptome mode prints the extension first, R:763)"""
    pre, e = os.path.splitext(infile)
    if echo:
        print(e)
    if e == ".gz":
        e = os.path.splitext(pre)[1]
    if e not in READ_FORMATS:
        stop(MSG_FASTA)


def show(title: str, rows) -> None:
    """the parameter block: the title between blank lines, then `name value` per row"""
    print("\n" + title + "\n")
    for name, value in rows:
        print(name, value)


def make_prefix_dir(prefix: str) -> None:
    d = os.path.dirname(prefix)
    if d != '':
        os.makedirs(d, exist_ok=True)


def aligner_command(kind: str, aligner: str, threads: str, ref: str, reads: str, prefix: str):
    """the shell commands with which the reference would have made the missing alignment file (R:84, 92-93, 136, 144-145, 170, 177-178).
    kind: "genome" (align_genome), "transcriptome" / "splice" (align_transcriptome's two alignments)"""
    stem = prefix + ("_transcriptome_alnm" if kind == "transcriptome" else "_genome_alnm")
    if aligner == "minimap2":
        preset = "splice" if kind == "splice" else "map-ont"
        return ["minimap2 --cs -ax " + preset + " -t " + threads + " " + ref + " " + reads + " | samtools view -b > " + stem + ".bam"]
    db = "ref_transcriptome" if kind == "transcriptome" else "ref_genome"
    return ["lastdb " + db + " " + ref, "lastal -a 1 -P " + threads + " " + db + " " + reads + " > " + stem + ".maf"]


def no_aligner(what: str, commands) -> None:
    """the place where the reference starts an aligner"""
    print("This build does not align reads: give the %s alignment file (SAM, BAM or MAF).  The reference would have run:" % what)
    for c in commands:
        print("    " + c)
    sys.exit(1)


def need_files(*paths) -> None:
    for p in paths:
        if p and not os.path.isfile(p):
            print("No such file: " + p)
            sys.exit(1)


def engine():
    from . import engine as EN
    return EN.Engine(0)


def run_quantify(a, modes) -> None:
    show("running the code with following parameters", [("mode", a.e), ("infile", a.read), ("ref_t", a.ref_t), ("genome_list", a.genome_list),
                                                        ("g_alnm", a.g_alnm), ("t_aln,", a.t_alnm), ("prefix", a.output),
                                                        ("num_threads", a.num_threads), ("normalize by transcript length", a.normalize)])
    make_prefix_dir(a.output)
    from . import characterize
    if a.e == "trans":
        check_format(a.t_alnm, ('sam', 'bam'), MSG_FORMAT_SB, modes["genome"])
        if a.t_alnm == '':
            log("Alignment with minimap2 to reference transcriptome")
            no_aligner("transcriptome", aligner_command("transcriptome", "minimap2", a.num_threads, a.ref_t, a.read, a.output))
        need_files(a.t_alnm)
        log("Processing transcriptome alignment file: " + ext(a.t_alnm))
        eng = engine()
        characterize.quantify_reads(a.output, a.t_alnm, eng, "trans", normalize=a.normalize)
        eng.close()
    elif a.e == "meta":
        check_format(a.g_alnm, ('sam', 'bam'), MSG_FORMAT_SB, modes["genome"])
        log("Processing reference genome")
        need_files(a.genome_list)
        expected = characterize.expected_abundance(a.genome_list)
        if a.g_alnm == '':
            log("Alignment with minimap2")
            no_aligner("genome", aligner_command("genome", "minimap2", a.num_threads, "reference_metagenome.fasta", a.read, a.output))
        need_files(a.g_alnm)
        log("Processing alignment file: " + ext(a.g_alnm))
        eng = engine()
        characterize.quantify_reads(a.output, a.g_alnm, eng, "meta", expected=expected, normalize=a.normalize)
        eng.close()
    log("Finished!")


def run_detect_ir(a, modes) -> None:
    usage = modes["detect_ir"]
    if a.g_alnm == '' and a.ref_g == '':
        stop(MSG_NEED_G, usage)
    if a.t_alnm == '' and a.ref_t == '':
        stop(MSG_NEED_T, usage)
    check_format(a.g_alnm, ('maf', 'sam', 'bam'), MSG_FORMAT_MSB_IR, usage)
    check_format(a.t_alnm, ('maf', 'sam', 'bam'), MSG_FORMAT_MSB, usage)
    show("running the code with following parameters:", [("annot", a.annotation), ("infile", a.read), ("aligner", a.aligner), ("ref_g", a.ref_g),
                                                         ("ref_t", a.ref_t), ("g_alnm", a.g_alnm), ("t_alnm", a.t_alnm), ("prefix", a.output)])
    make_prefix_dir(a.output)
    if a.t_alnm == '':
        log("Alignment with " + a.aligner + " to reference transcriptome")
        no_aligner("transcriptome", aligner_command("transcriptome", a.aligner, a.num_threads, a.ref_t, a.read, a.output))
    if a.g_alnm == '':
        log("Alignment with " + a.aligner + " to reference genome")
        no_aligner("genome", aligner_command("splice", a.aligner, a.num_threads, a.ref_g, a.read, a.output))
    if "maf" in (ext(a.t_alnm), ext(a.g_alnm)):
        stop(MSG_IR_MAF, usage)
    need_files(a.annotation, a.t_alnm, a.g_alnm)
    from . import characterize
    log("Processing transcriptome alignment file: " + ext(a.t_alnm))
    log("Processing genome alignment file: " + ext(a.g_alnm))
    log("Parse the annotation file (GTF/GFF3)")
    log("Modeling Intron Retention")
    eng = engine()
    characterize.detect_ir(a.output, a.annotation, a.g_alnm, a.t_alnm, eng)
    eng.close()
    log("Finished!")


def run_genome(a, modes, meta: bool) -> None:
    usage = modes["genome"]                                 # (metagenome mode prints genome mode's usage too, R:633)
    check_format(a.g_alnm, ('sam', 'bam') if meta else ('maf', 'sam', 'bam'), MSG_FORMAT_SB if meta else MSG_FORMAT_MSB, usage)
    if not meta and a.g_alnm == '' and a.ref_g == '':
        stop(MSG_NEED_G, usage)
    if a.homopolymer and int(a.min_homopolymer_len) < 0:
        stop(MSG_HP_LEN, usage)
    if a.fastq:
        check_reads_are_fastq(a.read)
    rows = [("infile", a.read)] + ([("genome_list", a.genome_list)] if meta else [("ref_g", a.ref_g), ("aligner", a.aligner)]) + \
        [("g_alnm", a.g_alnm), ("prefix", a.output), ("num_threads", a.num_threads), ("model_fit", a.no_model_fit), ("chimeric", a.chimeric)]
    if meta:
        rows += [("fastq", a.fastq), ("quantification", a.quantification)]
    else:
        rows += [("homopolymer", a.homopolymer)] + ([("min_homopolymer_len", a.min_homopolymer_len)] if a.homopolymer else []) + [("fastq", a.fastq)]
    show("Running the code with following parameters:", rows)
    make_prefix_dir(a.output)
    log("Read pre-process")
    from . import characterize
    expected = None
    if meta:
        log("Processing reference genome")
        need_files(a.genome_list)
        expected = characterize.expected_abundance(a.genome_list)
    if a.g_alnm == '':
        aligner = "minimap2" if meta else a.aligner
        log("Alignment with " + aligner)
        no_aligner("genome", aligner_command("genome", aligner, a.num_threads, "reference_metagenome.fasta" if meta else a.ref_g, a.read, a.output))
    if ext(a.g_alnm) == "maf" and (a.fastq or os.path.splitext(a.read[:-3] if a.read.endswith(".gz") else a.read)[1] in READ_FORMATS):
        sys.stderr.write(MSG_MAF_QUAL)
        sys.exit(1)
    need_files(a.g_alnm, a.read if ext(a.g_alnm) == "maf" else '')
    eng = engine()
    common = dict(chimeric_reads=a.chimeric, homopolymer=a.homopolymer, min_hp_len=int(a.min_homopolymer_len), fastq=a.fastq, model_fit=a.no_model_fit,
                  log=log)
    if meta:
        characterize.train_metagenome(a.output, a.g_alnm, a.read, eng, quantification=a.quantification, expected=expected, **common)
    else:
        characterize.train_genome(a.output, a.g_alnm, a.read, eng, **common)
    eng.close()
    log("Finished!")


def run_transcriptome(a, modes) -> None:
    ir = a.no_intron_retention
    if ir and a.g_alnm == '' and a.ref_g == '':
        stop(MSG_NEED_G_IR, modes["detect_ir"])
    if a.t_alnm == '' and a.ref_t == '':
        stop(MSG_NEED_T, modes["detect_ir"])
    usage = modes["transcriptome"]
    if a.g_alnm != '' and a.t_alnm != '':
        if ext(a.g_alnm) != ext(a.t_alnm) or ext(a.g_alnm) not in ('maf', 'sam', 'bam'):
            stop(MSG_SAME_FORMAT, usage)
        if ext(a.g_alnm) == "maf" and ir:
            stop(MSG_IR_MAF, usage)
    if ir and (a.ref_g == '' or a.annotation == ''):
        stop(MSG_IR_NEEDS, usage)
    if a.homopolymer and int(a.min_homopolymer_len) < 0:
        stop(MSG_HP_LEN, modes["genome"])
    if a.fastq:
        check_reads_are_fastq(a.read, echo=True)
    show("running the code with following parameters:",
         [("infile", a.read), ("ref_g", a.ref_g), ("ref_t", a.ref_t), ("annot", a.annotation), ("aligner", a.aligner), ("g_alnm", a.g_alnm),
          ("t_alnm", a.t_alnm), ("prefix", a.output), ("num_threads", a.num_threads), ("model_fit", a.no_model_fit), ("intron_retention", ir),
          ("homopolymer", a.homopolymer)] + ([("min_homopolymer_len", a.min_homopolymer_len)] if a.homopolymer else []) +
         [("fastq", a.fastq), ("quantification", a.quantification), ("normalize by transcript length", a.normalize)])
    make_prefix_dir(a.output)
    log("Read pre-process and unaligned reads analysis")
    if a.t_alnm == '':
        log("Alignment with " + a.aligner + " to reference transcriptome")
        no_aligner("transcriptome", aligner_command("transcriptome", a.aligner, a.num_threads, a.ref_t, a.read, a.output))
    if a.g_alnm == '':
        log("Alignment with " + a.aligner + " to reference genome")
        no_aligner("genome", aligner_command("splice", a.aligner, a.num_threads, a.ref_g, a.read, a.output))
    if ext(a.t_alnm) == "maf":
        print("transcriptome mode of this build takes SAM or BAM alignments")
        sys.exit(1)
    need_files(a.t_alnm, a.g_alnm, a.annotation if ir else '')
    from . import characterize
    eng = engine()
    characterize.train_transcriptome(a.output, a.t_alnm, a.g_alnm, a.read, eng, annotation=a.annotation, ir=ir, chimeric_reads=a.chimeric,
                                     quantification=a.quantification, normalize=a.normalize, homopolymer=a.homopolymer,
                                     min_hp_len=int(a.min_homopolymer_len), fastq=a.fastq, model_fit=a.no_model_fit, log=log)
    eng.close()
    log("Finished!")


def main(argv=None) -> None:
    parser, modes = build_parser()
    argv = sys.argv[1:] if argv is None else list(argv)
    a = parser.parse_args(argv)
    if not argv or a.mode is None:
        parser.print_help(sys.stderr)
        sys.exit(1)
    if a.mode == "quantify":
        run_quantify(a, modes)
    elif a.mode == "detect_ir":
        run_detect_ir(a, modes)
    elif a.mode == "transcriptome":
        run_transcriptome(a, modes)
    else:
        run_genome(a, modes, meta=a.mode == "metagenome")


if __name__ == "__main__":
    main()
