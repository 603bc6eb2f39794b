"""What the modes of ``read_analysis.py`` run behind the aligner (src/read_analysis.py, R:76-205, 416-457, 511-521, 605-611, 815-890) are
the fourteenth piece: one function per mode over the stage functions of the other modules, in the reference's sequence.  Every
alignment file is indexed once (``SamTable``; a ``.bam`` through ``read_bam``) and every stage reads the table or a view of it:

    characterize.train_genome("training", "aln.bam", "reads.fq", eng, chimeric_reads=True, homopolymer=True, fastq=True)
    characterize.train_metagenome("training", "aln.sam", "reads.fa", eng, quantification=True, expected={"spA": 60.0, "spB": 40.0})
    characterize.train_transcriptome("training", "t.sam", "g.sam", "reads.fa", eng, annotation="annot.gff3")
    characterize.quantify_reads("expression", "t.sam", eng, "trans")
    characterize.detect_ir("ir_info", "annot.gff3", "g.sam", "t.sam", eng)

``python -m nanosim_amd.read_analysis`` parses the reference's command line for them.  Deviations: nothing is aligned, so
the pre-processed copy of the reads and the concatenated metagenome, which exist to be aligned, are not written; transcriptome mode
takes SAM / BAM (its MAF branch is genome mode's, ``train_genome_from_maf``); the annotation is GFF3 (``add_introns``)."""
import os

from .bam import read_bam
from .chimeric_reads import chimeric
from .errors import cs_from_sam, hist
from .ir_model import add_introns, intron_retention
from .lengths import primary_and_unaligned, read_lengths
from .maf_besthit import train_genome_from_maf
from .mixfit import model_fitting
from .qualities import base_qualities, quals_from_sam
from .quantification import quantify
from .sam_pairs import homopolymer_lengths_from_sam, sam_records
from .sam_table import SamTable


def alignment_format(path: str) -> str:
    """the extension of an alignment file without its dot, as the reference takes it (R:181-182)"""
    return os.path.splitext(path)[1][1:]


def alignment_table(path: str, eng) -> SamTable:
    """the SamTable of a `.sam` or `.bam` alignment file"""
    return SamTable(read_bam(path, eng) if alignment_format(path) == "bam" else path, eng)


def expected_abundance(genome_list: str):
    """{species: percent} from column 3 of a metagenome list (R:687-694: the species name with its blanks dashed); None when no line has one"""
    expected = {}
    with open(genome_list) as f:
        for line in f:
            info = line.strip().split("\t")
            if len(info) == 3:
                expected["-".join(info[0].split())] = float(info[2])
    return expected or None


def primary_stage(prefix: str, table: SamTable, eng, chimeric_reads: bool = False, quantification=None, expected=None, normalize: bool = True, pickles=None):
    """get_primary_sam's part of a mode (R:192-198, 109-117) over one table: with chimeric_reads chimeric() — which quantifies when
    `quantification` ("meta" / "trans") says so — else primary_and_unaligned and, for "meta", quantify().  <prefix>_primary.sam is
    written either way.  -> (refs, records, unaligned_len, strandness, the view of the primary records)"""
    if chimeric_reads:
        selected = []
        refs, records, unaligned_len, strandness = chimeric(prefix, table, eng, pickles=pickles, quantify=quantification, normalize=normalize, selected=selected)
        primary = table.take(table.mapped_rows()[selected])
    else:
        refs, records, unaligned_len, strandness = primary_and_unaligned(table)
        if quantification == "meta":
            quantify(prefix, table, eng, "meta", expected=expected, normalize=normalize)
        primary = table.primary()
        primary.write_sam(prefix + "_primary.sam")
    return refs, records, unaligned_len, strandness, primary


def _say(log, stage: str) -> None:
    """a stage line of the reference (its wording behind the timestamp) to the caller's `log`, when it gave one"""
    if log is not None:
        log(stage)


def _models(prefix: str, errors_from: SamTable, primary: SamTable, table: SamTable, eng, model_fit, homopolymer, min_hp_len, fastq, hist_prefix=None, log=None):
    """R:854-890: the error model, its fit, the homopolymer-length and the base-quality model"""
    _say(log, "match and error models")
    hist(hist_prefix or prefix, cs_from_sam(errors_from), eng)
    if model_fit:
        _say(log, "Model fitting")
        model_fitting(prefix, eng)
    if homopolymer:
        _say(log, "Analyzing homopolymer lengths and estimating model parameters")
        homopolymer_lengths_from_sam(prefix, sam_records(primary), eng, min_hp_len, maf_file=True)
    if fastq:
        _say(log, "Analyzing base qualities and estimating model parameters")
        base_qualities(prefix, quals_from_sam(primary)[0], table.unmapped_quals(), eng)


def train_genome(prefix: str, alignment: str, reads: str, eng, chimeric_reads: bool = False, homopolymer: bool = False, min_hp_len: int = 5, fastq: bool = False,
                 model_fit: bool = True, pickles=None, quantification=None, expected=None, log=None) -> SamTable:
    """what `read_analysis.py genome -ga alignment` leaves (R:192-205, 605-611, 833-890): the primary records (chimeric(), merged into
    the length models, with chimeric_reads) and <prefix>_primary.sam, the read-length files, the error model from the primary records'
    cs strings, its fit unless model_fit is False, with `homopolymer` the homopolymer-length model and <prefix>_processed.maf, with
    `fastq` the base-quality model from the primary records and the QUAL of the unmapped ones.  A `.maf` alignment goes through
    train_genome_from_maf with `reads` (FASTA); `reads` is not read otherwise.  The prefix opens with model.load_model(prefix), with
    chimeric_reads with load_model(prefix, chimeric=True).  log: a function that takes the reference's stage lines ("Aligned reads
    analysis", ...) as the work comes to them.  -> the table (a `.maf`: besthit's dict)"""
    if alignment_format(alignment) == "maf":
        if fastq:
            raise ValueError("the base-quality model cannot be estimated from alignments in MAF format")
        _say(log, "Processing alignment file: maf")
        return train_genome_from_maf(prefix, alignment, reads, eng, model_fit=model_fit, homopolymer=homopolymer, min_hp_len=min_hp_len, pickles=pickles)
    _say(log, "Processing alignment file: " + alignment_format(alignment))
    table = alignment_table(alignment, eng)
    refs, records, unaligned_len, strandness, primary = primary_stage(prefix, table, eng, chimeric_reads, quantification, expected, pickles=pickles)
    _say(log, "Aligned reads analysis")
    _say(log, "Unaligned reads analysis")
    read_lengths(prefix, refs, records, eng, unaligned_len, strandness, pickles=pickles, merge=chimeric_reads)
    _models(prefix, primary, primary, table, eng, model_fit, homopolymer, min_hp_len, fastq, log=log)
    return table


def train_metagenome(prefix: str, alignment: str, reads: str, eng, chimeric_reads: bool = False, quantification: bool = False, expected=None,
                     homopolymer: bool = False, min_hp_len: int = 5, fastq: bool = False, model_fit: bool = True, pickles=None, log=None) -> SamTable:
    """what `read_analysis.py metagenome -ga alignment` leaves (R:685-705): train_genome over SAM / BAM with, under `quantification`,
    the abundances of the species (the part of every reference name in front of its last `_`) in <prefix>_quantification.tsv — from
    chimeric() with chimeric_reads, which puts them behind the shrinkage rate, else from quantify(), which takes `expected`
    ({species: percent}, expected_abundance of the metagenome list)"""
    if alignment_format(alignment) == "maf":
        raise ValueError("metagenome mode takes SAM or BAM alignments")
    return train_genome(prefix, alignment, reads, eng, chimeric_reads, homopolymer, min_hp_len, fastq, model_fit, pickles,
                        quantification="meta" if quantification else None, expected=expected, log=log)


def train_transcriptome(prefix: str, t_alignment: str, g_alignment: str, reads: str, eng, annotation=None, ir: bool = True, chimeric_reads: bool = False,
                        quantification: bool = False, normalize: bool = False, homopolymer: bool = False, min_hp_len: int = 5, fastq: bool = False,
                        model_fit: bool = True, pickles=None, log=None):
    """what `read_analysis.py transcriptome -ta t_alignment -ga g_alignment` leaves (R:76-159, 815-890): the primary records of the
    transcriptome alignment under <prefix>_transcriptome (through chimeric() with chimeric_reads, which quantifies the transcripts
    under `quantification`, by length with `normalize`), those of the genome alignment in <prefix>_genome_primary.sam; with `ir`
    <prefix>_added_intron_final.gff3 from `annotation` and the intron-retention model; the read-length files in transcriptome mode
    with the genome records' heads and tails; the error model from the GENOME primaries, the homopolymer-length and base-quality
    models from the TRANSCRIPTOME primaries.  SAM / BAM.  -> (the transcriptome table, the genome table)"""
    for path in (t_alignment, g_alignment):
        if alignment_format(path) == "maf":
            raise ValueError("transcriptome mode takes SAM or BAM alignments (a MAF alignment trains in genome mode: train_genome_from_maf)")
    _say(log, "Processing transcriptome alignment file: " + alignment_format(t_alignment))
    t_table = alignment_table(t_alignment, eng)
    refs, records, unaligned_len, strandness, t_primary = primary_stage(prefix + "_transcriptome", t_table, eng, chimeric_reads,
                                                                        "trans" if quantification and chimeric_reads else None, normalize=normalize, pickles=pickles)
    _say(log, "Processing genome alignment file: " + alignment_format(g_alignment))
    g_table = alignment_table(g_alignment, eng)
    _, g_records, _, _ = primary_and_unaligned(g_table)
    g_primary = g_table.primary()
    g_primary.write_sam(prefix + "_genome_primary.sam")
    if ir:
        if not annotation:
            raise ValueError("the intron-retention model needs an annotation file")
        _say(log, "Parse the annotation file (GTF/GFF3)")
        add_introns(annotation, prefix + "_added_intron_final.gff3")
        _say(log, "Modeling Intron Retention")
        intron_retention(prefix, prefix + "_added_intron_final.gff3", g_table, t_table, eng)
    _say(log, "Aligned reads analysis")
    _say(log, "Unaligned reads analysis")
    read_lengths(prefix, refs, records, eng, unaligned_len, strandness, mode="transcriptome", genome_records=g_records, pickles=pickles, merge=chimeric_reads)
    _models(prefix, g_primary, t_primary, t_table, eng, model_fit, homopolymer, min_hp_len, fastq, hist_prefix=prefix + "_genome", log=log)
    return t_table, g_table


def quantify_reads(prefix: str, alignment: str, eng, kind: str, expected=None, normalize: bool = False):
    """`read_analysis.py quantify -e trans|meta` (R:416-457): <prefix>_quantification.tsv from a SAM / BAM alignment and nothing else;
    -> quantify's pair"""
    return quantify(prefix, alignment_table(alignment, eng), eng, kind, expected=expected if kind == "meta" else None, normalize=normalize)


def detect_ir(prefix: str, annotation: str, g_alignment: str, t_alignment: str, eng) -> dict:
    """`read_analysis.py detect_ir` (R:511-521): <prefix>_added_intron_final.gff3 from the annotation, then <prefix>_IR_markov_model
    and <prefix>_IR_info from the two alignments; -> intron_retention's counts"""
    add_introns(annotation, prefix + "_added_intron_final.gff3")
    return intron_retention(prefix, prefix + "_added_intron_final.gff3", alignment_table(g_alignment, eng), alignment_table(t_alignment, eng), eng)
