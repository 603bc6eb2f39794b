"""Training side: what the reference's ``read_analysis.py`` leaves behind for ``simulator.py``, from alignments.  The
walks run on the GPU through the C-ABI (include/nanosim_amd.h); the modules read the input and format the reference's files from the
counts, text for text.  One stage per module, whose docstring names the part of the reference it stands in for, with the line
references, and every deviation from it.  Every name of a module is a name of the package; with eng = engine.Engine(0):

    errors          characterize.hist("training", characterize.cs_from_sam("training_primary.sam"), eng)
    qualities       characterize.base_qualities("training", *characterize.quals_from_sam("training.sam"), eng)
    homopolymers    characterize.homopolymer_lengths("training", characterize.maf_records("training_besthit.maf"), eng, min_hp_len=5)
    sam_pairs       characterize.homopolymer_lengths_from_sam("training", characterize.sam_records("training_primary.sam"), eng)
    mixfit          characterize.model_fitting("training", eng)
    lengths         characterize.read_lengths("training", refs, recs, eng, unaligned_len, strandness)   # of primary_and_unaligned("training.sam")
    chimeric_reads  refs, recs, unaligned_len, strandness = characterize.chimeric("training", "training.sam", eng)
    quantification  abundance, variation = characterize.quantify("training", "training.sam", eng, "meta", expected={"spA": 60.0, "spB": 40.0})
    ir_model        characterize.intron_retention("training", "training_added_intron_final.gff3", "genome.sam", "transcriptome.sam", eng)
    maf_besthit     characterize.train_genome_from_maf("training", "last.maf", "reads.fasta", eng)
    bam             characterize.cs_from_sam(characterize.read_bam("training_primary.bam", eng))    # a BAM file wherever a reader takes a SAM path
    calmd           characterize.cs_from_sam(characterize.with_reference("calls.sam", "genome.fa", eng))   # MD:Z and cs:Z from the reference genome

    sam_table       table = characterize.SamTable("training.sam", eng)    # the SAM text indexed on the GPU: every reader takes it for the path
    training        characterize.train_genome("training", "aln.bam", "reads.fq", eng, chimeric_reads=True, homopolymer=True, fastq=True)
                    characterize.train_metagenome("training", "aln.sam", "reads.fa", eng, quantification=True, expected={"spA": 60.0, "spB": 40.0})
                    characterize.train_transcriptome("training", "t.sam", "g.sam", "reads.fa", eng, annotation="annot.gff3")
                    characterize.quantify_reads("expression", "t.sam", eng, "trans")
                    characterize.detect_ir("ir_info", "annot.gff3", "g.sam", "t.sam", eng)

The five functions of `training` are the modes of ``python -m nanosim_amd.read_analysis``, which only parses their arguments.
Below them: chim_select (what chimeric_reads and quantification share), sam_text (the one loop over SAM text), _abi (marshalling)."""
from __future__ import annotations

from . import (_abi, sam_text, sam_table, errors, qualities, homopolymers, sam_pairs, mixfit, lengths, chim_select, quantification,
               chimeric_reads, ir_model, maf_besthit, bam, calmd, training)

for _module in (_abi, sam_text, sam_table, errors, qualities, homopolymers, sam_pairs, mixfit, lengths, chim_select, quantification,
                chimeric_reads, ir_model, maf_besthit, bam, calmd, training):             # the underscore names too: tests and scripts use _pack, _qual_call, _strip_chr, ...
    globals().update((k, v) for k, v in vars(_module).items() if not k.startswith("__"))
