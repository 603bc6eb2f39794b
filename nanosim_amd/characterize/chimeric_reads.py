"""Chimeric training (``primary_and_unaligned_chimeric`` of src/get_primary_sam.py, G:220-478) is the seventh piece: what ``--chimeric``
and metagenome mode need next to the files above — ``<prefix>_chimeric_info`` and the ``gap_length`` KDE — and the choice of the records
every later training step reads (``<prefix>_primary.bam`` there, ``<prefix>_primary.sam`` here).  For every primary alignment with an
``SA:Z`` tag the reference parses the CIGAR of every entry, sorts the entries into lists of compatible pieces, keeps the best list and
records the gaps between its pieces; here the CIGAR walks and the choice run on the GPU (``ns_cigar_spans``, ``ns_chimeric_select``;
csrc/ns_chimeric.h names every corner of the reference that is kept), and this module matches the chosen pieces to SAM records and
writes the files:

    refs, recs, unaligned_len, strandness = characterize.chimeric("training", "training.sam", eng)
    characterize.read_lengths("training", refs, recs, eng, unaligned_len, strandness, merge=True)

``read_lengths`` writes ``<prefix>_kde.npz`` anew and ``chimeric`` merges into it: ``read_lengths(..., merge=True)`` keeps ``gap_length``.
Deviations: SAM text instead of BAM; a primary record without ``NM``, an SA entry without six fields, a reference name without an
``@SQ`` line, a supplementary or secondary record in front of the first primary, a chosen piece that no record matches (the reference
hands ``None`` to pysam) and a file without a primary record raise ValueError where the reference stops with another exception; the
abundances behind the shrinkage rate come from the caller unless ``quantify="meta"`` is given."""
import statistics

import numpy as np

from ._abi import write_text
from .chim_select import chimeric_records, select_chimeric, species_of_reference
from .lengths import write_kde
from .quantification import em_quantify, format_quantification, quant_items, quant_targets


def chimeric_beta(species_count: dict, abundance: dict) -> float:
    """the shrinkage rate (G:449-455, 475): the median over the species with a recorded gap of other / (same + other) * 100 /
    (100 - abundance), abundance in percent (the reference's come from its EM, G:428: the caller's here)"""
    betas = []
    for sp, counts in species_count.items():
        other_prob = 100 - abundance[sp]
        if counts[0] + counts[1] == 0:
            continue
        betas.append(counts[1] / (counts[0] + counts[1]) * 100 / other_prob)
    if not betas:
        raise ValueError("no gap between pieces was recorded: there is no shrinkage rate")
    return statistics.median(betas)


def format_chimeric_info(n_gaps: int, num_aligned: int, beta=None) -> str:
    """the text of <prefix>_chimeric_info (G:472-475); the second line, written in metagenome mode, has no newline"""
    text = "Mean segments for each aligned read:\t" + str((n_gaps + num_aligned) / num_aligned) + "\n"
    if beta is not None:
        text += "Shrinkage rate (beta):\t" + str(beta)
    return text


def chimeric(prefix: str, path: str, eng, species=None, abundance=None, primary_sam: bool = True, pickles=None, quantify=None, normalize: bool = True,
             selected=None):
    """primary_and_unaligned_chimeric (G:220-478): writes <prefix>_chimeric_info, adds gap_length —
    log10(gap + 1), bandwidth 0.01 (G:465-469) — to <prefix>_kde.npz next to the keys it holds (and writes <prefix>_gap_length.pkl by
    write_kde's rule), and, with primary_sam, <prefix>_primary.sam: the header and the selected lines, unchanged, in the reference's
    order — what its later steps read from <prefix>_primary.bam, for cs_from_sam, quals_from_sam, sam_records and length_records.
    abundance ({species: percent}, with a species mapping): the second line of _chimeric_info (chimeric_beta).
    quantify: None — no quantification, as before; "meta" — the EM over the species (species: the mapping, by default
    species_of_reference of every @SQ name) writes <prefix>_quantification.tsv and its abundances stand behind the shrinkage rate
    (abundance= next to it is a ValueError); "trans" — the EM over the transcripts writes the file (normalize: EM_trans').
    selected: a list that takes the indices of the selected records among chimeric_records' records (SamTable.mapped_rows names
    their rows), in the order of <prefix>_primary.sam.
    -> (refs, records, unaligned_len, strandness): read_lengths' arguments, the records being the selected ones."""
    if quantify not in (None, "meta", "trans"):
        raise ValueError("quantify must be None, 'meta' or 'trans'")
    if quantify == "meta" and abundance is not None:
        raise ValueError("quantify='meta' computes the abundances: abundance= cannot be given as well")
    if abundance is not None and species is None:
        raise ValueError("abundance needs the species mapping")
    refs, records, unaligned_len, header = chimeric_records(path)
    if quantify == "meta" and species is None:
        species = {name: species_of_reference(name) for name, _ in refs}
    sel = select_chimeric(eng, refs, records, species)
    if selected is not None:
        selected.extend(int(i) for i in sel["selected"])
    if quantify is not None:
        items = quant_items(records, sel, refs, species if quantify == "meta" else None)
        res = em_quantify(eng, items, quant_targets(refs, quantify, species), quantify, normalize)
        write_text(prefix + "_quantification.tsv", format_quantification(quantify, res["result"]))
        if quantify == "meta":
            abundance = res["result"]
    beta = chimeric_beta(sel["species_count"], abundance) if abundance is not None else None
    write_text(prefix + "_chimeric_info", format_chimeric_info(len(sel["gap_length"]), sel["num_aligned"], beta))
    write_kde(prefix, {"gap_length": (np.log10(sel["gap_length"] + 1).astype(np.float64), 0.01)}, pickles, merge=True)
    if primary_sam:
        with open(prefix + "_primary.sam", "w") as f:
            f.writelines(header)
            f.writelines(records[i].line for i in sel["selected"])
    return refs, [tuple(records[i][:5]) for i in sel["selected"]], unaligned_len, sel["strandness"]
