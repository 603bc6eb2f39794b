"""nanosim_amd.characterize as a package: every name the single module had is still a name of the package, the mirrors of the
library's structures keep their size and fields, and every submodule imports on its own."""
import ctypes
import os
import pkgutil
import subprocess
import sys

import numpy as np
import pytest

from nanosim_amd import characterize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every non-dunder, non-module name of vars(characterize) when it was one module; a ctypes structure or a dtype with its size and fields
NAMES = (
    ('CHIM_ALONE',), ('CHIM_ENT_DTYPE', 16, ('qstart', 'qend', 'qlen', 'rlen')), ('CHIM_HAS_SA',), ('CHIM_NO_GAP',),
    ('CHIM_PIECE_DTYPE', 16, ('entry', 'is_primary', 'gap')), ('CHIM_POS_STRAND',), ('CHIM_READ_DTYPE', 8, ('n_pieces', 'flags')), ('ChimRecord',),
    ('DICT_MAX',), ('EM_KINDS',), ('ERR_COLS',), ('ERR_ROWS',), ('HP_CLASSES',), ('HP_COLUMNS',), ('HP_NOT_CONVERGED',), ('HP_PW_KEYS',),
    ('HP_RECORD_DTYPE', 16, ('aln', 'start', 'ref_len', 'read_base')), ('IR_NONE',), ('IR_READ_IR',), ('IR_READ_NONE',), ('IR_READ_NO_IR',),
    ('IrRead',), ('KDE_NAMES',), ('LEN_ALN_DTYPE', 24, ('head', 'tail', 'read_len', 'ref_len', 'query_aln_len', 'edge')), ('LEN_GENOME',),
    ('LEN_MODES',), ('LEN_NONE',), ('LEN_READ_DTYPE', 16, ('read_len', 'head', 'tail', 'n_segments')), ('LEN_TRANSCRIPTOME',),
    ('MAF_FIGURES_DTYPE', 24, ('aligned_ref', 'ref_total', 'head', 'total', 'ht')),
    ('MAF_LINES_DTYPE', 32, ('ref_begin', 'ref_end', 'qry_begin', 'qry_end')),
    ('MAF_RECORD_DTYPE', 40, ('ref_name_at', 'ref_seq_at', 'qry_seq_at', 'ref_name_len', 'ref_seq_len', 'qry_seq_len', 'ref_start')),
    ('MIXFIT_DTYPE', 64, ('x', 'fun', 'residual', 'nfev', 'nit', 'status', 'reserved')), ('MIXFIT_EVALUATE',), ('MIXFIT_FIT',), ('MIXFIT_INDEL',),
    ('MIXFIT_MISMATCH',), ('MIXFIT_TYPES',),
    ('NsChimResult', 80, ('ent', 'pieces', 'reads', 'species_count', 'n_gaps', 'pos_strand', 'n_bad', 'first_bad', 'ms_kernel', 'ms_scan')),
    ('NsCsHist', 40256, ('cap_match2d', '_pad', 'match_list', 'dic', 'error_list', 'first_error', 'max_match', 'n_match2d_overflow', 'n_skip', 'ms_kernel')),
    ('NsEmProblem', 64, ('n_targets', 'n_multi', 'multi_off', 'target', 'weight', 'unique', 'total', 'factor', 'max_iter', 'group')),
    ('NsEmResult', 48, ('abundance', 'count', 'diff_trace', 'n_iter', 'reserved', 'n_nonfinite', 'ms_kernel')),
    ('NsHpHist', 104, ('cap_ref', 'cap_read', 'table', 'records', 'cap_records', 'n_hp', 'columns', 'max_ref', 'max_read', 'n_overflow', 'ms_kernel')),
    ('NsIrIntrons', 72, ('n_trx', 'n_chrom', 'intr_off', 'intr_chrom', 'intr_start', 'intr_end', 'merged_off', 'merged_chrom', 'merged_start', 'merged_end')),
    ('NsIrTrainResult', 88, ('state', 'retained', 'first', 'states', 'n_bad', 'first_bad', 'ms_kernel')),
    ('NsLenResult', 56, ('aln', 'reads', 'segments', 'n_segments', 'n_bad', 'first_bad', 'ms_kernel')),
    ('NsMafBestResult', 88, ('found', 'lines', 'records', 'figures', 'n_lines', 'n_pairs', 'n_kept', 'pos_strand', 'first_bad_line', 'first_bad_offset', 'ms_kernel')),
    ('NsMixfitFit', 64, ('x', 'fun', 'residual', 'nfev', 'nit', 'status', 'reserved')), ('NsMixfitResult', 16, ('fits', 'ms_kernel')),
    ('NsQualAln', 16, ('head', 'tail', 'unmapped', 'reserved')), ('NsQualHist', 5144, ('hist', 'n_short', 'n_bad_qual', 'ms_kernel')),
    ('NsSamPairs', 72, ('ref_lines', 'query_lines', 'cap_bytes', 'aln_off', 'aln', 'n_bytes', 'n_bad', 'first_bad', 'ms_kernel')), ('PackedPairs',),
    ('QUAL_ALN_DTYPE', 16, ('head', 'tail', 'unmapped', 'reserved')), ('QUAL_TYPES',), ('QUAL_VALUES',),
    ('SAM_ALN_DTYPE', 16, ('head', 'tail', 'ref_len', 'query_len')), ('_CIGAR_TOKEN',), ('_CLIP_HEAD',), ('_CLIP_TAIL',), ('_MD_TOKEN',),
    ('_alone_winner',), ('_count',), ('_dict_len',), ('_file_bytes',), ('_hp_count',), ('_last_s_line',), ('_len_call',), ('_line_number',),
    ('_mapped_records',), ('_pack',), ('_pack_pairs',), ('_pack_sam',), ('_parser_interval',), ('_piecewise_rss',), ('_pysam_interval',),
    ('_qual_call',), ('_sam_out',), ('_sam_packed',), ('_sam_refs',), ('_strip_chr',), ('abundance_variation',), ('add_introns',), ('annotations',),
    ('base_qualities',), ('besthit',), ('besthit_and_unaligned',), ('besthit_call',), ('chimeric',), ('chimeric_beta',), ('chimeric_call',),
    ('chimeric_records',), ('cigar_spans',), ('count',), ('count_homopolymers',), ('count_homopolymers_sam',), ('count_intron_retention',),
    ('count_maf',), ('count_qualities',), ('count_read_lengths',), ('cs_from_sam',), ('em_call',), ('em_problem',), ('em_quantify',),
    ('empirical_cdf',), ('fasta_lines',), ('figures_from_rows',), ('fit_homopolymers',), ('fit_mixtures',), ('fit_piecewise',), ('fit_qualities',),
    ('fit_starts',), ('format_alignment_rate',), ('format_base_qualities',), ('format_chimeric_info',), ('format_hp_lengths',), ('format_hp_model',),
    ('format_ir_info',), ('format_ir_markov_model',), ('format_maf',), ('format_model_profile',), ('format_quantification',), ('format_strandness',),
    ('format_tables',), ('get_cs',), ('hist',), ('homopolymer_lengths',), ('homopolymer_lengths_from_sam',), ('intron_retention',),
    ('ir_alignments',), ('ir_introns',), ('ir_tables',), ('ir_train_call',), ('iteration_lines',), ('kde_models',), ('length_figures_maf',),
    ('length_records',), ('maf_pairs',), ('maf_records',), ('mixture_fit',), ('model_fitting',), ('pairs_from_sam',), ('primary_and_unaligned',),
    ('quals_from_sam',), ('quant_items',), ('quant_items_primary',), ('quant_targets',), ('quantify',), ('read_length_hist',), ('read_lengths',),
    ('read_lengths_from_maf',), ('sa_entries',), ('sam_records',), ('select_chimeric',), ('select_fit',), ('species_of_reference',),
    ('train_genome_from_maf',), ('write_besthit',), ('write_kde',), ('write_maf',),
)
SUBMODULES = sorted(m.name for m in pkgutil.iter_modules(characterize.__path__))


def test_every_name_of_the_single_module_is_a_name_of_the_package():
    assert len(NAMES) == 160 and len(set(n[0] for n in NAMES)) == 160
    missing = [n[0] for n in NAMES if not hasattr(characterize, n[0])]
    assert not missing, missing
    for name in ("hist", "chimeric", "quantify", "read_lengths", "intron_retention", "besthit"):       # functions, whatever the modules are called
        assert callable(getattr(characterize, name)), name


def test_structures_and_dtypes_keep_size_and_fields():
    sized = [n for n in NAMES if len(n) == 3]
    assert len(sized) == 26
    for name, size, fields in sized:
        obj = getattr(characterize, name)
        if isinstance(obj, np.dtype):
            assert (obj.itemsize, tuple(obj.names)) == (size, fields), name
        else:
            assert issubclass(obj, ctypes.Structure), name
            assert (ctypes.sizeof(obj), tuple(f[0] for f in obj._fields_)) == (size, fields), name


def test_no_submodule_shares_its_name_with_a_function_of_the_package():
    """`characterize.<name>` cannot be both: a submodule named like a function would be shadowed by it"""
    assert len(SUBMODULES) >= 12
    assert not [m for m in SUBMODULES if m in set(n[0] for n in NAMES)]


@pytest.mark.parametrize("module", SUBMODULES)
def test_submodule_imports_on_its_own(module):
    """a fresh interpreter each: an import cycle or a dependence on the order in which __init__ imports fails here"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", "import nanosim_amd.characterize." + module], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
