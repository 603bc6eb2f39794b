#!/usr/bin/env python3
"""The census table of tests/test_gpu_kernel_classes.py, on the CPU oracle: every counter of
tests/kernel_classes.py summed over the existing cases that reach the record, dense and error-profile kernels without -k ("before":
test_gpu_parity.CASES, the model of test_dense_events_and_long_payloads on the linear and the circular reference, the circular-reference
cases, test_gpu_metagenome.CASES, one transcriptome batch) and over the cases of that file ("cases").  No GPU needed.
Usage: python scripts/kernel_census.py"""
import collections
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nanosim_amd import engine as E                      # noqa: E402
from nanosim_amd import metagenome as MG                 # noqa: E402
from nanosim_amd import model as M                       # noqa: E402
from nanosim_amd import transcriptome as T               # noqa: E402
from tests import kernel_classes as K                    # noqa: E402
from tests import oracle_lib as O                        # noqa: E402
from tests import test_gpu_kernel_classes as KC          # noqa: E402
from tests import test_gpu_metagenome as TM              # noqa: E402
from tests import test_gpu_parity as TP                  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def add(tot, exp, ref, p):
    if p.kmer_bias or not p.emit_records or p.n_reads == 0:
        return
    for which, c in KC.census(exp, ref, p).items():
        if which == "errlog" and p.kind != E.NS_KIND_ALIGNED:
            continue
        for k, v in c.items():
            if k.startswith("max_"):
                tot[which][k] = max(tot[which][k], int(v))
            elif k != "predicted_bytes":
                tot[which][k] += int(v)


def main():
    before = collections.defaultdict(collections.Counter)
    cases = collections.defaultdict(collections.Counter)
    with tempfile.TemporaryDirectory() as d:
        models, refs = KC.build_models(d), KC.build_refs()
        small, ref, circ = models["small"], refs["small"], refs["circ"]
        perfect = M.load_model(KC.PREFIX, perfect=True, fastq=True)
        for case in TP.CASES:
            p = E.make_params(**{**dict(seed=0x5EED1234ABCD, first_read=0, max_len=ref.max_chrom), **case})
            if p.n_reads == 0 or p.kmer_bias:
                continue
            big = p.use_lognormal and p.median_len >= 10000
            mdl = perfect if p.kind == E.NS_KIND_PERFECT else small
            add(before, O.generate(mdl, ref, p, bytes_per_read=400000 if big else 40000, events_per_read=60000 if big else 4000), ref, p)
        for r in (ref, circ):
            for kw in (dict(n_reads=300, emit_errlog=True), dict(n_reads=200, fastq=True, chimeric=True, emit_errlog=True),
                       dict(n_reads=100, kind=E.NS_KIND_UNALIGNED, fastq=True)):
                p = E.make_params(**{**dict(seed=987654321, first_read=3, max_len=r.max_chrom), **kw})
                add(before, O.generate(models["dense"], r, p), r, p)
        p = E.make_params(seed=77, first_read=0, n_reads=200, max_len=circ.max_chrom, emit_errlog=True)
        add(before, O.generate(small, circ, p), circ, p)
        for kw in (dict(kind=E.NS_KIND_UNALIGNED, n_reads=400, fastq=True), dict(kind=E.NS_KIND_UNALIGNED, n_reads=300, median_len=9000, sd_len=0.3),
                   dict(kind=E.NS_KIND_ALIGNED, n_reads=300, chimeric=True, emit_errlog=True)):
            p = E.make_params(seed=1234, first_read=0, max_len=circ.max_chrom, **kw)
            add(before, O.generate(small, circ, p, bytes_per_read=100000, events_per_read=20000), circ, p)
        os.chdir(ROOT)                                   # (the genome list names its files relative to the repository)
        meta_dir = os.path.join(GOLDEN, "meta")
        meta = MG.read_metagenome(os.path.join(meta_dir, "genome_list.tsv"), os.path.join(meta_dir, "dna_type_list.tsv"))
        abun = MG.read_abundance(os.path.join(meta_dir, "abundance.tsv"), meta.species)[1][0]
        infl = {sp: MG.inflate_abun(abun, sp, small.abun_inflation) for sp in abun}
        for case in TM.CASES:
            p = E.make_params(**{**dict(seed=0xFEED5EED77, first_read=0, max_len=meta.max_chrom, meta=True), **case})
            mdl = perfect if p.kind == E.NS_KIND_PERFECT else small
            if not p.kmer_bias and p.emit_records:
                add(before, O.generate_meta(mdl, meta, abun, infl if p.chimeric else None, p), meta.ref, p)
        trx_dir = os.path.join(GOLDEN, "trx")
        trx = T.read_transcriptome(os.path.join(trx_dir, "transcripts.fa"), os.path.join(trx_dir, "expression.tsv"),
                                   os.path.join(trx_dir, "polya.txt"), "guppy")
        p = E.make_params(seed=0xABCD1234, first_read=0, max_len=10 ** 9, trx=True, n_reads=300, fastq=True, emit_errlog=True)
        add(before, O.generate_trx(M.load_model(KC.PREFIX, transcriptome=True, fastq=True, homopolymer=True), trx, p), trx.ref, p)
        for cid, rname, mname, case, reach in KC.CASES:
            p, exp, cen = KC.oracle_case(cid, rname, mname, case, models, refs)
            add(cases, exp, refs[rname], p)
    for which in ("record", "dense", "errlog"):
        print("%-46s %9s %9s" % (which + "_classes", "before", "cases"))
        for k in sorted(set(before[which]) | set(cases[which])):
            print("%-46s %9d %9d" % (k, before[which].get(k, 0), cases[which].get(k, 0)))
        print()


if __name__ == "__main__":
    main()
