"""The mode functions of nanosim_amd.characterize (train_genome, train_metagenome, train_transcriptome, quantify_reads, detect_ir: what
`python -m nanosim_amd.read_analysis` runs) on CPU: every file a mode writes equals what the documented stage calls of
characterize/__init__.py write when they are made by hand with the PATH readers — which are pinned against the reference stage by
stage.  The engine is a stand-in that joins the host builds of the stages' walks (the tests/*_host.cpp of their own tests); the inputs
are composed from the fixtures.  tests/test_gpu_zzzzzzzzzzzz_read_analysis.py runs the command itself on the GPU against the same
expectation (`by_hand`, `same_files`)."""
import ctypes as C
import gzip
import json
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine, model
from tests import bam_lib, mixfit_lib, test_basequal, test_besthit, test_ir_train, test_quantify, test_read_lengths, test_sam_index, test_sam_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_engine():
    """an object that stands in for an Engine for every call the modes make: each ns_* is the engine's code compiled for the host"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libcs_hist_host.so")
    mine = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", mine, os.path.join(ROOT, "tests", "cs_hist_host.cpp")])
    os.replace(mine, so)
    H = C.CDLL(so)
    H.csh_host_count.restype = C.c_int
    H.csh_host_count.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5

    def cs_histograms(ctx, cs, nbytes, off, n, href):
        h = href._obj
        misc = np.zeros(4, dtype=np.uint64)
        H.csh_host_count(cs, off, n, h.cap_match2d, C.addressof(h.dic), h.match_list, C.addressof(h.error_list), C.addressof(h.first_error), misc.ctypes.data)
        h.max_match, h.n_match2d_overflow, h.n_skip = int(misc[0]), int(misc[1]), int(misc[2])
        return 0

    def check(rc):
        if rc:
            raise engine.EngineError("host walk: error %d" % rc)
    L = types.SimpleNamespace(ns_cs_histograms=cs_histograms)
    for part in (test_sam_index.build_host_walk(), test_basequal.build_host_walk(), test_sam_pairs.build_host_walk(), mixfit_lib.build_host(),
                 test_read_lengths.build_host_walk(), test_quantify.build_host_engine(), test_ir_train.build_host_walk(), test_besthit.build_host_walk()):
        vars(L).update(vars(part.L))
    return types.SimpleNamespace(ctx=None, _check=check, L=L, close=lambda: None)


@pytest.fixture(scope="module")
def host():
    return build_host_engine()


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------------
_OPS = re.compile(r"(\d+)([MIDNSHP=X])")


def decorate(line: str, rng) -> str:
    """a SAM record with SEQ, QUAL, NM:i, MD:Z and cs:Z that agree with its CIGAR: the bases of runs of 1-6 equal letters, 1-4 mismatches from
    the second column of every M block of 6 columns or more, qualities over the whole range; an unmapped record gets SEQ and QUAL"""
    fld = line.rstrip("\n").split("\t")
    flag, cigar = int(fld[1]), fld[5]
    keep = [t for t in fld[11:] if t[:5] not in ("NM:i:", "MD:Z:", "cs:Z:")]

    def bases(n):
        out = []
        while sum(map(len, out)) < n:
            out.append("ACGT"[int(rng.integers(0, 4))] * int(rng.integers(1, 7)))
        return "".join(out)[:n]

    def quals(n):
        return rng.integers(34, 127, n).astype(np.uint8).tobytes().decode()
    if flag & 0x4 or cigar == "*":
        n = int(rng.integers(20, 200))
        fld[9], fld[10] = bases(n), quals(n)
        return "\t".join(fld[:11] + keep) + "\n"
    seq, cs, md, run, nm = [], [], [], 0, 0
    for n, op in ((int(a), b) for a, b in _OPS.findall(cigar)):
        if op == "S":
            seq.append(bases(n))
        elif op == "I":
            ins = bases(n)
            seq.append(ins)
            cs.append("+" + ins.lower())
            nm += n
        elif op == "D":
            gone = bases(n)
            cs.append("-" + gone.lower())
            md.append("%d^%s" % (run, gone))
            run, nm = 0, nm + n
        elif op == "M":
            b = bases(n)
            if n >= 6:
                k = int(rng.integers(1, 5))                 # a run of 1-4 mismatches from the second column on
                refs = ["ACGT"[("ACGT".index(c) + 1) % 4] for c in b[1:1 + k]]
                cs.append(":1" + "".join("*%s%s" % (r.lower(), c.lower()) for r, c in zip(refs, b[1:1 + k])) + ":%d" % (n - 1 - k))
                md.append("%d%s" % (run + 1, refs[0]) + "".join("0" + r for r in refs[1:]))
                run, nm = n - 1 - k, nm + k
            else:
                cs.append(":%d" % n)
                run += n
            seq.append(b)
    md.append("%d" % run)
    fld[9] = "".join(seq)
    fld[10] = quals(len(fld[9])) if fld[9] else "*"
    if not fld[9]:
        fld[9] = "*"
    return "\t".join(fld[:11] + ["NM:i:%d" % nm] + keep + ["MD:Z:" + "".join(md), "cs:Z:" + "".join(cs)]) + "\n"


def composed_sam(seed: int = 20261021, fixture: str = "reference_chimeric_train.json.gz", key: str = "sam", clip: bool = False) -> str:
    """the SAM text of a fixture with every record decorated: a few hundred records with cs, MD, NM, SA, SEQ and QUAL.  clip: every
    CIGAR gets soft clips around it first (the length models need heads and tails: a KDE of no value cannot be fitted)"""
    rng = np.random.default_rng(seed)
    with gzip.open(os.path.join(ROOT, "tests", "golden", fixture), "rt") as f:
        text = json.load(f)[key]

    def clipped(line, i):
        fld = line.split("\t")
        if clip and fld[5] != "*":
            fld[5] = "%dS%s%dS" % (i % 7 + 1, fld[5], i % 5 + 2)
        return "\t".join(fld)
    return "".join(x if x.startswith("@") else decorate(clipped(x, i), rng) for i, x in enumerate(text.splitlines(True)))


def write(tmp, name, text, mode="w"):
    path = os.path.join(str(tmp), name)
    with open(path, mode) as f:
        f.write(text)
    return path


def genome_inputs(tmp):
    """-> dict(sam, bam, reads, list): the composed alignment as SAM and as BAM, a reads file name for -i (not read), a metagenome list"""
    text = composed_sam()
    return dict(sam=write(tmp, "aln.sam", text), bam=write(tmp, "aln.bam", bam_lib.sam_to_bam(text), "wb"), reads=write(tmp, "reads.fq", ""),
                list=write(tmp, "genomes.tsv", "spA\tspA.fa\t75.0\nspB\tspB.fa\t25.0\n"), text=text)


def transcriptome_inputs(tmp):
    """-> dict(t, g, annot, reads): the intron-retention fixture's two alignments, decorated (the genome one without the records whose
    CIGAR the length walk refuses), and its annotation"""
    fx = test_ir_train.load_fixture()
    t = composed_sam(1, "reference_ir_train.json.gz", "t_sam", clip=True)
    g = "".join(x for x in composed_sam(2, "reference_ir_train.json.gz", "g_sam").splitlines(True)
                if x.startswith("@") or not re.search(r"[HPX=]", x.split("\t")[5]))
    return dict(t=write(tmp, "t.sam", t), g=write(tmp, "g.sam", g), annot=write(tmp, "annot.gff3", fx["gff"]), reads=write(tmp, "reads.fa", ""))


# ---- the expectation: the documented stage calls, made by hand with the path readers ---------------------------------------------------------------
def by_hand(what: str, prefix: str, eng, inp: dict) -> None:
    ch = characterize
    if what in ("genome -c -hp --fastq", "metagenome -c -q"):
        meta = what.startswith("meta")
        refs, recs, unaligned, strand = ch.chimeric(prefix, inp["sam"], eng, pickles=False, quantify="meta" if meta else None)
        ch.read_lengths(prefix, refs, recs, eng, unaligned, strand, pickles=False, merge=True)
        ch.hist(prefix, ch.cs_from_sam(prefix + "_primary.sam"), eng)
        ch.model_fitting(prefix, eng)
        if not meta:
            ch.homopolymer_lengths_from_sam(prefix, ch.sam_records(prefix + "_primary.sam"), eng, min_hp_len=5, maf_file=True)
            ch.base_qualities(prefix, ch.quals_from_sam(prefix + "_primary.sam")[0], ch.quals_from_sam(inp["sam"])[1], eng)
    elif what == "genome":
        refs, recs, unaligned, strand = ch.primary_and_unaligned(inp["sam"])
        lines = inp["text"].splitlines(True)
        write(os.path.dirname(prefix), os.path.basename(prefix) + "_primary.sam",
              "".join(x for x in lines if x.startswith("@")) + "".join(x for x in lines if not x.startswith("@") and not int(x.split("\t")[1]) & 0x904))
        ch.read_lengths(prefix, refs, recs, eng, unaligned, strand, pickles=False)
        ch.hist(prefix, ch.cs_from_sam(prefix + "_primary.sam"), eng)
        ch.model_fitting(prefix, eng)
    elif what.startswith("transcriptome"):
        refs, recs, unaligned, strand = ch.primary_and_unaligned(inp["t"])
        for key, name in (("t", "_transcriptome_primary.sam"), ("g", "_genome_primary.sam")):
            with open(inp[key]) as f:
                lines = f.readlines()
            write(os.path.dirname(prefix), os.path.basename(prefix) + name,
                  "".join(x for x in lines if x.startswith("@")) + "".join(x for x in lines if not x.startswith("@") and not int(x.split("\t")[1]) & 0x904))
        if "--no_intron_retention" not in what:
            ch.add_introns(inp["annot"], prefix + "_added_intron_final.gff3")
            ch.intron_retention(prefix, prefix + "_added_intron_final.gff3", inp["g"], inp["t"], eng)
        ch.read_lengths(prefix, refs, recs, eng, unaligned, strand, mode="transcriptome", genome_records=ch.length_records(prefix + "_genome_primary.sam")[1],
                        pickles=False)
        ch.hist(prefix + "_genome", ch.cs_from_sam(prefix + "_genome_primary.sam"), eng)
        ch.model_fitting(prefix, eng)
    elif what == "quantify -e meta":
        ch.quantify(prefix, inp["sam"], eng, "meta", expected={"spA": 75.0, "spB": 25.0}, normalize=False)
    elif what == "quantify -e trans":
        ch.quantify(prefix, inp["sam"], eng, "trans", normalize=False)
    elif what == "detect_ir":
        ch.add_introns(inp["annot"], prefix + "_added_intron_final.gff3")
        ch.intron_retention(prefix, prefix + "_added_intron_final.gff3", inp["g"], inp["t"], eng)
    else:
        raise KeyError(what)


def same_files(got_prefix: str, want_prefix: str, ignore=()) -> list:
    """every file of one prefix equals the file of the other byte for byte, `_kde.npz` array by array; -> the suffixes"""
    def files(prefix):
        d, b = os.path.split(prefix)
        return sorted(x[len(b):] for x in os.listdir(d) if x.startswith(b + "_") and not x.endswith(".pkl") and x[len(b):] not in ignore)
    got, want = files(got_prefix), files(want_prefix)
    assert got == want, (got, want)
    for suffix in got:
        if suffix == "_kde.npz":
            with np.load(got_prefix + suffix) as a, np.load(want_prefix + suffix) as b:
                assert sorted(a.files) == sorted(b.files)
                for k in a.files:
                    assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        else:
            with open(got_prefix + suffix, "rb") as a, open(want_prefix + suffix, "rb") as b:
                assert a.read() == b.read(), suffix
    return got


def prefixes(tmp):
    for d in ("got", "want"):
        os.makedirs(os.path.join(str(tmp), d), exist_ok=True)
    return os.path.join(str(tmp), "got", "training"), os.path.join(str(tmp), "want", "training")


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
def test_composed_alignment_has_what_the_stages_need():
    text = composed_sam()
    recs = [x.split("\t") for x in text.splitlines() if not x.startswith("@")]
    assert 300 < len(recs) < 1000 and all(len(r) >= 11 for r in recs)
    mapped = [r for r in recs if not int(r[1]) & 4]
    assert all(any(t.startswith(p) for t in r[11:]) for r in mapped for p in ("cs:Z:", "MD:Z:", "NM:i:")) and any(t.startswith("SA:Z:") for r in mapped for t in r[11:])
    assert all(r[10] != "*" and len(r[9]) == len(r[10]) for r in mapped) and any(int(r[1]) & 4 and r[10] != "*" for r in recs)
    cs = "".join(t for r in mapped for t in r[11:] if t.startswith("cs:Z:"))
    assert "*" in cs and "+" in cs and "-" in cs and any("S" in r[5] for r in mapped)          # every quality class: mis, ins, match, ht, unmapped


def test_chimeric_homopolymer_fastq_from_sam_and_bam(host, tmp_path):
    inp = genome_inputs(tmp_path)
    got, want = prefixes(tmp_path)
    by_hand("genome -c -hp --fastq", want, host, inp)
    said = []
    table = characterize.train_genome(got, inp["sam"], inp["reads"], host, chimeric_reads=True, homopolymer=True, fastq=True, pickles=False, log=said.append)
    assert said == ["Processing alignment file: sam", "Aligned reads analysis", "Unaligned reads analysis", "match and error models", "Model fitting",
                    "Analyzing homopolymer lengths and estimating model parameters", "Analyzing base qualities and estimating model parameters"]
    names = same_files(got, want)
    assert {"_primary.sam", "_kde.npz", "_chimeric_info", "_model_profile", "_strandness_rate", "_reads_alignment_rate"} <= set(names)
    assert "_base_qualities_model_parameters.tsv" in names and "_processed.maf" in names and "_error_markov_model" in names and len(table) > 300
    model.load_model(got, chimeric=True)
    shutil.rmtree(os.path.dirname(got))
    os.makedirs(os.path.dirname(got))
    characterize.train_genome(got, inp["bam"], inp["reads"], host, chimeric_reads=True, homopolymer=True, fastq=True, pickles=False)
    same_files(got, want)


def test_without_chimeric_the_primary_lines_are_written(host, tmp_path):
    inp = genome_inputs(tmp_path)
    got, want = prefixes(tmp_path)
    by_hand("genome", want, host, inp)
    characterize.train_genome(got, inp["sam"], inp["reads"], host)
    assert "_primary.sam" in same_files(got, want)
    model.load_model(got)


def test_metagenome_chimeric_quantification(host, tmp_path):
    inp = genome_inputs(tmp_path)
    got, want = prefixes(tmp_path)
    by_hand("metagenome -c -q", want, host, inp)
    characterize.train_metagenome(got, inp["sam"], inp["reads"], host, chimeric_reads=True, quantification=True,
                                  expected=characterize.expected_abundance(inp["list"]), pickles=False)
    assert "_quantification.tsv" in same_files(got, want)


@pytest.mark.parametrize("ir", [True, False])
def test_transcriptome(host, tmp_path, ir):
    inp = transcriptome_inputs(tmp_path)
    got, want = prefixes(tmp_path)
    by_hand("transcriptome" if ir else "transcriptome --no_intron_retention", want, host, inp)
    characterize.train_transcriptome(got, inp["t"], inp["g"], inp["reads"], host, annotation=inp["annot"], ir=ir)       # (pickles as the command line: when scikit-learn is there)
    names = same_files(got, want)
    assert ("_IR_markov_model" in names) == ir and "_genome_primary.sam" in names and "_transcriptome_primary.sam" in names


def test_quantify_and_detect_ir(host, tmp_path):
    inp = dict(genome_inputs(tmp_path), **{k: v for k, v in transcriptome_inputs(tmp_path).items() if k != "reads"})
    got, want = prefixes(tmp_path)
    for kind in ("meta", "trans"):
        by_hand("quantify -e " + kind, want, host, inp)
        characterize.quantify_reads(got, inp["sam"], host, kind, expected=characterize.expected_abundance(inp["list"]))
        assert same_files(got, want) == ["_quantification.tsv"]
    by_hand("detect_ir", want, host, inp)
    characterize.detect_ir(got, inp["annot"], inp["g"], inp["t"], host)
    assert same_files(got, want) == ["_IR_info", "_IR_markov_model", "_added_intron_final.gff3", "_quantification.tsv"]


def test_a_maf_alignment_goes_the_maf_way(tmp_path):
    host = test_besthit.build_host_walk()
    fx = test_besthit.load_fixture()
    src = os.path.join(ROOT, "tests", "golden", "model_small")
    maf_path, reads_path = test_besthit.write_inputs(fx, tmp_path)
    got, want = prefixes(tmp_path)
    for p in (got, want):
        shutil.copy(os.path.join(src, "training_model_profile"), p + "_model_profile")
    characterize.train_genome_from_maf(want, maf_path, reads_path, host, model_fit=False, pickles=False)
    characterize.train_genome(got, maf_path, reads_path, host, model_fit=False, pickles=False)
    assert "_besthit.maf" in same_files(got, want)
    with pytest.raises(ValueError, match="MAF"):
        characterize.train_genome(got, maf_path, reads_path, host, fastq=True)
