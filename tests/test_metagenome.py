"""Metagenome mode: host loader + the oracle's assign_species / extract_read restatements pinned by
tape replay against the reference (tests/golden/reference_metagenome.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from nanosim_amd import metagenome as MG
from nanosim_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = os.path.join(ROOT, "tests", "golden", "meta")


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "reference_metagenome.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def meta_ref():
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        return MG.read_metagenome(os.path.join(META, "genome_list.tsv"), os.path.join(META, "dna_type_list.tsv"))
    finally:
        os.chdir(cwd)


def test_loader_matches_read_profile(fx, meta_ref):
    assert meta_ref.species == fx["species"]
    lens = np.diff(meta_ref.ref.chrom_off.astype(np.int64))
    ci = 0
    for si, sp in enumerate(meta_ref.species):
        assert meta_ref.species_chrom_off[si] == ci
        for key, ln in fx["seq_len"][sp]:
            assert meta_ref.ref.names[ci] == sp + "-" + key and lens[ci] == ln
            assert bool(meta_ref.ref.circular[ci]) == (fx["dna_type"][sp][key] == "circular")
            ci += 1
    assert ci == len(meta_ref.ref.names)
    assert meta_ref.max_chrom == max(fx["max_chrom"].values())
    assert meta_ref.total_len() == fx["abundance_var"]["total_len"]
    numbers, samples = MG.read_abundance(os.path.join(META, "abundance.tsv"), meta_ref.species)
    assert samples == [fx["abun"]["sample0"], fx["abun"]["sample1"]]
    mdl = M.load_model(os.path.join(ROOT, "tests", "golden", "model_small", "training"), chimeric=True)
    assert [mdl.split_counts(n) for n in numbers] == list(zip(fx["number_aligned"], fx["number_unaligned"]))
    assert mdl.abun_inflation == fx["abun_inflation"] and mdl.segment_mean == fx["segment_mean"]
    for sp, v in fx["abun_inflated"].items():
        assert MG.inflate_abun(fx["abun"]["sample0"], sp, mdl.abun_inflation) == pytest.approx(v, rel=1e-15)


def test_abundance_variation_tape(fx):
    av = fx["abundance_var"]
    got = MG.add_abundance_var(fx["abun"]["sample1"], av["total_len"], -0.5, 0.5, iter(av["u"]))
    assert got.keys() == av["result"].keys()
    for k in got:
        assert got[k] == pytest.approx(av["result"][k], rel=1e-14)


def test_assign_species_tape_replay(fx, meta_ref):
    from tests import oracle_lib as O
    L = O.lib()
    mg, keep = O.make_meta(meta_ref, fx["abun"]["sample0"], fx["abun_inflated"])
    for case in fx["assign_species"]:
        lens = np.array(case["lengths"], dtype=np.float64)
        segs = np.array(case["segs"], dtype=np.int32)
        cur = np.array([case["current"][sp] for sp in meta_ref.species], dtype=np.float64)
        d, k2 = O.make_tape(case["u"])
        sp_out = np.zeros(len(lens), dtype=np.uint16)
        len_out = np.zeros(len(lens), dtype=np.float64)
        seg_out = np.zeros(len(segs), dtype=np.int32)
        n = L.nso_assign_species(C.byref(mg), lens.ctypes.data, len(lens), segs.ctypes.data, len(segs), cur.ctypes.data, C.byref(d), 0,
                                 sp_out.ctypes.data, len_out.ctypes.data, seg_out.ctypes.data)
        assert not d.tape_err and d.i_u == len(case["u"])
        assert n == len(case["species"])
        assert [meta_ref.species[i] for i in sp_out[:n]] == case["species"]
        assert len_out[:n].tolist() == case["out_lengths"]
        assert seg_out[:n].tolist() == case["out_segs"]            # S:811: the segment list is cut at the segment pointer


def test_extract_read_metagenome_tape_replay(fx, meta_ref):
    from tests import oracle_lib as O
    L = O.lib()
    mg, keep = O.make_meta(meta_ref, fx["abun"]["sample0"], None)
    bases = O.normalise_bases(meta_ref.ref.bases)
    chrom, pos = C.c_uint32(), C.c_uint64()
    n_warn = 0
    for case in fx["extract_read"]:
        d, k2 = O.make_tape(case["u"])
        sp = -1 if case["species"] is None else meta_ref.species.index(case["species"])
        rc = L.nso_extract_meta(C.byref(mg), meta_ref.ref.chrom_off.ctypes.data, meta_ref.ref.circular.ctypes.data, case["length"], sp,
                                C.byref(d), 0, 0, C.byref(chrom), C.byref(pos))
        assert rc >= 0 and not d.tape_err and d.i_u == len(case["u"])
        n_warn += rc
        assert "%s_%d" % (meta_ref.ref.names[chrom.value], pos.value) == case["name"]
        # the extracted bases (with wrap-around on circular chromosomes) start / end like the reference's
        c0, c1 = int(meta_ref.ref.chrom_off[chrom.value]), int(meta_ref.ref.chrom_off[chrom.value + 1])
        idx = c0 + (pos.value + np.arange(case["length"])) % (c1 - c0)
        raw = meta_ref.ref.bases[idx]
        assert bytes(raw[:30]).decode() == case["head"] and bytes(raw[-30:]).decode() == case["tail"]
    assert n_warn > 0


def _species_of_piece(meta_ref, chrom):
    return np.searchsorted(meta_ref.species_chrom_off, chrom, side="right") - 1


@pytest.mark.parametrize("chimeric", [False, True])
def test_oracle_metagenome_batches_match_reference_runs(fx, meta_ref, chimeric):
    """8 workers x 12 500 reads of the reference vs 8 oracle batches of the same size: species base fractions (incl. the fall-back to
    other species when a chromosome is too short), read lengths (KS <= 1 %), chimeric share, one strand per pass, name grammar."""
    from nanosim_amd import engine as E
    from tests import oracle_lib as O
    from tests.test_distributions import ks_vs_quantiles
    run = fx["runs"]["chimeric" if chimeric else "plain"]
    mdl = M.load_model(os.path.join(ROOT, "tests", "golden", "model_small", "training"), chimeric=True)
    abun = fx["abun"]["sample0"]
    infl = {sp: MG.inflate_abun(abun, sp, mdl.abun_inflation) for sp in abun} if chimeric else None
    bases = np.zeros(len(meta_ref.species))
    lens, n_chim, strands_single = [], 0, 0
    per = fx["runs"]["reads_per_worker"]["chimeric" if chimeric else "plain"]
    for w in range(8):
        p = E.make_params(seed=900 + w, first_read=w * per, n_reads=per, chimeric=chimeric, max_len=meta_ref.max_chrom)
        out = O.generate_meta(mdl, meta_ref, abun, infl, p)
        rd, pc = out["reads"], out["pieces"]
        aligned = pc[pc["kind"] == 0]
        sp = _species_of_piece(meta_ref, aligned["chrom"])
        bases += np.bincount(sp, weights=aligned["ref_len"], minlength=len(bases))
        lens.append(rd["seq_len"])
        n_chim += int(np.sum(rd["n_pieces"] > 1))
        strands_single += len(set(rd["reversed"].tolist())) == 1
        if w == 0:
            names = [x[1:].decode() for x in out["records"].tobytes().split(b"\n")[0:-1:2]]
            assert names[0].split("_aligned_")[1].startswith("0_")
            for nm in names[:200]:
                body = nm.split("_aligned_")[0]
                for comp in body.split(";"):
                    assert comp.startswith("gap_") or any(comp.startswith(s + "-") for s in meta_ref.species), nm
    frac = bases / bases.sum()
    ref_tot = sum(run["bases"].values())
    for i, spn in enumerate(meta_ref.species):
        assert abs(frac[i] - run["bases"][spn] / ref_tot) < 0.01, (spn, frac[i], run["bases"][spn] / ref_tot)
    lens = np.concatenate(lens)
    assert abs(lens.mean() / run["mean_len"] - 1) < 0.01
    assert ks_vs_quantiles(lens, run["q_len"]) <= 0.01
    ref_chim = sum(wk["n_chim"] for wk in run["workers"])
    if chimeric:
        # ~4 800 chimeric reads among 100 000 on either side: one standard deviation of the difference of two such counts is ~100 (2 %).
        # Measured at these seeds: oracle 4 704, reference 4 799 (ratio 0.980, one sigma).  Gate: 8 % = four sigma.
        assert abs(n_chim / ref_chim - 1.0) <= 0.08, (n_chim, ref_chim)
    else:
        assert n_chim == 0
    # S:860: the strand is drawn once per pass, so workers that finish in one pass have a single strand
    assert strands_single >= 1 or sum(len(wk["strands"]) == 1 for wk in run["workers"]) == 0


def test_oracle_perfect_metagenome_batches_match_reference_runs(fx, meta_ref):
    """--perfect workers (S:838-842, 879-910): species base fractions, read lengths, one strand per pass, descending lengths,
    consecutive numbering, quotas that are never updated."""
    from nanosim_amd import engine as E
    from tests import oracle_lib as O
    from tests.test_distributions import ks_vs_quantiles
    run = fx["runs"]["perfect"]
    mdl = M.load_model(os.path.join(ROOT, "tests", "golden", "model_small", "training"), perfect=True)
    abun = fx["abun"]["sample0"]
    bases = np.zeros(len(meta_ref.species))
    lens = []
    per = fx["runs"]["reads_per_worker"]["perfect"]
    for w in range(8):
        p = E.make_params(seed=300 + w, first_read=w * per, n_reads=per, kind=E.NS_KIND_PERFECT, max_len=meta_ref.max_chrom, meta=True)
        out = O.generate_meta(mdl, meta_ref, abun, None, p)
        rd, pc = out["reads"], out["pieces"]
        assert np.all(pc["n_ev"] == 0) and np.all(rd["head"] == 0) and np.all(rd["tail"] == 0)
        assert np.all(out["species_bases"] == 0)                              # S:1001-1002 is not reached with --perfect
        sp = _species_of_piece(meta_ref, pc["chrom"])
        bases += np.bincount(sp, weights=pc["ref_len"], minlength=len(bases))
        lens.append(rd["seq_len"])
        if int(rd["attempts"].max()) == 0:                                    # a single pass: one strand, lengths sorted descending
            assert len(set(rd["reversed"].tolist())) == 1
            assert np.all(np.diff(rd["seq_len"].astype(np.int64)) <= 0)
        names = [x[1:].decode() for x in out["records"].tobytes().split(b"\n")[0:-1:2]]
        for i, nm in enumerate(names[:50]):
            f = nm.partition("_perfect_")[2].split("_")
            assert int(f[0]) == w * per + i and f[2] == "0" and f[4] == "0" and int(f[3]) == rd["seq_len"][i]
    frac = bases / bases.sum()
    tot = sum(run["bases"].values())
    for i, spn in enumerate(meta_ref.species):
        assert abs(frac[i] - run["bases"][spn] / tot) < 0.005
    lens = np.concatenate(lens)
    assert abs(lens.mean() / run["mean_len"] - 1) < 0.01 and ks_vs_quantiles(lens, run["q_len"]) <= 0.01
    assert all(wk["sorted_desc_frac"] == 1.0 and len(wk["strands"]) == 1 and wk["indices"][:3] == [0, 1, 2] for wk in run["workers"])


def _pass_log_run(meta_ref, abun, chimeric, **kw):
    from nanosim_amd import engine as E
    from tests import oracle_lib as O
    mdl = M.load_model(os.path.join(ROOT, "tests", "golden", "model_small", "training"), chimeric=True, fastq=True)
    infl = {sp: MG.inflate_abun(abun, sp, mdl.abun_inflation) for sp in abun} if chimeric else None
    kw = dict(dict(seed=0xE7A05710, first_read=0, n_reads=300, max_len=meta_ref.max_chrom), **kw)
    p = E.make_params(meta=True, chimeric=chimeric, **kw)
    try:
        O.generate_meta(mdl, meta_ref, abun, infl, p)
        err = None
    except RuntimeError as e:
        err = e
    np_spec, np_ = O.meta_pass_log()
    return np_spec.astype(np.int64), np_.astype(np.int64), err


QUOTA_TABLES = [
    (50.0, 30.0, 20.0),                  # the golden sample
    (1e6, 1.0, 0.0),                     # extreme ratio, one species without a share
    (0.0, 0.0, 1.0),                     # one species takes every read
    (1.0, 1e-300, 1e-300),               # quotas below one base
    (5e-324, 5e-324, 0.0),               # subnormal abundances: total * abun rounds to whole bases
    (1.0, 0.002, 0.001),                 # quotas of about one read length
]


@pytest.mark.parametrize("table", QUOTA_TABLES)
@pytest.mark.parametrize("chimeric", [False, True])
def test_metagenome_quotas_are_exhausted_only_when_no_quota_is_finite(meta_ref, table, chimeric):
    """np_spec: the reads a pass's lengths can cover; np: the reads assign_species (S:758-811) assigns.  np < np_spec needs every quota
    used up before the lengths are.  With finite quotas that cannot happen: quota[s] = total * abun[s] / sum(abun) - current[s] adds up
    to bases_to_add over all species, so the positive quotas add up to at least bases_to_add; a segment of length l lowers the remaining
    lengths by l and the positive quotas by min(l, quota) <= l (the fall-back to a species whose quota is below l, S:787-788, spends only
    what that species had).  Positive quota >= remaining lengths > 0 holds to the last segment, up to the rounding of the quota sums
    (a few ulp of the total: ~1e-9 bases for 10^6 bases, at most half a base for subnormal abundances), far below any length a pass draws.
    So np == np_spec in every pass of these batches: extreme ratios, species with no share, narrow length windows (many passes), chimeric
    walks that charge the previous species."""
    abun = dict(zip(meta_ref.species, table))
    for kw in (dict(), dict(min_len=3000, max_len=9000), dict(median_len=3000, sd_len=0.9)):
        np_spec, np_, err = _pass_log_run(meta_ref, abun, chimeric, **kw)
        assert err is None and len(np_spec) >= 1
        assert np.array_equal(np_, np_spec), (kw, np_spec, np_)
    assert len(_pass_log_run(meta_ref, abun, chimeric, min_len=3000, max_len=9000)[0]) > 3     # (many passes were walked)


@pytest.mark.parametrize("table", [(0.0, 0.0, 0.0), (float("inf"), 1.0, 1.0)])
@pytest.mark.parametrize("chimeric", [False, True])
def test_metagenome_quotas_without_finite_share_assign_no_read(meta_ref, table, chimeric):
    """The inputs that do reach np < np_spec: an abundance table whose quotas are not finite (all zero: 0 / 0; an infinite abundance:
    inf / inf and 0 - current).  No species has quota > 0, the walk stops at the first segment (random.choice([]) raises in the reference,
    S:788), so np == 0 < np_spec in every pass, no read is ever accepted, and the batch ends at the attempt limit (1000 passes)."""
    abun = dict(zip(meta_ref.species, table))
    np_spec, np_, err = _pass_log_run(meta_ref, abun, chimeric, n_reads=20)
    assert err is not None and "-16" in str(err)
    assert len(np_spec) == 1000
    assert np.all(np_spec > 0) and np.all(np_ == 0)


def test_pass_log_is_reset_by_every_metagenome_call(meta_ref):
    """the oracle's pass log belongs to the last call: an unaligned metagenome call (no passes) leaves it empty"""
    abun = dict(zip(meta_ref.species, (50.0, 30.0, 20.0)))
    assert len(_pass_log_run(meta_ref, abun, False)[0]) >= 1
    from nanosim_amd import engine as E
    assert len(_pass_log_run(meta_ref, abun, False, kind=E.NS_KIND_UNALIGNED)[0]) == 0
