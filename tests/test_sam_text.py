"""The seven readers of SAM text (nanosim_amd.characterize: cs_from_sam, quals_from_sam, sam_records, length_records,
primary_and_unaligned, chimeric_records, _mapped_records) pinned where they differ: the minimum field count, the treatment of a `*`
CIGAR / SEQ / QUAL, the FLAG bits dropped, the tags read, what is collected and every ValueError.  One small SAM text, and variants of
it without the records that stop one reader or another; what every reader returned or raised on every variant before the readers
shared their loop is stored in tests/golden/sam_readers.json (tests/golden/make_sam_readers_golden.py, which takes the texts and
`observe` from here)."""
import json
import os

import numpy as np
import pytest

from nanosim_amd import characterize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADER = ("@HD\tVN:1.6\tSO:unsorted\n"
          "@SQ\tSN:chr1\tLN:1000\n"
          "@SQ\tSN:chr2\tLN:500\n"
          "@SQ\tSN:nolen\n"                                 # no LN: not a reference of any reader
          "@PG\tID:minimap2\tPN:minimap2\n")
Q19 = "IIIIHHHHGGGGFFFFEEE"
RECORDS = (                                                 # (name of the record in VARIANTS, its line)
    ("short5", "short5\t0\tchr1\t1\t60\n"),                                                                     # fewer than 6 fields
    ("short8", "short8\t0\tchr1\t5\t60\t4M\t*\t0\n"),                                                           # 6 - 10 fields
    ("fwd", "fwd\t0\tchr1\t11\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tNM:i:0\tcs:Z::10\n"),                    # cs only
    ("rev", "rev\t16\tchr2\t21\t60\t2S8M1I4M2D3M1S\t*\t0\t0\tACGTACGTACGTACGTACG\t" + Q19 + "\tNM:i:4\tMD:Z:3A8^GT3\n"),   # MD only
    ("clip", "clip\t0\tchr1\t101\t60\t3H4S10M5S2H\t*\t0\t0\tACGTACGTACGTACGTACG\t" + Q19 + "\tNM:i:0\tcs:Z::10\tMD:Z:10\t"
             "SA:Z:chr2,301,+,12S7M,60,0;\n"),                                                                  # cs and MD, clips, SA
    ("supp", "clip\t2048\tchr2\t301\t60\t12H7M\t*\t0\t0\tACGTACG\tIIIIIII\tNM:i:0\tcs:Z::7\n"),                 # supplementary, H only
    ("sec", "fwd\t256\tchr2\t51\t0\t10M\t*\t0\t0\t*\t*\tNM:i:2\tMD:Z:10\n"),                                    # secondary, SEQ / QUAL `*`
    ("un1", "un1\t4\t*\t0\t0\t*\t*\t0\t0\tACGTAC\tIIIIII\n"),                                                   # unmapped with SEQ / QUAL
    ("un2", "un2\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"),                                                             # unmapped without
    ("nocigar", "nocigar\t0\tchr1\t201\t60\t*\t*\t0\t0\tACGT\tIIII\tNM:i:0\tMD:Z:4\n"),                         # mapped, CIGAR `*`
    ("noqual", "noqual\t16\tchr1\t301\t60\t6M\t*\t0\t0\tACGTAC\t*\tMD:Z:6\n"),                                  # mapped, QUAL `*`, no NM
    ("bare", "bare\t0\tchr1\t501\t60\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0\n"),                                      # neither cs nor MD
    ("badsa", "badsa\t0\tchr1\t401\t60\t5S5M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tNM:i:0\tcs:Z::5\tSA:Z:chrX,1,-,5M5S,60,0;\n"),   # SA entry on an unknown reference
    ("noref", "noref\t0\tnolen\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0\tcs:Z::4\n"),                            # a reference without a usable @SQ line
)
EARLY = "early\t2048\tchr2\t7\t60\t3H5M\t*\t0\t0\tACGTA\tIIIII\tNM:i:0\tcs:Z::5\n"                              # a supplementary record in front of the first primary

# variant -> (the records left out, lines put in front of the records)
VARIANTS = {
    "main": ((), ()),
    "cs_ok": (("bare",), ()),
    "quals_neither": (("noqual",), ()),
    "no_sq": (("noqual", "badsa"), ()),
    "chim_ok": (("noqual", "badsa", "noref"), ()),
    "all_ok": (("noqual", "bare", "badsa", "noref"), ()),
    "pairs_ok": (("fwd", "clip", "bare", "badsa", "noref"), ()),
    "pairs_hard_clip": (("fwd",), ()),
    "early_supp": (("noqual", "badsa", "noref"), (EARLY,)),
    "unmapped_only": (tuple(k for k, _ in RECORDS if k not in ("un1", "un2")), ()),
}

READERS = {
    "cs_from_sam": lambda p: characterize.cs_from_sam(p),
    "quals_from_sam": lambda p: characterize.quals_from_sam(p),
    "quals_from_sam_all": lambda p: characterize.quals_from_sam(p, primary_only=False),
    "sam_records": lambda p: characterize.sam_records(p),
    "length_records": lambda p: characterize.length_records(p),
    "primary_and_unaligned": lambda p: characterize.primary_and_unaligned(p),
    "chimeric_records": lambda p: characterize.chimeric_records(p),
    "_mapped_records": lambda p: list(characterize._mapped_records(p)),
}


def text_of(variant: str) -> str:
    drop, first = VARIANTS[variant]
    return HEADER + "".join(first) + "".join(line for k, line in RECORDS if k not in drop)


def plain(x):
    """what json stores of a reader's result: arrays and tuples (named ones too) as lists"""
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def observe(path: str) -> dict:
    """{reader: {"returns": ...} | {"raises": [type, message]}} for the SAM text at `path` (which the messages name as <path>)"""
    out = {}
    for name, reader in READERS.items():
        try:
            out[name] = {"returns": plain(reader(path))}
        except Exception as e:
            out[name] = {"raises": [type(e).__name__, str(e).replace(path, "<path>")]}
    return out


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "sam_readers.json")) as f:
        return json.load(f)


def test_text_is_small_and_holds_every_case():
    lines = text_of("main").splitlines() + [EARLY]
    assert len(lines) < 40
    recs = [x.split("\t") for x in lines if not x.startswith("@")]
    assert [x.split("\t")[0] for x in lines if x.startswith("@")] == ["@HD", "@SQ", "@SQ", "@SQ", "@PG"]
    assert any(len(r) < 6 for r in recs) and any(6 <= len(r) < 11 for r in recs)
    full = [r for r in recs if len(r) >= 11]
    flags = [int(r[1]) for r in full]
    assert {0, 16, 256, 2048, 4} <= set(flags)
    assert any(f & 4 and r[9] != "*" and r[10] != "*" for f, r in zip(flags, full)) and any(f & 4 and r[9] == "*" for f, r in zip(flags, full))
    assert any(not f & 4 and r[5] == "*" for f, r in zip(flags, full)) and any(not f & 4 and r[10] == "*" and r[5] != "*" for f, r in zip(flags, full))
    has = lambda r, tag: any(t.startswith(tag) for t in r[11:])
    assert {(has(r, "cs:Z:"), has(r, "MD:Z:")) for r in full if r[5] != "*"} == {(True, False), (False, True), (False, False), (True, True)}
    primary = [r for f, r in zip(flags, full) if not f & (4 | 256 | 2048)]
    assert any(has(r, "NM:i:") for r in primary) and any(not has(r, "NM:i:") for r in primary)
    assert any("SA:Z:chr2," in "\t".join(r) for r in primary) and any("SA:Z:chrX," in "\t".join(r) for r in primary)
    assert any(r[5] == "3H4S10M5S2H" for r in full) and any("H" in r[5] and "S" not in r[5] for r in full)
    assert int(text_of("early_supp").splitlines()[5].split("\t")[1]) & 2048


def test_every_reader_returns_somewhere_and_every_stop_is_met(golden):
    for name in READERS:
        assert any("returns" in golden[v][name] for v in VARIANTS), name
    raised = {golden[v][name]["raises"][1] for v in VARIANTS for name in READERS if "raises" in golden[v][name]}
    for piece in ("neither a cs nor an MD tag", "has no QUAL", "has no MD tag", "hard clip", "nolen, which has no @SQ line", "has no NM:i tag",
                  "chrX, which has no @SQ line", "in front of the first primary", "holds no primary alignment"):
        assert any(piece in m for m in raised), piece


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_readers_against_golden(variant, golden, tmp_path):
    path = str(tmp_path / "in.sam")
    with open(path, "w") as f:
        f.write(text_of(variant))
    got = json.loads(json.dumps(observe(path)))
    assert sorted(got) == sorted(golden[variant]) == sorted(READERS)
    for name in READERS:
        assert got[name] == golden[variant][name], (variant, name)
