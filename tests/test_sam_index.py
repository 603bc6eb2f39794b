"""Training side, the index of a SAM text ("SAM text: one indexed pass and the CLI") on CPU: the engine's masks, lists, tag
choice and rows (nanosim_amd/csrc/ns_sam_index.h, compiled for the host with the tabs offering one after the other; on the GPU the
k_sam_sep_*, k_sam_tags and k_sam_rows kernels of ns_train.h run it) against a restatement written out here — line.split("\\t"),
sam_tag, digits-only numbers — and characterize.SamTable, whose seven readers have to return or raise what the path readers do.
Behind the fixed texts: near misses of the four prefixes, records that end with FLAG or POS, texts of nothing but separators and two
separators at every pair of seams ("What the mutation audit leaves", says which mutant or device-only line each decides).
The check_* functions take an engine: tests/test_gpu_zzzzzzzzzzzz_sam_index.py runs them on the real one."""
import ctypes as C
import functools
import gzip
import itertools
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine, model
from tests import test_bam, test_chimeric_train, test_sam_pairs, test_sam_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIXES = ("cs:Z:", "MD:Z:", "NM:i:", "SA:Z:")


def build_host_walk():
    """an object that stands in for an Engine: its ns_sam_index is the engine's per-item code compiled for the host
    (tests/sam_index_host.cpp), its ns_bam_to_sam that of tests/test_bam.py; `order(k)` sets the order in which the tabs offer their
    fields, `span` is SAM_SPAN"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libsam_index_host.so")
    mine = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", mine, os.path.join(ROOT, "tests", "sam_index_host.cpp")])
    os.replace(mine, so)
    L = C.CDLL(so)
    L.sam_host_index.restype = C.c_int
    L.sam_host_index.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.sam_host_span.restype = C.c_uint64

    def check(rc):
        if rc:
            raise engine.EngineError("host walk: error %d" % rc)
    return types.SimpleNamespace(ctx=None, _check=check, order=L.sam_host_set_order, span=int(L.sam_host_span()),
                                 L=types.SimpleNamespace(ns_sam_index=L.sam_host_index, ns_bam_to_sam=test_bam.build_host().L.ns_bam_to_sam))


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


# ---- the texts -----------------------------------------------------------------------------------------------------------------------------
def fixture(name):
    with gzip.open(os.path.join(ROOT, "tests", "golden", name), "rt") as f:
        return json.load(f)


def composed_texts():
    """(the SAM text of reference_chimeric_train.json.gz, the records of reference_sam_pairs.json.gz as lines under its header, composed
    the way scripts/bench_sam_readers.py composes them)"""
    chim = fixture("reference_chimeric_train.json.gz")["sam"]
    header = [x for x in chim.splitlines(True) if x.startswith("@")]
    pairs = ["\t".join([q, str(flag), rname, str(pos), "60", cigar, "*", "0", "0", seq, "I" * len(seq), "NM:i:0", "MD:Z:" + md]) + "\n"
             for q, flag, rname, pos, cigar, md, seq in fixture("reference_sam_pairs.json.gz")["records"]]
    return chim, "".join(header) + "".join(pairs)


def rec(name, flag="0", *tags, rname="chr1", pos="7", cigar="4M", seq="ACGT", qual="IIII"):
    return "\t".join([name, flag, rname, pos, "60", cigar, "*", "0", "0", seq, qual] + list(tags)) + "\n"


# every rule of ns_sam_index.h in one text (no '\n' at its end: the last field is the four bytes `cs:Z`)
HAND = ("@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n" +
        rec("twice", "0", "NM:i:1", "cs:Z::4", "XX:Z:between", "NM:i:2", "cs:Z::3*ag", "MD:Z:4", "MD:Z:3A") +   # a tag given twice: the last wins
        "@CO\ta header line in the middle\n" +
        "\n" +                                                                                              # an empty line: a record of one empty field
        "five\t0\tchr1\t1\t60\n" +
        "ten\t16\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\n" +
        "adj\t0\t\tchr1\t1\t\t60\t4M\t*\t0\t0\tAC\tII\tMD:Z:2\n" +                                          # two adjacent tabs, twice
        rec("emptycs", "0", "cs:Z:", "SA:Z:chr1,5,+,4M,60,0;", "NM:i:0") +                                  # an empty value
        rec("early", "0", "NM:i:3", qual="cs:Z:notatag") +                                                  # field 10 is no tag
        rec("short", "0", "NM:i", "cs:Z", "MD:Z:", "SA:Z") +                                                # fields shorter than five bytes
        rec("blank", " 16", "NM:i:0", "cs:Z::4") + rec("plus", "+16", "NM:i:0", "cs:Z::4") + rec("under", "1_6", "NM:i:0", "cs:Z::4") +
        rec("big", "4294967296", "NM:i:0", "cs:Z::4") + rec("max", "4294967295", "NM:i:4294967295", pos="4294967295") +
        rec("eleven", "00000000016", "NM:i:0", "cs:Z::4") + rec("ten0", "0000000016", "NM:i:0000000007", "cs:Z::4") +
        rec("noflag", "", "NM:i:0", "cs:Z::4") + rec("nopos", "0", "NM:i:0", "cs:Z::4", pos="") + rec("negpos", "0", "NM:i:0", "cs:Z::4", pos="-1") +
        rec("negnm", "0", "NM:i:-1", "cs:Z::4") + rec("emptynm", "2048", "NM:i:", "cs:Z::4") +
        "notab\n" +
        "@only\n" +
        rec("last", "0", "MD:Z:4", "cs:Z")[:-1])
assert HAND.endswith("\tcs:Z")


def plain_number(s: str):
    return int(s) if re.fullmatch("[0-9]{1,10}", s) and int(s) < 1 << 32 else None


@functools.lru_cache(maxsize=1 << 16)
def restate_line(line: str):
    """what a row says of a record line apart from where the line stands: the tuple behind begin and end.  (Kept per distinct line: a
    text of 30 000 equal lines is restated once.)"""
    fld = line.split("\t")
    ends, e = [], -1
    for f in fld:
        e += len(f) + 1
        ends.append(e)
    starts = [0] + [x + 1 for x in ends[:-1]]
    field_end = tuple(ends[k] if k < len(fld) else len(line) for k in range(11))
    bits = 0
    flag = plain_number(fld[1]) if len(fld) > 1 else None
    pos = plain_number(fld[3]) if len(fld) > 3 else None
    bits |= (1 if flag is None else 0) | (2 if pos is None else 0)
    tag_at, tag_len, nm = [0] * 4, [0] * 4, 0
    for g, prefix in enumerate(PREFIXES):
        value = characterize.sam_tag(fld, prefix)
        if value is None:
            continue
        k = max(i for i in range(11, len(fld)) if fld[i].startswith(prefix))
        assert fld[k][5:] == value
        tag_at[g], tag_len[g] = starts[k] + 5, len(value)
        bits |= 16 << g
        if g == 2:
            nm = plain_number(value)
            bits |= 4 if nm is None else 0
    return (len(fld), bits, field_end, flag or 0, pos or 0, nm or 0, tuple(tag_at), tuple(tag_len))


def restate(text: str):
    """(rows, header) of a text by the rules written out: tuples in the order of SAM_ROW_DTYPE / SAM_SPAN_DTYPE"""
    rows, header, at = [], [], 0
    lines = text.split("\n")
    if lines[-1] == "":
        lines.pop()                                         # (behind the last '\n' there is no line)
    for line in lines:
        begin, end = at, at + len(line)
        at = end + 1
        if line[:1] == "@":
            header.append((begin, end))
            continue
        n_fields, bits, field_end, flag, pos, nm, tag_at, tag_len = (restate_line if len(line) < 256 else restate_line.__wrapped__)(line)
        rows.append((begin, end, n_fields, bits, list(field_end), flag, pos, nm, list(tag_at), list(tag_len)))
    return rows, header


def restate_arrays(text):
    """restate() as the arrays the call gives: (SAM_ROW_DTYPE rows, SAM_SPAN_DTYPE header spans, the number of odd bytes).  `text`: a str of
    ASCII, or bytes, which are restated byte for byte (latin-1)"""
    raw = text.encode("ascii") if isinstance(text, str) else bytes(text)
    rows, header = restate(raw.decode("latin-1"))
    want = np.zeros(len(rows), dtype=characterize.SAM_ROW_DTYPE)
    for k, name in enumerate(characterize.SAM_ROW_DTYPE.names):
        if rows:
            want[name] = np.array([x[k] for x in rows], dtype=np.uint64)
    spans = np.zeros(len(header), dtype=characterize.SAM_SPAN_DTYPE)
    if header:
        spans["begin"], spans["end"] = np.array(header, dtype=np.uint64).T
    b = np.frombuffer(raw, dtype=np.uint8)
    return want, spans, int(np.count_nonzero((b == 13) | (b >= 128)))


def as_bytes(text) -> np.ndarray:
    return np.frombuffer(text.encode() if isinstance(text, str) else text, dtype=np.uint8)


def check_rows(eng, text: str, shifted_from=None):
    """the call's rows and header spans equal the restatement; -> the call's dict.  shifted_from = (rows, header, shift): and they are
    these, `shift` bytes further on"""
    r = characterize.sam_index_call(eng, as_bytes(text))
    rows, header = restate(text)
    got = [tuple(x[k].tolist() if x[k].ndim else int(x[k]) for k in characterize.SAM_ROW_DTYPE.names) for x in r["rows"]]
    assert len(got) == len(rows) == int(r["raw"].n_records)
    for k, (a, b) in enumerate(zip(got, rows)):
        assert a == b, (k, a, b)
    assert [tuple(x) for x in r["header"].tolist()] == header and int(r["raw"].n_header) == len(header)
    assert int(r["raw"].n_cs) == sum(1 for x in rows if x[3] & 16) and int(r["raw"].n_md) == sum(1 for x in rows if x[3] & 32)
    assert int(r["raw"].n_odd) == sum(1 for c in text.encode() if c == 13 or c >= 128)
    if shifted_from is not None:
        rows0, header0, shift = shifted_from
        moved = r["rows"][len(r["rows"]) - len(rows0):].copy()
        moved["begin"] -= shift
        moved["end"] -= shift
        assert moved.tobytes() == rows0.tobytes()
        assert (r["header"][len(r["header"]) - len(header0):]["begin"] - shift).tolist() == header0["begin"].tolist()
    return r


def check_texts(eng):
    """the three texts against the restatement; -> {name: text}"""
    chim, pairs = composed_texts()
    for text in (chim, pairs, HAND, HAND + "\n"):
        check_rows(eng, text)
    r = characterize.sam_index_call(eng, as_bytes(HAND))
    names = [HAND[b:b + fe[0]] for b, fe in zip(r["rows"]["begin"].tolist(), r["rows"]["field_end"].tolist())]
    row = dict(zip(names, r["rows"]))
    val = lambda name, g: HAND[int(row[name]["begin"]) + int(row[name]["tag_at"][g]):][:int(row[name]["tag_len"][g])]
    assert (val("twice", 0), val("twice", 1), int(row["twice"]["nm"])) == (":3*ag", "3A", 2)
    assert row["emptycs"]["bits"] & 16 and val("emptycs", 0) == "" and not row["early"]["bits"] & 16 and row["short"]["bits"] == 32
    assert [int(row[k]["bits"]) & 1 for k in ("blank", "plus", "under", "big", "max", "eleven", "ten0", "noflag")] == [1, 1, 1, 1, 0, 1, 0, 1]
    assert (int(row["max"]["flag"]), int(row["max"]["pos"]), int(row["max"]["nm"]), int(row["ten0"]["flag"]), int(row["ten0"]["nm"])) == (0xffffffff,) * 3 + (16, 7)
    assert row["negnm"]["bits"] & 4 and row["emptynm"]["bits"] & 4 and row["nopos"]["bits"] & 2 and row["negpos"]["bits"] & 2
    assert int(row[""]["n_fields"]) == 1 and int(row["notab"]["n_fields"]) == 1 and int(row["five"]["n_fields"]) == 5 and int(row["ten"]["n_fields"]) == 10
    assert int(row["adj"]["n_fields"]) == 14 and not row["last"]["bits"] & 16 and row["last"]["bits"] & 32 and int(row["last"]["end"]) == len(HAND)
    assert [HAND[b:e] for b, e in r["header"].tolist()] == ["@HD\tVN:1.6", "@SQ\tSN:chr1\tLN:1000", "@CO\ta header line in the middle", "@only"]
    return dict(chim=chim, pairs=pairs, hand=HAND)


def check_boundaries(eng, S: int):
    """sizes and separators at the borders of the scan kernels' spans"""
    chim, pairs = composed_texts()
    for text in (chim, pairs):
        r0 = characterize.sam_index_call(eng, as_bytes(text))
        for d in (-1, 0, 1):                                # the total length is S - 1, S, S + 1 beyond a multiple of S
            pad = (d - len(text)) % S + S
            front = "@CO\t" + "x" * (pad - 5) + "\n"
            assert (len(front) + len(text)) % S == d % S
            check_rows(eng, front + text, (r0["rows"], r0["header"], len(front)))
    r0 = characterize.sam_index_call(eng, as_bytes(HAND))

    def behind(front_len, text=HAND, base=r0):
        front = "@CO\t" + "x" * (front_len - 5) + "\n"
        assert len(front) == front_len
        return check_rows(eng, front + text, (base["rows"], base["header"], front_len))
    # a '\t' is the last byte of a span and a '\n' the first of the next: the line `endtab\t0\t` + '\n'
    line = "endtab\t0\t\n"
    text = line + HAND
    base = characterize.sam_index_call(eng, as_bytes(text))
    r = behind(2 * S - (len(line) - 1), text, base)
    whole = "@CO\t" + "x" * (2 * S - (len(line) - 1) - 5) + "\n" + text
    assert whole[2 * S - 1] == "\t" and whole[2 * S] == "\n" and int(r["rows"][0]["n_fields"]) == 3
    # the five prefix bytes of a tag straddle a border at each of their four cuts, for each tag
    for prefix in PREFIXES:
        line = rec("straddle", "0", "XY:Z:first", prefix + "7", "ZZ:i:1")
        text = line + HAND
        base = characterize.sam_index_call(eng, as_bytes(text))
        at = line.index(prefix)
        for cut in (1, 2, 3, 4):
            r = behind(S - at - cut, text, base)
            assert int(r["rows"][0]["bits"]) >> 4 == 1 << PREFIXES.index(prefix) and (r["rows"][0]["begin"] + r["rows"][0]["tag_at"][PREFIXES.index(prefix)] - 5) % S == S - cut
    # a line of 2 S + 3 bytes with no separator inside one whole span
    seq = "ACGT" * (S // 4)
    line = rec("long", "16", "NM:i:5", "cs:Z::%d" % len(seq), seq=seq, qual="*")
    line = line.replace(seq, seq + "A" * (2 * S + 3 - (len(line) - 1)))
    assert len(line) - 1 == 2 * S + 3
    text = line + HAND
    base = characterize.sam_index_call(eng, as_bytes(text))
    for front_len in (5, S - 40, S - 27):
        r = behind(front_len, text, base)
    whole = "@CO\t" + "x" * (S - 40 - 5) + "\n" + text
    assert "\t" not in whole[S:2 * S] and "\n" not in whole[S:2 * S]
    # the empty text, header lines only, a single byte of each kind
    for text in ("", "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:5\n", "@HD", "\n", "\t", "x", "\n\n", "\t\n\t", "@\n@"):
        check_rows(eng, text)


# ---- near misses, short records, dense separators ------------------------------------------------------------------------------------
def check_arrays(eng, text, what=""):
    """the call's rows, header spans and counts equal the restatement, compared as arrays (check_rows walks tuples: too slow for
    30 000 rows); `text`: ASCII str or bytes; -> the call's dict"""
    r = characterize.sam_index_call(eng, as_bytes(text))
    want, spans, n_odd = restate_arrays(text)
    assert (int(r["raw"].n_records), int(r["raw"].n_header)) == (len(want), len(spans)) == (len(r["rows"]), len(r["header"])), what
    if r["rows"].tobytes() != want.tobytes():
        for name in characterize.SAM_ROW_DTYPE.names:
            differ = r["rows"][name] != want[name]
            bad = np.flatnonzero(differ.reshape(len(want), -1).any(axis=1))
            assert not len(bad), (what, name, int(bad[0]), len(bad), r["rows"][name][bad[0]].tolist(), want[name][bad[0]].tolist())
        assert False, (what, "rows differ outside their fields")
    bad = np.flatnonzero((r["header"]["begin"] != spans["begin"]) | (r["header"]["end"] != spans["end"]))
    assert not len(bad), (what, "header", int(bad[0]), r["header"][bad[0]].tolist(), spans[bad[0]].tolist())
    assert int(r["raw"].n_odd) == n_odd, (what, int(r["raw"].n_odd), n_odd)
    assert (int(r["raw"].n_cs), int(r["raw"].n_md)) == (int(np.count_nonzero(want["bits"] & 16)), int(np.count_nonzero(want["bits"] & 32))), what
    return r


REAL_TAGS = ("cs:Z::4", "MD:Z:4", "NM:i:1", "SA:Z:chr1,5,+,4M,60,0;")
NEIGHBOURS = ("cm:i:", "s1:i:", "s2:i:", "ms:i:", "nn:i:", "MC:Z:", "MM:Z:", "ML:B:", "NH:i:", "XA:Z:", "CS:Z:", "cs:z:", "md:Z:", "nm:i:", "sa:Z:")


def near_prefixes():
    """five-byte field starts next to the four prefixes: one letter, the type or one colon off (the four prefixes themselves are among
    them), and the tags that stand next to them in real files"""
    grid = [c0 + c1 + s2 + c3 + s4 for c0 in "cMNSx" for c1 in "sDMAx" for c3 in "Zix" for s2, s4 in ((":", ":"), (";", ":"), (":", ";"))]
    return grid + list(NEIGHBOURS)


def near_prefix_text() -> str:
    """every candidate, with one value byte, three times: alone on an unmapped record (so that the readers go on to the end of the
    text), behind the four real tags of a mapped record, in front of them"""
    out = ["@SQ\tSN:chr1\tLN:1000\n"]
    for k, c in enumerate(near_prefixes()):
        out.append(rec("alone%d" % k, "4", c + "7", rname="*", pos="0", cigar="*"))
        out.append(rec("behind%d" % k, "0", *REAL_TAGS, c + "7"))
        out.append(rec("front%d" % k, "16", c + "7", *REAL_TAGS))
    return "".join(out)


def check_near_prefixes(eng, tmp_path):
    """a field that only looks like a tag is none: the rows equal the restatement, a near miss sets no HAS bit and moves no real tag's
    span, and the table readers do on this text what the path readers do"""
    cands, text = near_prefixes(), near_prefix_text()
    assert len(cands) == 225 + 15 and len(set(cands)) == 239          # (MM:Z: is in the grid and among the names)
    assert [c for c in cands if c in PREFIXES] == ["cs:Z:", "MD:Z:", "NM:i:", "SA:Z:"]
    r = check_arrays(eng, text, "near prefixes")
    rows = r["rows"]
    assert len(rows) == 3 * len(cands)
    begin, tag_at, tag_len = rows["begin"].tolist(), rows["tag_at"].tolist(), rows["tag_len"].tolist()
    for k, c in enumerate(cands):
        if c in PREFIXES:
            continue                                        # (a true prefix: the restatement has said what it does)
        alone, behind, front = 3 * k, 3 * k + 1, 3 * k + 2
        assert int(rows["bits"][alone]) >> 4 == 0 and tag_at[alone] == tag_len[alone] == [0] * 4 and int(rows["nm"][alone]) == 0, c
        for j in (behind, front):
            assert int(rows["bits"][j]) == 16 + 32 + 64 + 128 and int(rows["nm"][j]) == 1, (c, j)
            assert [text[begin[j] + a:begin[j] + a + n] for a, n in zip(tag_at[j], tag_len[j])] == [t[5:] for t in REAL_TAGS], (c, j)
    path = write_text(tmp_path, "near.sam", text)
    table = characterize.SamTable(path, eng)
    assert table.rows.tobytes() == rows.tobytes() and "".join(table) == text
    seen = check_same_outcome(table, path)
    assert len(seen) == len(test_sam_text.READERS) and all(v[0] == "returns" for v in seen.values()), {k: v[1:] for k, v in seen.items() if v[0] != "returns"}


def short_lines():
    """records of exactly 1 .. 5 fields: with plain FLAG and POS, with a FLAG or a POS that is not plain, of tabs only, and with FLAG
    and POS both empty"""
    whole = ["q", "16", "chr1", "7", "60"]
    out = ["\t".join(whole[:n]) for n in (1, 2, 3, 4, 5)]
    for bad in ("x", "-7", ""):
        out += ["\t".join((whole[:1] + [bad] + whole[2:])[:n]) for n in (2, 3, 4, 5)]
        out += ["\t".join((whole[:3] + [bad] + whole[4:])[:n]) for n in (4, 5)]
    return out + ["\t", "\t\t", "\t\t\t", "\t\t\t\t", "q\t\tchr1\t\t60"]


def check_short_records(eng):
    """a record whose LAST field is FLAG or POS has that number; each short line in the middle of a text, as its last line without
    '\\n', and all of them in one text"""
    lines = short_lines()
    assert {x.count("\t") + 1 for x in lines} == {1, 2, 3, 4, 5} and len(set(lines)) == len(lines)
    for line in lines:
        r = check_arrays(eng, rec("a") + line + "\n" + rec("b", "16", "NM:i:3"), repr(line))
        assert int(r["rows"][1]["n_fields"]) == line.count("\t") + 1
        r = check_arrays(eng, rec("a") + line, repr(line))
        assert int(r["rows"][1]["end"]) == len(rec("a") + line)
    check_arrays(eng, "\n".join(lines), "short lines")
    r = check_arrays(eng, "\n".join(lines) + "\n", "short lines")
    row = dict(zip(lines, r["rows"]))
    say = lambda line: (int(row[line]["bits"]), int(row[line]["flag"]), int(row[line]["pos"]))
    assert [say("\t".join(["q", "16", "chr1", "7", "60"][:n])) for n in (1, 2, 3, 4, 5)] == [(3, 0, 0), (2, 16, 0), (2, 16, 0), (0, 16, 7), (0, 16, 7)]
    assert say("q\t-7") == (3, 0, 0) and say("q\t16\tchr1\t") == (2, 16, 0) and say("q\t\tchr1\t7") == (1, 0, 7) and say("\t\t\t") == (3, 0, 0)


def dense_lengths(S: int):
    """one lane's load is 16 bytes, a wavefront's 1 KiB, the workgroup's 4 KiB, the workgroup's span S; 2 S + 1: a third span of one byte"""
    return (1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, S - 1, S, S + 1, 2 * S, 2 * S + 1)


def dense_texts(n: int) -> dict:
    cut = lambda unit: (unit * (n // len(unit) + 1))[:n]
    return dict(nl=b"\n" * n, tab=b"\t" * n, tab_nl=cut(b"\t\n"), nl_tab=cut(b"\n\t"), cr=b"\r" * n, high=b"\xff" * n, headers=cut(b"@\n"), header_x=cut(b"@\nx\n"))


def check_dense(eng, S: int):
    """texts that are nothing but separators (or odd bytes, or header lines), at the sizes where the counting and ranking of
    k_sam_sep_count / k_sam_sep_write change hands: the packed counts at their largest values"""
    for n in dense_lengths(S):
        got = {name: check_arrays(eng, text, "%s, %d bytes" % (name, n)) for name, text in dense_texts(n).items()}
        count = lambda name: (len(got[name]["rows"]), len(got[name]["header"]), int(got[name]["raw"].n_odd))
        assert count("nl") == (n, 0, 0) and count("tab") == (1, 0, 0) and count("cr") == count("high") == (1, 0, n)
        assert count("tab_nl") == ((n + 1) // 2, 0, 0) and count("nl_tab") == (n // 2 + 1, 0, 0) and count("headers") == (0, (n + 1) // 2, 0)
        assert count("header_x") == ((n + 1) // 4, (n + 3) // 4, 0)
        assert int(got["tab"]["rows"]["n_fields"][0]) == n + 1 and np.all(got["nl"]["rows"]["n_fields"] == 1)
        assert np.array_equal(got["nl"]["rows"]["begin"], np.arange(n, dtype=np.uint64))


TAG_DENSE_LINE = "\t" * 11 + "\t".join(["cs:Z:a", "NM:i:7", "MD:Z:3", "SA:Z:x", "cs:Z:b", "NM:i:x"]) + "\n"


def tag_dense_text(S: int, head: int) -> str:
    """lines of eleven empty fields and six tags, two of them given twice, past 2 S, behind a header line of `head` bytes"""
    return "@" + "x" * (head - 1) + "\n" + TAG_DENSE_LINE * (2 * S // len(TAG_DENSE_LINE) + 2)


def check_tag_dense(eng, S: int):
    """every line slides through every chunk offset: the last cs and the last NM, which is not plain, win on each"""
    assert {(head + 1 + k * len(TAG_DENSE_LINE)) % 16 for head in range(1, 17) for k in range(16)} == set(range(16))
    for head in range(1, 17):
        text = tag_dense_text(S, head)
        r = check_arrays(eng, text, "tag-dense text behind %d bytes" % head)
        rows = r["rows"]
        assert len(text) > 2 * S + 17 and len(rows) == text.count("\n") - 1 and len(r["header"]) == 1
        assert np.all(rows["bits"] == 3 + 4 + 16 + 32 + 64 + 128) and np.all(rows["n_fields"] == 17) and np.all(rows["nm"] == 0)
        at = lambda g: (rows["begin"] + rows["tag_at"][:, g]).astype(np.int64)
        b = as_bytes(text)
        assert np.all(rows["tag_len"] == 1) and bytes(b[at(0)]) == b"b" * len(rows) and bytes(b[at(2)]) == b"x" * len(rows)
        assert bytes(b[at(1)]) == b"3" * len(rows) and np.all(b[at(0) - 6] == 9) and np.all(b[at(0) - 7] == ord("x"))


def seam_positions(S: int):
    """one in front of, at and one behind where a chunk, a wavefront's load, a load of the workgroup and a span begin, in a text of 2 S + 17 bytes"""
    return sorted({c + d for c in (0, 16, 1024, 4096, 8192, 12288, S, S + 1024, S + 4096, 2 * S, 2 * S + 16) for d in (-1, 0, 1) if 0 <= c + d < 2 * S + 17})


def check_seam_pairs(eng, S: int):
    """two separators in a text of `x`, at every pair of seam positions and in every pair of kinds: where the order of the lanes and
    the order of the text disagree (a tab at byte 4096 is load 1, lane 0; one at byte 16 is load 0, lane 1); -> the number of texts"""
    P, n_texts = seam_positions(S), 0
    assert len(P) == 31
    text = bytearray(b"x" * (2 * S + 17))
    for p, q in itertools.combinations(P, 2):
        for a, b in itertools.product(b"\n\t", repeat=2):
            text[p], text[q] = a, b
            r = check_arrays(eng, bytes(text), "%r at %d, %r at %d" % (chr(a), p, chr(b), q))
            assert len(r["rows"]) == 1 + (a == 10) + (b == 10) - (q == len(text) - 1 and b == 10)
            n_texts += 1
        text[p] = text[q] = ord("x")
    return n_texts


# ---- the readers -------------------------------------------------------------------------------------------------------------------------
def same(a, b) -> bool:
    """== on what the readers return, np.array_equal (and the dtype) on the arrays in it, the types all the way down"""
    if type(a) is not type(b):
        return False
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def outcome(reader, source, names=()):
    try:
        return ("returns", reader(source))
    except Exception as e:
        text = str(e)
        for n in names:
            text = text.replace(n, "<path>")
        return ("raises", type(e), text)


def check_same_outcome(source, path, names=(), only=None):
    """every reader of test_sam_text.READERS returns or raises on `source` (a table) what it does on the file at `path`;
    -> {reader: what happened}"""
    seen = {}
    for name, reader in test_sam_text.READERS.items():
        if only and name not in only:
            continue
        want, got = outcome(reader, path, names), outcome(reader, source, names)
        assert want[0] == got[0], (name, want, got)
        if want[0] == "returns":
            assert same(want[1], got[1]), (name, path)
        else:
            assert want[1:] == got[1:], (name, want, got)
        seen[name] = want
    return seen


def write_text(tmp_path, name, text):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w", newline="") as f:
        f.write(text)
    return path


def reader_texts():
    chim, pairs = composed_texts()
    texts = {"sam_text_" + v: test_sam_text.text_of(v) for v in test_sam_text.VARIANTS}
    texts.update(chim=chim, pairs=pairs)
    return texts


def check_readers(eng, tmp_path):
    """the seven readers on a table == on the path: every input, in batches of 1 byte (every line its own batch), of one line's length
    and of the whole text; on the primary() and take() views; on a BamText"""
    seen = set()
    for name, text in reader_texts().items():
        path = write_text(tmp_path, name + ".sam", text)
        one_line = len(text.splitlines(True)[len(text.splitlines()) // 2])
        for batch in (1, one_line, len(text), characterize.SAM_BATCH_BYTES):
            if batch == 1 and len(text) > 100000:
                continue                                    # (thousands of calls: the small texts cover it)
            table = characterize.SamTable(path, eng, batch_bytes=batch)
            assert str(table) == path and len(table) == sum(1 for x in text.splitlines() if not x.startswith("@"))
            assert "".join(table) == text and table.header_lines() == [x for x in text.splitlines(True) if x.startswith("@")]
            for reader, what in check_same_outcome(table, path).items():
                seen.add((reader, what[0]))
        # the views: a reader takes a view as it takes the file write_sam writes of it
        for k, view in enumerate((table.primary(), table.take(np.arange(len(table))[::-2]), table.take([]), table.primary().take([0]) if len(table.primary()) else table.take([]))):
            out = os.path.join(str(tmp_path), "%s.view%d.sam" % (name, k))
            view.write_sam(out)
            with open(out) as f:
                assert f.read() == "".join(view)
            check_same_outcome(view, out, names=(out, path))
        flags = [int(x.split("\t")[1]) for x in text.splitlines() if not x.startswith("@") and x.count("\t")]
        assert len(table.primary()) == sum(1 for f in flags if not f & 0x904)
    assert all((r, "returns") in seen for r in test_sam_text.READERS) and sum(1 for _, w in seen if w == "raises") >= 5
    # a BamText, a TaggedText-like source
    for v in ("main", "all_ok", "chim_ok"):
        text = test_bam.encodable(test_sam_text.text_of(v))
        sam = write_text(tmp_path, v + ".enc.sam", text)
        bam = characterize.read_bam(test_bam.write_bam(tmp_path, v + ".bam", text), eng)
        table = characterize.SamTable(bam, eng, batch_bytes=200)
        assert str(table) == str(bam) and "".join(table) == text
        check_same_outcome(table, sam, names=(sam, str(bam)))


def error_texts():
    """the texts on which the path readers raise in the readers' own tests, and those next to them"""
    H, line = test_chimeric_train.HEAD, test_chimeric_train.line
    qrec = lambda name, flag, cigar, qual, *tags: "\t".join([name, str(flag), "chr", "1", "60", cigar, "*", "0", "0", "A" * (len(qual) if qual != "*" else 4), qual] + list(tags)) + "\n"
    qhead = "@HD\tVN:1.6\n@SQ\tSN:chr\tLN:1000\n"
    texts = [H + line("r1", 0, "chrA", 100, "100M"),
             H + line("r1", 0, "chrA", 100, "100M", "NM:i:1", "SA:Z:chrB,200,-,130S50M,60;"),
             H + line("r1", 0, "chrA", 100, "100M", "NM:i:1", "SA:Z:chrB,200,-,130S50M,60,2,9;"),
             H + line("r1", 0, "chrC", 100, "100M", "NM:i:1"),
             H + line("r1", 0, "chrA", 100, "100M", "NM:i:1", "SA:Z:chrC,200,-,130S50M,60,2;"),
             H + line("r1", 2048, "chrA", 100, "100M", "NM:i:1") + line("r1", 0, "chrA", 100, "100M", "NM:i:1"),
             H + line("r1", 256, "chrA", 100, "100M") + line("r1", 0, "chrA", 100, "100M", "NM:i:1"),
             H + line("u0", 4, "*", 0, "*", seq="ACGT"),
             H,
             H + line("r1", 0, "chrA", 100, "100M", "NM:i:-1"),
             test_sam_pairs.SAM_TEXT + "r8\t16\tchr1\t9\t0\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0\n",
             test_sam_pairs.SAM_TEXT + "r9\t0\tchr1\t9\t0\t2H4M\t*\t0\t0\tACGT\tIIII\tMD:Z:4\n",
             qhead + qrec("noqual", 0, "4M", "*", "cs:Z::4"),
             qhead + qrec("notag", 0, "4M", "IIII"),
             "@SQ\tSN:chrA_1\tLN:60000\n" + "ok\t0\tchrA_1\t5\t60\t10M\t*\t0\t0\t*\t*\n" + "stray\t0\tchrZ\t5\t60\t10M\t*\t0\t0\t*\t*\n",
             "@SQ\tSN:chrA_1\tLN:60000\nu1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\nsec\t256\tchrA_1\t5\t0\t4M\t*\t0\t0\t*\t*\n",
             # numbers that are not plain: int() takes some (a blank, a sign, an underscore) and refuses others, each where its reader asks
             H + line("r1", " 16", "chrA", 100, "100M", "NM:i:1", "MD:Z:100") + line("r2", "+0", "chrA", "1_0", "10M", "NM:i: 2", "cs:Z::10"),
             H + line("r1", 0, "chrA", 100, "100M", "NM:i:1", "cs:Z::100") + line("r2", "x", "chrA", 5, "10M", "NM:i:2", "cs:Z::10"),
             H + line("r1", 0, "chrA", "", "100M", "NM:i:1", "cs:Z::100") + line("r2", 0, "chrA", 5, "*", "NM:i:2"),
             H + line("r1", 4, "*", "bad", "*") + line("r2", 256, "chrA", "bad", "*") + line("r3", 0, "chrA", 7, "10M", "NM:i:0", "MD:Z:10"),
             H + line("r1", 0, "chrA", 7, "10M", "NM:i:zero", "MD:Z:10"),
             H + line("r1", 0, "chrA", 7, "10M", "NM:i:0", "MD:Z:10") + "@SQ\tSN:late\tLN:ten\n" + line("r2", 0, "chrA", "bad", "10M", "NM:i:0", "MD:Z:10"),
             H + line("r1", 0, "chrA", "bad", "10M", "NM:i:0", "MD:Z:10") + "@SQ\tSN:late\tLN:ten\n",
             H + "short\tbad\tchrA\tbad\t60\t4M\n" + "short\t4\tchrA\tbad\t60\t4M\n" + "five\tbad\tchrA\t1\t60\n",
             H + line("r1", "99999999999999999999", "chrA", "99999999999999999999", "10M", "NM:i:99999999999999999999", "MD:Z:10")]
    return texts


def check_errors(eng, tmp_path):
    """every ValueError of the path readers comes with the same message from the table readers; a FLAG of ` 16` is 16 for both; a
    text with a '\\r' or a byte that is not ASCII is turned away"""
    raised = set()
    for k, text in enumerate(error_texts()):
        path = write_text(tmp_path, "err%d.sam" % k, text)
        for batch in (1, characterize.SAM_BATCH_BYTES):
            for what in check_same_outcome(characterize.SamTable(path, eng, batch_bytes=batch), path).values():
                if what[0] == "raises":
                    assert what[1] is ValueError
                    raised.add(what[2].replace(path, "<path>"))
    for piece in ("has no NM:i tag", "six comma-separated", "chrC, which has no @SQ line", "in front of the first primary", "holds no primary alignment",
                  "negative NM", "r8 has no MD tag", "r9 has a hard clip", "noqual has no QUAL", "neither a cs nor an MD tag", "stray lies on chrZ",
                  "invalid literal for int() with base 10: 'x'", "invalid literal for int() with base 10: ''", "invalid literal for int() with base 10: 'bad'",
                  "invalid literal for int() with base 10: 'zero'", "invalid literal for int() with base 10: 'ten'"):
        assert any(piece in m for m in raised), piece
    H, line = test_chimeric_train.HEAD, test_chimeric_train.line
    path = write_text(tmp_path, "blank.sam", H + line("r1", " 16", "chrA", 100, "100M", "NM:i:1", "MD:Z:100"))
    table = characterize.SamTable(path, eng)
    assert table.rows["bits"][0] & characterize.SAM_FLAG_ODD
    assert characterize.primary_and_unaligned(table)[1] == characterize.primary_and_unaligned(path)[1] == [("r1", 16, "chrA", 100, "100M")]
    assert characterize.sam_records(table) == characterize.sam_records(path) == []          # (the text ` 16` is not `16`)
    for k, bad in enumerate((H + "r1\t0\tchrA\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\r\n", H + line("r1", 0, "chrA", 1, "4M") + line("ré", 0, "chrA", 1, "4M"))):
        path = os.path.join(str(tmp_path), "odd%d.sam" % k)
        with open(path, "wb") as f:
            f.write(bad.encode())
        with pytest.raises(ValueError, match=re.escape(path) + ":%d: a '.r' or a byte that is not ASCII" % (4 + k)):
            characterize.SamTable(path, eng)
    path = os.path.join(str(tmp_path), "packed.sam")
    with gzip.open(path, "wb") as f:
        f.write(H.encode())
    with pytest.raises(ValueError, match="gzip magic"):
        characterize.SamTable(path, eng)
    empty = characterize.SamTable(write_text(tmp_path, "empty.sam", ""), eng)
    assert len(empty) == 0 and list(empty) == [] and characterize.cs_from_sam(empty) == []


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
def test_rows_equal_the_restatement_in_any_order_of_the_tabs(host, order):
    host.order(order)
    try:
        check_texts(host)
    finally:
        host.order(0)


def test_hand_written_text_holds_every_rule():
    lines = HAND.split("\n")
    flds = [x.split("\t") for x in lines if not x.startswith("@")]
    assert lines[3].startswith("@CO") and "" in lines and not HAND.endswith("\n") and lines[-1].endswith("\tcs:Z")
    assert {5, 10, 1} <= {len(f) for f in flds} and any("\t\t" in x for x in lines)
    assert any(sum(t.startswith("cs:Z:") for t in f[11:]) == 2 for f in flds) and any("cs:Z:" in f[11:] for f in flds)
    assert {" 16", "+16", "1_6", "4294967296", ""} <= {f[1] for f in flds if len(f) > 1} and any("NM:i:-1" in f for f in flds)


def test_sizes_and_separators_at_the_borders_of_the_spans(host):
    with open(os.path.join(ROOT, "nanosim_amd", "csrc", "ns_sam_index.h")) as f:
        src = f.read()
    S = int(re.search(r"#define SAM_SPAN (\d+)u", src).group(1))
    assert S == host.span == 16384 == int(re.search(r"#define SAM_CHUNK (\d+)u", src).group(1)) * 256 * int(re.search(r"#define SAM_LOADS (\d+)u", src).group(1))
    check_boundaries(host, S)


@pytest.mark.parametrize("order", [0, 1])
def test_a_near_miss_of_a_prefix_is_no_tag_in_any_order_of_the_tabs(host, tmp_path, order):
    host.order(order)
    try:
        check_near_prefixes(host, tmp_path)
    finally:
        host.order(0)


def test_records_that_end_with_their_flag_or_their_pos(host):
    check_short_records(host)


def test_texts_of_nothing_but_separators(host):
    check_dense(host, host.span)


@pytest.mark.parametrize("order", [0, 1])
def test_tag_dense_lines_at_every_chunk_offset_in_any_order_of_the_tabs(host, order):
    host.order(order)
    try:
        check_tag_dense(host, host.span)
    finally:
        host.order(0)


def test_two_separators_at_every_pair_of_seams(host):
    assert check_seam_pairs(host, host.span) == 1860


def test_every_table_reader_equals_its_path_reader(host, tmp_path):
    check_readers(host, tmp_path)


def test_every_value_error_of_the_path_readers_and_the_texts_turned_away(host, tmp_path):
    check_errors(host, tmp_path)


def test_a_stage_that_takes_a_path_takes_a_table(host, tmp_path):
    """ir_alignments hands its paths on: the same from two tables"""
    chim, _ = composed_texts()
    path = write_text(tmp_path, "t.sam", chim)
    table = characterize.SamTable(path, host)
    assert characterize.ir_alignments(table, table) == characterize.ir_alignments(path, path) != []
    assert table.n_cs == sum(1 for x in chim.splitlines() if "\tcs:Z:" in x) and table.n_md == sum(1 for x in chim.splitlines() if "\tMD:Z:" in x)


def test_host_code_is_clean_under_the_sanitizers(tmp_path):
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "sam_index_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSAM_INDEX_MAIN", "-o", exe,
                           os.path.join(ROOT, "tests", "sam_index_host.cpp")])
    chim, pairs = composed_texts()
    rows, header = restate(HAND)
    first, _ = subprocess.check_output([exe, write_text(tmp_path, "hand.sam", HAND)], text=True).strip().split("\n")
    assert [int(v) for v in first.split()] == [len(rows), len(header), 0, sum(1 for x in rows if x[3] & 16), sum(1 for x in rows if x[3] & 32)]
    S = 16384
    edge = ["", "\n", "\t", "@", "x", "a\tcs:Z", "\t" * 11 + "cs:Z", "\t" * 11 + "cs:Z:", "\t" * 15, "\n" * 15, "q\t\r\n\xff", HAND + "\n", chim, pairs,
            "@CO\t" + "x" * (S - 6) + "\t\n" + HAND, "x" * (S - 3) + "\t" * 11 + "cs:Z", "x" * (2 * S + 3),
            near_prefix_text(), "\n".join(short_lines()), "\n".join(short_lines()) + "\n"] + [rec("a") + x for x in short_lines()] + \
           [tag_dense_text(S, head) for head in (1, 8, 16)] + [tag_dense_text(S, 5)[:-k] for k in range(1, 8)]
    for k, text in enumerate(edge):
        p = os.path.join(str(tmp_path), "t%d.sam" % k)
        with open(p, "wb") as f:
            f.write(text.encode("latin-1"))
        subprocess.check_call([exe, p], stdout=subprocess.DEVNULL)


def test_struct_layout_export_and_abi():
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "nanosim_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ns_sam_row), offsetof(ns_sam_row, begin), offsetof(ns_sam_row, end), offsetof(ns_sam_row, n_fields),
         offsetof(ns_sam_row, bits), offsetof(ns_sam_row, field_end), offsetof(ns_sam_row, flag), offsetof(ns_sam_row, pos), offsetof(ns_sam_row, nm),
         offsetof(ns_sam_row, tag_at), offsetof(ns_sam_row, tag_len));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ns_sam_index_result), offsetof(ns_sam_index_result, rows), offsetof(ns_sam_index_result, header),
         offsetof(ns_sam_index_result, n_records), offsetof(ns_sam_index_result, n_header), offsetof(ns_sam_index_result, n_odd),
         offsetof(ns_sam_index_result, n_cs), offsetof(ns_sam_index_result, n_md), offsetof(ns_sam_index_result, ms_kernel));
  printf("%zu %d %d %d %d %d %d %d\n", sizeof(ns_sam_span), NS_SAM_FLAG_ODD, NS_SAM_POS_ODD, NS_SAM_NM_ODD, NS_SAM_HAS_CS, NS_SAM_HAS_MD, NS_SAM_HAS_NM, NS_SAM_HAS_SA);
  printf("%u\n", NS_ABI_VERSION);
  return 0; }'''
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    c = os.path.join(out, "sam_index_layout.c")
    with open(c, "w") as f:
        f.write(src)
    exe = os.path.join(out, "sam_index_layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
    a, b, s, v = subprocess.check_output([exe], text=True).strip().split("\n")
    d, R = characterize.SAM_ROW_DTYPE, characterize.NsSamIndexResult
    assert d.names == ("begin", "end", "n_fields", "bits", "field_end", "flag", "pos", "nm", "tag_at", "tag_len")
    assert [int(x) for x in a.split()] == [d.itemsize] + [d.fields[k][1] for k in d.names] == [112, 0, 8, 16, 20, 24, 68, 72, 76, 80, 96]
    assert [int(x) for x in b.split()] == [C.sizeof(R)] + [getattr(R, k).offset for k, _ in R._fields_]
    assert [int(x) for x in s.split()] == [characterize.SAM_SPAN_DTYPE.itemsize, characterize.SAM_FLAG_ODD, characterize.SAM_POS_ODD, characterize.SAM_NM_ODD,
                                           characterize.SAM_HAS_CS, characterize.SAM_HAS_MD, characterize.SAM_HAS_NM, characterize.SAM_HAS_SA]
    assert "ns_sam_index" in engine.EXPORTS and int(v) == model.NS_ABI_VERSION == 7
