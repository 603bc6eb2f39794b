"""LAST's MAF as alignment input (``besthit_and_unaligned`` of src/get_besthit_maf.py, G:8-56; ``-a LAST`` / ``-ga x.maf``) is the tenth
piece: of the alignments of every read the one with the largest size, the first of several, written to ``<prefix>_besthit.maf``, which
the MAF branches above read.  The `s` lines are found, parsed and chosen on the GPU from the bytes of the file (``ns_maf_besthit``,
csrc/ns_maf_best.h); this module walks the reads file and writes the files:

    unaligned_len, strandness = characterize.besthit_and_unaligned("training", "last.maf", "reads.fasta", eng)
    characterize.train_genome_from_maf("training", "last.maf", "reads.fasta", eng)      # what `read_analysis.py genome -ga last.maf` leaves

Deviations: a line whose start, size or srcSize is not made of decimal digits below 2^32 raises ValueError (Python's int() takes more);
a file without any alignment raises ValueError (the reference divides by zero); the reads file is FASTA."""
import ctypes as C
import gzip
import os

import numpy as np

from ._abi import _pack, arr, ptr
from .errors import hist
from .homopolymers import homopolymer_lengths
from .lengths import maf_figures, read_lengths_from_maf
from .mixfit import model_fitting


class NsMafBestResult(C.Structure):
    """mirror of ns_maf_best_result (include/nanosim_amd.h)"""
    _fields_ = [("found", C.c_void_p), ("lines", C.c_void_p), ("records", C.c_void_p), ("figures", C.c_void_p), ("n_lines", C.c_uint64),
                ("n_pairs", C.c_uint64), ("n_kept", C.c_uint64), ("pos_strand", C.c_uint64), ("first_bad_line", C.c_uint64),
                ("first_bad_offset", C.c_uint64), ("ms_kernel", C.c_double)]


MAF_LINES_DTYPE = np.dtype([("ref_begin", "<u8"), ("ref_end", "<u8"), ("qry_begin", "<u8"), ("qry_end", "<u8")])                # ns_maf_best_lines
MAF_RECORD_DTYPE = np.dtype([("ref_name_at", "<u8"), ("ref_seq_at", "<u8"), ("qry_seq_at", "<u8"), ("ref_name_len", "<u4"), ("ref_seq_len", "<u4"),
                             ("qry_seq_len", "<u4"), ("ref_start", "<u4")])                                                   # ns_maf_best_record
MAF_FIGURES_DTYPE = np.dtype([("aligned_ref", "<u4"), ("ref_total", "<u4"), ("head", "<u4"), ("total", "<u4"), ("ht", "<i8")])  # ns_maf_best_figures


def _file_bytes(path: str) -> np.ndarray:
    """the bytes of a file as a uint8 array (mapped, not read; `.gz` as file_handler.gzopen: unpacked)"""
    if path.lower().endswith(".gz"):
        with gzip.open(path, "rb") as f:
            return np.frombuffer(f.read(), dtype=np.uint8)
    if os.path.getsize(path) == 0:
        return np.zeros(0, dtype=np.uint8)
    return np.memmap(path, dtype=np.uint8, mode="r")


def _line_number(text: np.ndarray, offset: int) -> int:
    """the 1-based line of the file in which byte `offset` stands"""
    return int(np.count_nonzero(text[:offset] == 10)) + 1


def _last_s_line(text: np.ndarray) -> int:
    """the offset of the last `s` line of the text (-1: none), looked for from the end in pieces"""
    n, step = len(text), 1 << 20
    hi = n
    while hi > 0:
        lo = max(0, hi - step)
        buf = text[lo:min(n, hi + 2)].tobytes()                    # (two bytes more: a start whose '\n' is the piece's last byte)
        at = max(buf.rfind(b"\ns "), buf.rfind(b"\ns\t"))
        if at >= 0:
            return lo + at + 1
        hi = lo
    return 0 if n >= 2 and text[:2].tobytes() in (b"s ", b"s\t") else -1


def besthit_call(eng, text, names=None) -> dict:
    """ns_maf_besthit on the bytes of a MAF file (a uint8 array) and, optionally, the names of a reads file (a list of bytes): the
    NsMafBestResult as `raw`, `lines` / `records` / `figure_rows` (copies of the per-kept-pair arrays, MAF_*_DTYPE) and `found` (a bool
    per name, None without names).  Raises nothing for a bad line (raw.first_bad_line < raw.n_lines) or an odd number of `s` lines
    (raw.n_lines & 1): the caller knows the file."""
    text = arr(text, np.uint8)
    out = NsMafBestResult()
    n_names = 0 if names is None else len(names)
    nm = nm_off = found = None
    if names is not None:
        found = np.zeros(n_names, dtype=np.uint8)
    if n_names:
        nm, nm_off = _pack(names)
        out.found = found.ctypes.data
    rc = eng.L.ns_maf_besthit(eng.ctx, ptr(text), len(text), ptr(nm), ptr(nm_off), n_names, C.addressof(out))
    if not (int(out.n_lines) & 1):
        eng._check(rc)
    k = int(out.n_kept)

    def rows(address, dtype):
        if not k:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer(C.string_at(address, k * dtype.itemsize), dtype=dtype).copy()       # (the library's arrays live until its next call)
    return dict(raw=out, lines=rows(out.lines, MAF_LINES_DTYPE), records=rows(out.records, MAF_RECORD_DTYPE),
                figure_rows=rows(out.figures, MAF_FIGURES_DTYPE), found=None if names is None else found.astype(bool))


def figures_from_rows(rows, mode: str = "genome") -> dict:
    """length_figures_maf's dict from the figure rows of besthit_call (A:91-110)"""
    return maf_figures(rows["aligned_ref"], rows["ref_total"], rows["head"], rows["total"], rows["ht"], mode)


def fasta_lines(path: str):
    """the reads file as G:43-52 walks it, FASTA (possibly `.gz`): (names: the first word of every `>` header without the `>`, as bytes;
    owner: per sequence line the index of its header; length: len(line.strip()) of it — a blank line is a 0).  ValueError for a header
    without a name and a sequence line in front of the first header."""
    names, owner, length = [], [], []
    with (gzip.open(path, "rb") if path.lower().endswith(".gz") else open(path, "rb")) as f:
        for no, line in enumerate(f, 1):
            if line[:1] == b">":
                word = line.strip().split()[0][1:]
                if not word:
                    raise ValueError("%s:%d: a `>` header without a name" % (path, no))
                names.append(word)
            elif not names:
                raise ValueError("%s:%d: a sequence line in front of the first header (the reference stops with a NameError)" % (path, no))
            else:
                owner.append(len(names) - 1)
                length.append(len(line.strip()))
    return names, np.array(owner, dtype=np.int64), np.array(length, dtype=np.int64)


def besthit(eng, maf_path: str, reads_path=None, mode: str = "genome") -> dict:
    """besthit_and_unaligned (G:8-56) without its file: of the pairs of `s` lines of every query name of a LAST MAF file — as it is, or
    what `grep '^s '` left of it — the one with the largest size, of several the first, chosen on the GPU from the file's bytes
    (ns_maf_besthit).  -> `lines` (MAF_LINES_DTYPE: the byte ranges of the two lines of every kept pair, in file order), `num_aligned`,
    `pos_strand`, `strandness` (float(pos_strand) / num_aligned, G:41), `figures` (length_figures_maf's dict for the kept pairs; `mode`
    as there), `figure_rows`, `records` (maf_records' list for them), `unaligned_length` (int64: len(line.strip()) of every sequence line
    of every read of `reads_path` whose name is no query name, G:43-52; None without a reads file) and `ms_kernel`.
    The reads file is FASTA (`.gz` too, as file_handler.gzopen); the reference reads FASTQ with the same loop and counts its `+` and
    quality lines as sequence: not restated, give FASTA.
    ValueError with the file and the line: an odd number of `s` lines, a line whose start, size or srcSize is not made of digits that fit
    32 bits or that has fewer than 7 fields, a reference sequence longer than the query's (maf_records), a file without any alignment
    (the reference divides by zero), and fasta_lines' two."""
    names = owner = length = None
    if reads_path is not None:
        names, owner, length = fasta_lines(reads_path)
    text = _file_bytes(maf_path)
    r = besthit_call(eng, text, names)
    raw = r["raw"]
    if int(raw.n_lines) & 1:
        raise ValueError("%s:%d: an `s` line without its partner (odd number of `s` lines)" % (maf_path, _line_number(text, max(_last_s_line(text), 0))))
    if raw.first_bad_line < raw.n_lines:
        raise ValueError("%s:%d: not an `s` line of LAST: start, size and srcSize have to be decimal digits below 2^32, in 7 fields or more"
                         % (maf_path, _line_number(text, int(raw.first_bad_offset))))
    if not raw.n_kept:
        raise ValueError("%s: no alignment at all (the reference divides by zero, G:41)" % maf_path)
    recs = []
    for rec in r["records"].tolist():
        name_at, rs, qs, name_len, rl, ql, start = rec
        if rl > ql:
            raise ValueError("%s:%d: not two `s` lines with an aligned sequence each (the reference sequence is the longer one)"
                             % (maf_path, _line_number(text, rs)))
        recs.append((text[name_at:name_at + name_len].tobytes().decode(), start, text[rs:rs + rl].tobytes().decode(), text[qs:qs + rl].tobytes().decode()))
    num_aligned, pos_strand = int(raw.n_kept), int(raw.pos_strand)
    return dict(lines=r["lines"], num_aligned=num_aligned, pos_strand=pos_strand, strandness=float(pos_strand) / num_aligned,
                figures=figures_from_rows(r["figure_rows"], mode), figure_rows=r["figure_rows"], records=recs,
                unaligned_length=None if names is None else length[~r["found"][owner]],
                ms_kernel=float(raw.ms_kernel))


def write_besthit(prefix: str, maf_path: str, result: dict) -> None:
    """<prefix>_besthit.maf as G:35 writes it: the two lines of every kept pair as they stand in the file, in file order (a last line
    without '\\n' stays without)"""
    text = _file_bytes(maf_path)
    with open(prefix + "_besthit.maf", "wb") as f:
        for rb, re_, qb, qe in result["lines"].tolist():
            f.write(text[rb:re_].tobytes())
            f.write(text[qb:qe].tobytes())


def besthit_and_unaligned(prefix: str, maf_path: str, reads_path: str, eng):
    """besthit_and_unaligned(infile, outmaf, prefix) of G:8: writes <prefix>_besthit.maf, -> (unaligned_length, strandness)"""
    r = besthit(eng, maf_path, reads_path)
    write_besthit(prefix, maf_path, r)
    return r["unaligned_length"], r["strandness"]


def train_genome_from_maf(prefix: str, maf_path: str, reads_path: str, eng, model_fit: bool = True, homopolymer: bool = False, min_hp_len: int = 5,
                          pickles=None) -> dict:
    """what `read_analysis.py genome -ga x.maf` runs behind the alignment (R:185-190, 605-611, 858-875): the best hit per read and
    <prefix>_besthit.maf, hist(prefix, "maf") from the kept pairs as they came from the GPU (the file is not read back), the read-length
    files, model_fitting unless model_fit is False (--no_model_fit) and, with `homopolymer`, the homopolymer-length model.  The prefix
    then opens with model.load_model(prefix) (with model_fit=False it needs a <prefix>_model_profile from elsewhere).  -> besthit's dict"""
    r = besthit(eng, maf_path, reads_path)
    write_besthit(prefix, maf_path, r)
    hist(prefix, [(ref, qry) for _, _, ref, qry in r["records"]], eng, "maf")
    read_lengths_from_maf(prefix, r["figures"], r["unaligned_length"], r["strandness"], pickles)
    if model_fit:
        model_fitting(prefix, eng)
    if homopolymer:
        homopolymer_lengths(prefix, r["records"], eng, min_hp_len)
    return r
