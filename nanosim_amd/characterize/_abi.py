"""What the stages share around a call of the library (include/nanosim_amd.h): strings packed into one buffer with offsets, arrays
of a type, a pointer that is NULL for nothing, the ValueError for bad records.  A stage's call reads pack, allocate, call, check, return."""
import numpy as np


def ptr(a):
    """the address of an array's data; None (NULL) for an empty array and for None"""
    return a.ctypes.data if a is not None and len(a) else None


def arr(values, dtype):
    """these values as a contiguous array of `dtype` (an array that is one already is not copied)"""
    return np.ascontiguousarray(values, dtype=dtype)


def check_bad(n_bad: int, first_bad: int, what: str, describe) -> None:
    """ValueError "<n_bad> <what>; the first is <describe(first_bad)>" when a call counted bad records"""
    if n_bad:
        raise ValueError("%d %s; the first is %s" % (n_bad, what, describe(int(first_bad))))


def _pack(strings):
    """(the bytes of these str / bytes one behind the other plus a NUL as a uint8 array, their len + 1 offsets as uint64)"""
    blobs = [x.encode() if isinstance(x, str) else bytes(x) for x in strings]
    off = np.zeros(len(blobs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in blobs], out=off[1:])
    return np.frombuffer(b"".join(blobs) + b"\0", dtype=np.uint8), off


class PackedPairs:
    """Aligned line pairs that are packed already (pairs_from_sam): `ref`, `qry`, `off` as _pack_pairs returns them (a NUL byte behind
    the lines), `aln` = the ns_sam_aln figures (SAM_ALN_DTYPE) and the records they come from.  _pack_pairs, count_maf and
    count_homopolymers take it as it is; indexing or iterating gives maf_records' tuples (rname, pos - 1, reference line, query line)."""

    def __init__(self, ref, qry, off, aln, sam_recs):
        self.ref, self.qry, self.off, self.aln, self.sam_recs = ref, qry, off, aln, sam_recs

    def __len__(self):
        return len(self.off) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        lo, hi = int(self.off[i]), int(self.off[i + 1])
        return (self.sam_recs[i][2], self.sam_recs[i][3] - 1, self.ref[lo:hi].tobytes().decode(), self.qry[lo:hi].tobytes().decode())

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def heads(self):
        """[(rname, pos - 1)]: what <prefix>_hp_lengths.tsv needs of every alignment, without its lines"""
        return [(r[2], r[3] - 1) for r in self.sam_recs]


def _pack_pairs(ref_lines, query_lines=None):
    """_pack of the two lines of every alignment: (reference bytes, query bytes, the offsets of both); a PackedPairs as it is"""
    if isinstance(ref_lines, PackedPairs):
        return ref_lines.ref, ref_lines.qry, ref_lines.off
    ref, off = _pack(ref_lines)
    qry, q_off = _pack(query_lines)
    if not np.array_equal(off, q_off):
        raise ValueError("the two lines of an alignment differ in length")
    return ref, qry, off


def write_text(path: str, text: str) -> None:
    with open(path, "w") as f:
        f.write(text)
