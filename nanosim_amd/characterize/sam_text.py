"""SAM text as the training stages read it: the one loop over the lines of a file (sam_lines), the look-up of an optional field
(sam_tag) and the cs string of a record (cs_of, get_cs).  The seven readers of the stages are filters over sam_lines.
BAM input: sam_lines takes the object characterize.read_bam returns (bam.py) wherever it takes a path."""
import re

_MD_TOKEN = re.compile(r'(\d+)|(\^[A-Za-z]+)|([A-Za-z])')
_CIGAR_TOKEN = re.compile(r'(\d+)([MIDSHX=])')          # (no N: introns are not looked for, as in the reference)


def _sam_refs(fld, refs):
    """an @SQ line's (SN, LN) behind `refs`"""
    tags = dict(t.split(":", 1) for t in fld[1:] if ":" in t)
    if "SN" in tags and "LN" in tags:
        refs.append((tags["SN"], int(tags["LN"])))


class SamSource:
    """something that is iterated like a SAM file opened for reading — its lines, each with its '\\n' — without being one: sam_lines
    takes it in the place of a path (bam.BamText is the one there is; str() of it names the file, for messages)"""


def _open_sam(path):
    """the SAM text file at `path`, opened for reading; ValueError for a gzip / BGZF file, which a BAM file is"""
    with open(path, "rb") as f:
        if f.read(2) == b"\x1f\x8b":
            raise ValueError("%s begins with the gzip magic: not SAM text.  A BAM file is read with characterize.read_bam(path, eng), "
                             "whose result every reader takes in the place of the path" % path)
    return open(path)


def sam_lines(path, min_fields: int, refs=None, header=None, drop: int = 0, lines: bool = False):
    """The records of a SAM text file, in file order, each as the list of its fields, split once (with `lines` as (the line as it
    stands, that list), for the reader that writes lines out again).  The header lines stay out of the stream: `header`, a list, takes
    them as they stand and `refs`, a list, the (SN, LN) of every @SQ line that has both.  min_fields: records with fewer fields are
    dropped (11: a whole record, 6: up to the CIGAR); drop: so are records with one of these FLAG bits.  Nothing is converted and no
    other rule applied: a reader's int() has to raise at the record the reader has come to, and a test here is paid by all seven.
    `path`: a SAM text file, or a SamSource (read_bam's BamText: the lines come from the GPU's decode of the BAM records)."""
    if isinstance(path, SamSource):
        yield from _sam_records(path, min_fields, refs, header, drop, lines)
        return
    with _open_sam(path) as f:
        yield from _sam_records(f, min_fields, refs, header, drop, lines)


def _sam_records(f, min_fields, refs, header, drop, lines):
    """sam_lines over the lines `f` gives"""
    for line in f:
        if line[0] == "@":
            if header is not None:
                header.append(line)
            if refs is not None and line.startswith("@SQ\t"):
                _sam_refs(line.rstrip("\n").split("\t"), refs)
            continue
        fld = line.rstrip("\n").split("\t")
        if len(fld) < min_fields or (drop and int(fld[1]) & drop):
            continue
        yield (line, fld) if lines else fld


def sam_tag(fld, prefix: str):
    """the text behind the optional field whose `TAG:TYPE:` is `prefix`, e.g. "MD:Z:" (of several the last); None without one"""
    value = None
    for t in fld[11:]:
        if t.startswith(prefix):
            value = t[5:]
    return value


def cs_of(fld) -> str:
    """the cs string of a record: its cs:Z tag, else from CIGAR + MD:Z (B:320-324); ValueError without either"""
    cs = sam_tag(fld, "cs:Z:")
    if cs is None:
        md = sam_tag(fld, "MD:Z:")
        if md is None:
            raise ValueError("alignment %s has neither a cs nor an MD tag" % fld[0])
        cs = get_cs(fld[5], md)
    return cs


def no_sq_line(qname: str, rname: str) -> ValueError:
    """the error for a record on a reference that the header does not name"""
    return ValueError("alignment %s lies on %s, which has no @SQ line" % (qname, rname))


def get_cs(cigar_str: str, md_str: str) -> str:
    """The cs string the reference derives for an alignment that carries only CIGAR + MD (B:76-132).  It models indels and mismatches,
    not bases: a mismatch is always `*ab`, an inserted base `I`.  Written as a walk of the MD items over a cursor into the CIGAR; the
    reference's corner behaviour is kept because its histograms depend on it: an MD item that ends exactly where an M block ends closes
    the block as a MATCH of the remaining length (so a mismatch in the last column of a block counts as `:1`, and an item that starts at
    a block end leaves a `:0`), and the items behind an insertion start with whatever is left of the MD count."""
    blocks = [(int(n), op) for n, op in _CIGAR_TOKEN.findall(cigar_str)]
    out = []
    at = 0              # cursor into `blocks`
    block_end = 0       # query-side end of the blocks consumed so far (M, I and S advance it)
    md_pos = 0          # how far the MD items have come on the same axis
    for count, deleted, base in _MD_TOKEN.findall(md_str):
        if deleted:
            out.append("-" + deleted[1:])
            at += 1                                         # the D block that carries it
            continue
        left = int(count) if count else 1
        while at < len(blocks) and blocks[at][1] != 'D':
            size, op = blocks[at]
            if op == 'I':
                out.append("+" + "I" * size)
            elif op == 'M':
                if md_pos + left < block_end + size:        # the item ends inside this block
                    if left > 0:
                        out.append("*ab" if base else ":%d" % left)
                    md_pos += left
                    break
                rest = block_end + size - md_pos            # ... or runs to its end: the rest of the block is a match
                out.append(":%d" % rest)
                md_pos += rest
                left -= rest
                block_end += size
                at += 1
                continue
            elif op != 'S':                                 # (H, X, = : the reference never advances on these; minimap2 -a writes M/I/D/S)
                raise ValueError("CIGAR operation %r is not handled by get_cs (src/besthit_to_histogram.py:100-129)" % op)
            block_end += size
            md_pos += size
            at += 1
    return "".join(out)
