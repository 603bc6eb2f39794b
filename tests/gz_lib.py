"""What the tests of the compressed output share (tests/test_gz_wave64.py, tests/test_gpu_gz_bytes.py): the inputs the issue of the
feature names, the host wavefront program of tests/gz_wave_host.cpp, and the two readers every member has to satisfy — Python's gzip and
the project's own BGZF walk (nanosim_amd/characterize/bam.py: BC/BSIZE, CRC32, ISIZE)."""
import gzip
import os
import subprocess

import numpy as np

from nanosim_amd import engine
from nanosim_amd.characterize import bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = engine.NS_GZ_BLOCK_BYTES
S = B // 64
LENGTHS = [1, 3, 4, S - 1, S, S + 1, 63 * S + 1, B - 1, B]
STARTS = [0, 1, 15]
KINDS = ["acgt", "one", "random", "lacking", "fib"]
MUST_BE_STORED = {"random", "lacking"}


def fib_counts():
    h = np.zeros(256, dtype=np.uint64)
    a, b = 1, 1
    for v in range(40):
        h[100 + v] = a
        a, b = b, a + b
    return h


def counts_of(data: bytes) -> np.ndarray:
    return np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256).astype(np.uint64)


def make_input(kind: str, n: int, seed: int = 1):
    """(the bytes, the counts the code is built from)"""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    if kind == "acgt":
        a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)
        a[79::80] = 10
        return a.tobytes(), counts_of(a.tobytes())
    if kind == "one":
        return b"A" * n, counts_of(b"A" * n)
    if kind == "random":
        a = rng.integers(0, 256, n, dtype=np.uint8)
        if n >= B:                                      # every value at least once: the code lacks none, the block is stored for its size
            a[:256] = np.arange(256, dtype=np.uint8)
        return a.tobytes(), counts_of(a.tobytes())
    if kind == "lacking":                               # one byte in the middle that the code has no code for
        a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)
        a[n // 2] = ord("N")
        h = counts_of(a.tobytes())
        h[ord("N")] = 0
        return a.tobytes(), h
    if kind == "fib":
        h = fib_counts()
        p = h[100:140].astype(np.float64)
        a = rng.choice(np.arange(100, 140, dtype=np.uint8), n, p=p / p.sum())
        return a.tobytes(), h
    raise ValueError(kind)


def check_members(members: bytes, data: bytes, tmp_dir: str, name: str = "m.gz"):
    """gzip gives the input back, and the BGZF walk accepts every member: BSIZE, CRC32, ISIZE <= B, member <= 65536.  Returns the
    (offset, stored) of the members."""
    assert gzip.decompress(members) == data
    path = os.path.join(tmp_dir, name)
    with open(path, "wb") as f:
        f.write(members + bam.BGZF_EOF)
    blocks = list(bam.bgzf_blocks(path))
    raw, out, at_expected = [], [], 0
    for k, blk in enumerate(blocks):
        deflate, crc, isize, at = blk
        assert at == at_expected
        assert 0 < isize <= B
        total = 18 + len(deflate) + 8
        assert total <= 65536
        at_expected += total
        raw.append(bam._inflate(path, blk))
        out.append((at, deflate[0] == 1))
        if k + 1 < len(blocks):
            assert isize == B                          # only the last block of a range is short
    assert at_expected == len(members)
    assert b"".join(raw) == data
    assert len(blocks) == (len(data) + B - 1) // B
    return out


def build_program(sanitize: str | None = None) -> str:
    exe = os.path.join(ROOT, "tests", "_tmp", "gz_wave_host" + ("_" + sanitize.split(",")[0] if sanitize else ""))
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "gz_wave_host.cpp")])
    return exe


def run_program(exe: str, tmp_dir: str, jobs):
    """jobs: (data, counts, start) each.  Returns per job (the members, [(input bytes, member bytes, stored) per block])"""
    lines = []
    for k, (data, counts, start) in enumerate(jobs):
        pi, pc, po = (os.path.join(tmp_dir, "%s%d.bin" % (x, k)) for x in ("in", "counts", "out"))
        with open(pi, "wb") as f:
            f.write(data)
        with open(pc, "wb") as f:
            f.write(np.ascontiguousarray(counts, dtype="<u8").tobytes())
        lines.append("%s %s %d %s\n" % (pi, pc, start, po))
    pj = os.path.join(tmp_dir, "jobs.txt")
    with open(pj, "w") as f:
        f.writelines(lines)
    done = subprocess.run([exe, pj], capture_output=True, text=True)
    assert done.returncode == 0, (done.stdout[-2000:], done.stderr[-4000:])
    blocks = [[] for _ in jobs]
    for ln in done.stdout.splitlines():
        k, n, m, stored = (int(x) for x in ln.split())
        blocks[k].append((n, m, bool(stored)))
    out = []
    for k in range(len(jobs)):
        with open(os.path.join(tmp_dir, "out%d.bin" % k), "rb") as f:
            out.append((f.read(), blocks[k]))
    return out
