"""The compressed output on the GPU ("BGZF output"): Engine.gz_bytes — ns_gz_bytes, host bytes in and BGZF members out, on the
kernels of ns_gz_result — over the inputs of tests/test_gz_wave64.py and the sizes only the device sees: more than one block per range,
more ranges than lanes, more blocks than a workgroup of the scan holds.  Every range gunzips to its bytes and passes the BGZF walk of
characterize/bam.py; for a coded and a stored input the members are, byte for byte, those of the host wavefront program.

Readers forgive, so every range is also held, byte for byte, against gz_lib.ref_members, the plain encoder: the inputs above, a sweep of
sizes around every lane boundary as ranges of one buffer (members begin at every alignment) under a code of 256 values, one of 60 and a
hand-made one with a header of 1 879 bits; and the code the device counts itself (k_gz_hist) against the code of numpy's counts."""
import gzip

import numpy as np
import pytest

from nanosim_amd import engine as E
from tests import gz_lib as G

pytestmark = pytest.mark.gpu
B = G.B
LENGTHS = G.LENGTHS + [B + 1, 2 * B, 2 * B + 1]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("kind", G.KINDS)
def test_every_input_gunzips_and_passes_the_bgzf_walk(eng, kind, tmp_path):
    """all lengths of a kind in ONE call, one range each, so the ranges begin at every alignment of the input"""
    parts = [G.make_input(kind, n) for n in LENGTHS]
    for (data, counts), n in zip(parts, LENGTHS):
        code = E.build_gz_code(counts)
        members, off = eng.gz_bytes(data, code=code)
        assert off.tolist() == [0, len(members)] and len(members) <= eng.L.ns_gz_bound(n, 1)
        assert members == G.ref_members(G.plain_code(code), data), n
        walked = G.check_members(members, data, str(tmp_path))
        if kind in G.MUST_BE_STORED:
            assert walked[(n // 2) // B][1], n                      # the block with the byte the code lacks / every random block
            if kind == "random":
                assert all(s for _, s in walked), n
        else:                                                       # (a block of a byte or four is stored: the header alone is longer)
            assert not any(s for k, (_, s) in enumerate(walked) if min(B, n - k * B) >= G.S - 1), n
    # ... and as ranges of one buffer, with the code counted on the device (code=None)
    blob = b"".join(d for d, _ in parts)
    cuts = np.cumsum([0] + [len(d) for d, _ in parts])
    members, off = eng.gz_bytes(blob, cuts=cuts)
    assert off[0] == 0 and (np.diff(off.astype(np.int64)) > 0).all() and off[-1] == len(members) <= eng.L.ns_gz_bound(len(blob), len(parts))
    counted = G.plain_code(E.build_gz_code(G.counts_of(blob)))
    for k, (data, _) in enumerate(parts):
        assert members[int(off[k]):int(off[k + 1])] == G.ref_members(counted, data), LENGTHS[k]
        G.check_members(members[int(off[k]):int(off[k + 1])], data, str(tmp_path))


def test_more_ranges_than_lanes_and_an_empty_one(eng, tmp_path):
    data, counts = G.make_input("acgt", 70)
    cuts = list(range(0, 30)) + [29] + list(range(30, 71))          # 70 ranges of one byte, an empty one among them
    members, off = eng.gz_bytes(data, cuts=cuts, code=E.build_gz_code(counts))
    d = np.diff(off.astype(np.int64))
    assert len(off) == 72 and (d >= 0).all() and d[29] == 0 and (np.delete(d, 29) > 0).all() and off[-1] == len(members)
    for k in range(71):
        lo, hi = cuts[k], cuts[k + 1]
        if hi > lo:
            G.check_members(members[int(off[k]):int(off[k + 1])], data[lo:hi], str(tmp_path))
    assert len(members) <= eng.L.ns_gz_bound(70, 71)


def test_300_blocks_two_runs_and_a_small_destination(eng, tmp_path):
    data, counts = G.make_input("acgt", 299 * B + 1234)
    code = E.build_gz_code(counts)
    members, off = eng.gz_bytes(data, code=code)
    walked = G.check_members(members, data, str(tmp_path))
    assert len(walked) == 300 and not any(s for _, s in walked)
    assert len(members) <= eng.L.ns_gz_bound(len(data), 1)
    again, off2 = eng.gz_bytes(data, code=code)
    assert again == members and off2.tolist() == off.tolist()
    # a destination one byte short: NS_EINVAL, nothing written out of bounds, and the size needed comes back
    with pytest.raises(E.EngineError) as err:
        eng.gz_bytes(data, code=code, cap=len(members) - 1)
    assert err.value.code == E.NS_EINVAL
    ok, _ = eng.gz_bytes(data, code=code, cap=len(members))
    assert ok == members


def test_bad_arguments_are_refused(eng):
    data, counts = G.make_input("acgt", 100)
    for cuts in ([0, 101], [50, 20], []):
        with pytest.raises(E.EngineError) as err:
            eng.gz_bytes(data, cuts=cuts)
        assert err.value.code == E.NS_EINVAL
    bad = E.build_gz_code(counts)
    bad.len[65] = 16
    with pytest.raises(E.EngineError) as err:
        eng.gz_bytes(data, code=bad)
    assert err.value.code == E.NS_EINVAL
    assert eng.gz_bytes(b"")[0] == b""


@pytest.mark.parametrize("kind", ["acgt", "random"])
def test_members_equal_the_host_wavefront_programs(eng, kind, tmp_path):
    """one coded and one stored input of two blocks and a short one: the device's bytes are the 64-lane host walk's for the same code"""
    data, counts = G.make_input(kind, 2 * B + 77)
    (host, blocks), = G.run_program(G.build_program(), str(tmp_path), [(data, counts, 0)])
    assert [s for _, _, s in blocks] == [kind == "random"] * 3
    members, _ = eng.gz_bytes(data, code=E.build_gz_code(counts))
    assert members == host


def irregular_code(n_values, seed):
    """(the values, their weights, a code of counts exp(U(0, 9)) over them)"""
    rng = np.random.default_rng([seed, n_values])
    values = rng.choice(256, n_values, replace=False)
    weights = np.exp(rng.uniform(0, 9, n_values))
    counts = np.zeros(256, dtype=np.uint64)
    counts[values] = weights.astype(np.uint64)
    return values, weights / weights.sum(), E.build_gz_code(counts)


@pytest.mark.parametrize("which", ["256_values", "60_values", "long_header"])
def test_sweep_as_ranges_of_one_buffer_equals_the_plain_encoder(eng, which):
    """the sizes of the host sweep (tests/test_gz_wave64.py) as the ranges of ONE buffer in one call, in an order that puts the ranges and
    their members at every alignment; every range is, byte for byte, what the plain encoder makes of it under the call's code"""
    rng = np.random.default_rng([5, len(which)])
    if which == "long_header":
        code = G.long_header_code()
        parts = [np.where(rng.random(n) < 0.9, 0, rng.integers(0, 256, n)).astype(np.uint8).tobytes() for n in G.SWEEP_SIZES]
        handed = code.struct()
    else:
        values, p, handed = irregular_code(int(which.split("_")[0]), 11)
        code = G.plain_code(handed)
        parts = [rng.choice(values, n, p=p).astype(np.uint8).tobytes() for n in G.SWEEP_SIZES]
    parts = [parts[i] for i in rng.permutation(len(parts))]
    cuts = np.cumsum([0] + [len(d) for d in parts])
    members, off = eng.gz_bytes(b"".join(parts), cuts=cuts, code=handed)
    assert off[0] == 0 and off[-1] == len(members)
    want = [G.ref_members(code, d) for d in parts]
    at = np.cumsum([0] + [len(w) for w in want])
    assert off.tolist() == at.tolist()
    for k, w in enumerate(want):
        assert members[int(off[k]):int(off[k + 1])] == w, (k, len(parts[k]))
    stored = [G.ref_is_stored(w) for w in want]
    assert any(stored) and not all(stored)
    for flag in (True, False):                              # coded and stored members and their inputs begin at every alignment
        assert {int(a) % 4 for a, s in zip(at[:-1], stored) if s == flag} == {0, 1, 2, 3}
        assert {int(c) % 4 for c, s in zip(cuts[:-1], stored) if s == flag} == {0, 1, 2, 3}


def lane_blob(n, seed=3):
    """n bytes whose four byte lanes carry different values: byte i is one of 12 values of its own for i mod 4, skewed so that they deflate"""
    rng = np.random.default_rng([seed, n])
    a = 60 * (np.arange(n) % 4) + np.minimum(rng.geometric(0.4, n) - 1, 11)
    return a.astype(np.uint8)


COUNTED_SIZES = [1, 2, 3, 5, 6, 7] + [4 * 4096 * k + d for k in (1, 2) for d in range(4)]


@pytest.mark.parametrize("n", COUNTED_SIZES)
def test_the_code_the_device_counts_is_the_code_of_the_counts(eng, n):
    """code=None: k_gz_hist counts the buffer.  Sizes with 1 to 3 bytes behind the last whole word, the first size with two workgroups
    (4 * 4096 + 1 words need one more) and the first at which a workgroup strides.  A block of a few bytes is stored under any code, so
    from 4 * 4096 on the bytes behind the last word are values that stand nowhere else: a count that drops them gives another header"""
    a = lane_blob(n)
    if n > 8:
        a[n - (n % 4):] = [250, 251, 252][:n % 4]
    blob = a.tobytes()
    code = E.build_gz_code(G.counts_of(blob))
    counted, off = eng.gz_bytes(blob)
    given, off2 = eng.gz_bytes(blob, code=code)
    assert counted == given and off.tolist() == off2.tolist()
    want = G.ref_members(G.plain_code(code), blob)
    assert counted == want
    assert G.ref_is_stored(want) == (n < 8)                 # (from 4 * 4096 on the first block is coded: its header names every value)


def test_the_device_counts_the_whole_buffer_not_the_ranges(eng):
    """cuts[0] > 0 and cuts[-1] < n: the code is still that of all n bytes (include/nanosim_amd.h), whose header names values that stand
    only in front of and behind the ranges"""
    n = 4 * 4096 + 2
    a = lane_blob(n)
    a[:5] = [240, 241, 242, 243, 244]
    a[n - 7:] = [245, 246, 247, 248, 249, 250, 251]
    blob, cuts = a.tobytes(), [5, 1001, n - 7]
    whole, inner = E.build_gz_code(G.counts_of(blob)), E.build_gz_code(G.counts_of(blob[5:n - 7]))
    assert bytes(whole.header) != bytes(inner.header)
    counted, off = eng.gz_bytes(blob, cuts=cuts)
    given, off2 = eng.gz_bytes(blob, cuts=cuts, code=whole)
    assert counted == given and off.tolist() == off2.tolist()
    assert counted == G.ref_members(G.plain_code(whole), blob[5:1001]) + G.ref_members(G.plain_code(whole), blob[1001:n - 7])


def test_the_count_of_16_mib_and_3_bytes(eng):
    """16 MiB + 3 bytes: 1 024 workgroups of k_gz_hist, the most a call starts, each at its last stride, and 3 bytes behind the last word.
    The bytes under the counted code against the bytes under the code of numpy's counts, and gunzip; no walk over the 1 025 blocks.
    Measured on an MI355X: 0.44 s for the whole test, making and gunzipping the 16 MiB on the host included."""
    n = (16 << 20) + 3
    a = lane_blob(n)
    a[n - 3:] = [250, 251, 252]
    blob = a.tobytes()
    counted, off = eng.gz_bytes(blob)
    given, _ = eng.gz_bytes(blob, code=E.build_gz_code(G.counts_of(blob)))
    assert counted == given and off.tolist() == [0, len(counted)]
    assert gzip.decompress(counted) == blob
    assert len(counted) < n                                 # (stored members would be longer than their input)
