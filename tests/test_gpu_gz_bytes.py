"""The compressed output on the GPU ("BGZF output"): Engine.gz_bytes — ns_gz_bytes, host bytes in and BGZF members out, on the
kernels of ns_gz_result — over the inputs of tests/test_gz_wave64.py and the sizes only the device sees: more than one block per range,
more ranges than lanes, more blocks than a workgroup of the scan holds.  Every range gunzips to its bytes and passes the BGZF walk of
characterize/bam.py; for a coded and a stored input the members are, byte for byte, those of the host wavefront program."""
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
    for k, (data, _) in enumerate(parts):
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
