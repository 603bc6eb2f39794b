"""The cs / MD walks at 64 lanes without a GPU ("cs and MD from the reference"): nanosim_amd/csrc/ns_calmd.h compiled for the
host on the lock-step wavefront of tests/wave64_host.h (tests/calmd_host.cpp with -DCALMD_HOST_LANES=64: 64 host threads, every
collective a rendezvous) behind the signature of ns_calmd.  With one lane the cross-lane arithmetic is degenerate — the mask of the
lanes below is 0, a ballot one bit, a round of the CIGAR one byte —, so the run-length bit tricks of calmd_text, the masks of the clip
order and "the lowest byte decides" of calmd_ops ran on the GPU alone, never under a sanitizer and never under the mutation audit.
Here the check_* functions of tests/test_calmd.py run on that build, and the stand-alone program of it runs as a child process under
-fsanitize=address,undefined (every record on copies of exactly its size) and under -fsanitize=thread (no two lanes store to one byte
of a text; the op table is read only behind fence(), which is the one collective of the host wave that orders memory: the same program
with a fence() that orders nothing is refused).  Nothing is loaded into Python under a sanitizer."""
import os
import re
import subprocess

import pytest

from nanosim_amd import characterize
from tests import test_calmd as T

ROOT = T.ROOT


@pytest.fixture(scope="module")
def wave():
    h = T.build_host(64)
    h.set_reference(T.REF)
    return h


def test_wave64_is_64_lanes_and_agrees_with_one_lane_on_a_record(wave):
    one = T.build_host()
    one.set_reference(T.REF)
    c = T.hand_cases()[4]
    assert T.tags(wave, [c[1:5]]) == T.tags(one, [c[1:5]]) == [(c[5], c[6])]
    assert [wave.constant(i) for i in range(4)] == [one.constant(i) for i in range(4)]


def test_wave64_hand_written_cases(wave):
    assert len(T.check_hand_cases(wave)) > 60


def test_wave64_bad_records_alone_and_among_good_ones(wave):
    T.check_bad_records(wave)


def columns(cigar: str) -> int:
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDSH=X])", cigar) if op in "M=X")


def test_wave64_a_fixed_slice_of_the_generated_records(wave):
    """every generated record below 200 columns and the first 150 above, and their = / X variants among the first 300"""
    fx = T.random_records()
    recs = fx["records"]
    short = [i for i, r in enumerate(recs) if columns(r["cigar"]) < 200]
    pick = sorted(short + [i for i, r in enumerate(recs) if columns(r["cigar"]) >= 200][:150])
    assert len(short) > 1000 and len(pick) == len(short) + 150 and max(columns(recs[i]["cigar"]) for i in pick) > 2000
    truth = [(recs[i]["md"], recs[i]["cs"]) for i in pick]
    assert [fx["writer"][i] for i in pick] == truth
    got = T.tags(wave, [(recs[i]["cigar"], recs[i]["seq"], recs[i]["chrom"], recs[i]["pos"]) for i in pick])
    for i, g, t in zip(pick, got, truth):
        assert g == t, recs[i]["name"]
    eqx = [i for i in pick if i < 300]
    assert len(eqx) > 150 and [fx["writer_eqx"][i] for i in eqx] == [(recs[i]["md"], recs[i]["cs"]) for i in eqx]
    got = T.tags(wave, [(recs[i]["cigar_eqx"], recs[i]["seq"], recs[i]["chrom"], recs[i]["pos"]) for i in eqx])
    assert got == [(recs[i]["md"], recs[i]["cs"]) for i in eqx]


def test_wave64_cross_lane_cases(wave):
    assert T.check_wave_cases(wave) > 90
    T.check_neighbours(wave)


def test_wave64_store_guard(wave):
    T.check_store_guard(wave)


def test_wave64_corrupted_records(wave):
    T.check_corrupted_records(wave, alone=10)


def program(sanitize: str, name: str):
    exe = os.path.join(ROOT, "tests", "_tmp", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-DCALMD_HOST_MAIN",
                           "-DCALMD_HOST_LANES=64", "-o", exe, os.path.join(ROOT, "tests", "calmd_host.cpp")])
    return exe


def sanitizer_records():
    """the bad records of test_calmd between two good ones, the cross-lane cases and 50 generated corrupted records.  What the programs
    print is compared with the 64-lane library, not with the Python references: these records have to stay among those that the tests
    above compare with write_tags and bad_reason on that library (bad_cases, wave_cases, corrupted_records)"""
    R = T.CHROMS[0]
    o = T.clean_window(R, 100)
    good = ("10M", R[o:o + 10].encode(), 0, o + 1)
    recs = []
    for c in T.bad_cases():
        recs += [good, (c[1], T.seq_bytes(c[2]), c[3], c[4])]
    recs += [good] + [(c[1], T.seq_bytes(c[2]), c[3], c[4]) for c in T.wave_cases()]
    recs += [(r["cigar"], r["seq"], r["chrom"], r["pos"]) for r in T.corrupted_records()["records"][:50]]
    return recs


def run_program(exe, tmp_path, records, env=None):
    genome = "".join("C %s\n" % T.REF.chrom(i).tobytes().decode("latin-1") for i in range(3))
    p = os.path.join(str(tmp_path), "records.txt")
    with open(p, "w", encoding="latin-1") as f:
        f.write(genome + "".join("R %s %s %d %d\n" % (c or "~", s.decode("latin-1") or "~", ch, ps) for c, s, ch, ps in records))
    done = subprocess.run([exe, p], capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert done.returncode == 0, done.stderr[-3000:]
    a, b = done.stdout.strip().split("\n")
    return [int(x) for x in a.split()], int(b)


def expected(wave, records):
    want = characterize.calmd_raw(wave, [r[0] for r in records], [r[1] for r in records], [r[2] for r in records], [r[3] for r in records])
    first = want["first_bad"] if want["n_bad"] else -1
    return ([len(records), want["n_bad"], first, want["bad_reason"]],
            T.checksum(want["md"], want["md_off"].tolist(), want["cs"], want["cs_off"].tolist()))


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_wave64_program_is_clean_under_the_sanitizers(wave, tmp_path, sanitize):
    """the stand-alone program of the 64-lane build, started as a child process.  address,undefined: every record on copies of exactly
    its size — CIGAR, SEQ, op table, texts, its chromosome —, so the lane behind the last byte of a CIGAR or the last column reads
    nothing.  thread: no two lanes store to one byte, no lane reads an op another lane wrote without a fence() between (the other
    collectives exchange relaxed atomics and order nothing; see the test below).  What it
    prints is what the library gives (which the tests above compare with the references)."""
    exe = program(sanitize, "calmd_host64_" + sanitize.split(",")[0])
    recs = sanitizer_records()
    assert len(recs) > 200
    assert run_program(exe, tmp_path, recs) == expected(wave, recs)
    if sanitize != "thread":
        R = T.CHROMS[0]
        o = T.clean_window(R, 100)
        good = ("10M", R[o:o + 10].encode(), 0, o + 1)
        for name, cigar, seq, chrom, pos, reason in T.bad_cases():   # each bad record as the last of its file
            got = run_program(exe, tmp_path, [good, (cigar, T.seq_bytes(seq), chrom, pos)])
            assert got == ([2, 1, 1, reason], T.checksum(b"10", [0, 2, 2], b":10", [0, 3, 3])), name


def test_wave64_thread_sanitizer_refuses_the_walk_without_its_fence(tmp_path):
    """what the clean -fsanitize=thread run above is worth: ballot, scan and bcast of tests/wave64_host.h order no memory (on the GPU
    they move registers), so the ballots between calmd_ops, which writes the op table, and calmd_text, which bisects in it, do not stand
    in for the fence() between them.  Built with a fence() that orders nothing either, the same program is refused: a data race on
    the table in calmd_text."""
    exe = os.path.join(ROOT, "tests", "_tmp", "calmd_host64_thread_nofence")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-fno-sanitize-recover=all", "-DCALMD_HOST_MAIN",
                           "-DCALMD_HOST_LANES=64", "-DWAVE64_FENCE_ORDERS_NOTHING", "-o", exe, os.path.join(ROOT, "tests", "calmd_host.cpp")])
    genome = "".join("C %s\n" % T.REF.chrom(i).tobytes().decode("latin-1") for i in range(3))
    recs = [(c[1], c[2], c[3], c[4]) for c in T.hand_cases()[:30]]
    p = os.path.join(str(tmp_path), "records.txt")
    with open(p, "w", encoding="latin-1") as f:
        f.write(genome + "".join("R %s %s %d %d\n" % r for r in recs))
    done = subprocess.run([exe, p], capture_output=True, text=True)
    assert done.returncode != 0 and "ThreadSanitizer: data race" in done.stderr and "calmd_text" in done.stderr, done.stderr[-2000:]


def test_wave64_stops_with_a_message_when_the_lanes_diverge(tmp_path):
    """the wave itself: its collectives on values that can be counted (the inclusive scan, the shuffle from a lane of one's own choice
    and the read of one lane among them: tests/chain_wave_host.hip); lanes at different kinds of collective, lanes that read different
    lanes in one readlane, and lanes that wait for one that has left, end run() with their message at once, and the wave runs the next body as if nothing had been.  Built with a time
    limit of 1 s, a lane that comes 1.5 s late finds the wave stopped by the lanes that waited for it."""
    src = os.path.join(str(tmp_path), "diverge.cpp")
    with open(src, "w") as f:
        f.write('#include "wave64_host.h"\n#include <string.h>\n'
                'static Wave64 g;\n'
                'int main() {\n'
                '    uint64_t sum[64];\n'
                '    if (!g.run([&](uint32_t l) { Wave64Lane w{&g, l}; uint64_t t; sum[l] = w.scan((uint64_t)l, t) + t + w.ballot(l == 63) + w.first(l >= 7) + w.bcast(l, 5); w.fence(); })) return 1;\n'
                '    for (uint32_t l = 0; l < 64; ++l) if (sum[l] != (uint64_t)l * (l - 1) / 2 + 2016 + (1ull << 63) + 7 + 5) return 2;\n'
                '    uint64_t big[64];\n'
                '    if (!g.run([&](uint32_t l) { Wave64Lane w{&g, l}; uint64_t t; big[l] = w.scan((uint64_t)l << 40, t) ^ t; })) return 11;\n'
                '    for (uint32_t l = 0; l < 64; ++l) if (big[l] != ((((uint64_t)l * (l - 1) / 2) << 40) ^ (2016ull << 40))) return 12;\n'
                '    if (g.run([&](uint32_t l) { Wave64Lane w{&g, l}; if (l == 9) w.fence(); else w.ballot(true); })) return 3;\n'
                '    if (!strstr(g.error().c_str(), "diverged")) return 4;\n'
                '    if (g.run([&](uint32_t l) { Wave64Lane w{&g, l}; if (l != 9) w.ballot(true); })) return 5;\n'
                '    if (!strstr(g.error().c_str(), "for lane 9, which has left the walk")) return 6;\n'
                '#if WAVE64_TIMEOUT_MS <= 1000\n'
                '    if (g.run([&](uint32_t l) { Wave64Lane w{&g, l};\n'
                '                                if (l == 9) { const auto t0 = std::chrono::steady_clock::now(); while (std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(1500)) {} }\n'
                '                                w.ballot(true); })) return 7;\n'
                '    if (!strstr(g.error().c_str(), "waited 1000 ms at ballot for lane 9")) return 8;\n'
                '#endif\n'
                '    uint32_t c[64];\n'
                '    if (!g.run([&](uint32_t l) { Wave64Lane w{&g, l}; c[l] = w.incl_scan(l + 1) + w.shfl(10 * l, 63 - l) + w.readlane(l * l, 7); w.fence(); })) return 13;\n'
                '    for (uint32_t l = 0; l < 64; ++l) if (c[l] != (l + 1) * (l + 2) / 2 + 10 * (63 - l) + 49) return 14;\n'
                '    if (g.run([&](uint32_t l) { Wave64Lane w{&g, l}; w.readlane(l, l == 9 ? 3 : 4); })) return 15;\n'
                '    if (!strstr(g.error().c_str(), "diverged") || !strstr(g.error().c_str(), "readlane of lane")) return 16;\n'
                '    if (g.run([&](uint32_t l) { Wave64Lane w{&g, l}; if (l == 9) w.shfl(l, 0); else w.readlane(l, 0); })) return 17;\n'
                '    if (!strstr(g.error().c_str(), "diverged") || !strstr(g.error().c_str(), "shfl")) return 18;\n'
                '    uint32_t n[64];\n'
                '    if (!g.run([&](uint32_t l) { Wave64Lane w{&g, l}; n[l] = w.first(l > 40); })) return 9;\n'
                '    for (uint32_t l = 0; l < 64; ++l) if (n[l] != 41) return 10;\n'
                '    return 0;\n}\n')
    for limit, messages in (("8000", 4), ("1000", 5)):
        exe = os.path.join(str(tmp_path), "diverge" + limit)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-DWAVE64_TIMEOUT_MS=" + limit, "-I", os.path.join(ROOT, "tests"), "-o", exe, src])
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr)
        assert "the lanes diverged: lane" in done.stderr and "left the walk" in done.stderr and done.stderr.count("wave64:") == messages
        assert ("waited 1000 ms" in done.stderr) == (limit == "1000")
