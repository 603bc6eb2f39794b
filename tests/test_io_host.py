"""The host threads of the output pipeline (nanosim_amd/csrc/ns_io.h: one copier, up to 16 writers and the caller around one mutex)
on CPU: tests/io_host.cpp drives the engine's own code — ns_io.h compiled unchanged against the asynchronous runtime stub of
tests/hip_host_stub — through seven scenarios (and an eighth that checks the stub's own strictness), as a stand-alone program built three ways: plain, under ThreadSanitizer, and under
AddressSanitizer + UndefinedBehaviorSanitizer.  Every scenario runs on every build as a child process; it must exit 0 and leave no
sanitizer report.  What the scenarios pin, and which break of ns_io.h each one catches: DESIGN.md §8, "The host threads under sanitizers".

A build whose sanitizer runtime does not link or start where the tests run is skipped, with a reason that names it; the plain build
never is.

The time limit is a deadlock detector, not a measurement.  Seconds per scenario on 8 cores (the slowest of three runs):

    scenario            -O2    -fsanitize=thread   -fsanitize=address,undefined
    roundtrip           0.71         1.25                 0.82
    slot_reuse          1.03         1.52                 1.07
    no_file             0.02         0.05                 0.03
    failed_writes       0.12         0.19                 0.13
    copy_failures       0.06         0.07                 0.07
    startup_failures    0.02         0.03                 0.03
    churn               1.69         3.33                 1.92
    stub_strict         0.02         0.03                 0.03

and about 20 s to compile the three programs side by side.  LIMIT_S is 36 times the slowest of them (churn under ThreadSanitizer: 3.3 s,
4.0 s while other work kept all cores busy); a child that is still running then has a thread that waits for something that does not come,
and says so itself (its watchdog, exit status 3) just before the limit of the test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "_tmp")
SCENARIOS = ["roundtrip", "slot_reuse", "no_file", "failed_writes", "copy_failures", "startup_failures", "churn", "stub_strict"]
LIMIT_S = 120
# flags of a build: the candidates in order of preference — the sanitizer's runtime linked statically first (such a program starts
# whatever else the environment loads in front of it)
BUILDS = {
    "plain": [["-O2"]],
    "tsan": [["-O1", "-g", "-fsanitize=thread", "-static-libtsan"], ["-O1", "-g", "-fsanitize=thread"]],
    "asan_ubsan": [["-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"], ["-O1", "-g", "-fsanitize=address,undefined"]],
}
CHILD_ENV = {
    "TSAN_OPTIONS": "halt_on_error=1",
    "ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1",
    "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
}
REPORTS = ("ThreadSanitizer", "AddressSanitizer", "LeakSanitizer", "runtime error:", "hip_stub: VIOLATION")


def _probe(name):
    """the flags with which a one-line program links and starts (None: with none of the candidates), and the environment of its children"""
    src = os.path.join(OUT, "io_host_probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    env = dict(os.environ, **CHILD_ENV)
    for flags in BUILDS[name]:
        exe = os.path.join(OUT, "io_host_probe_" + name)
        if subprocess.run(["g++"] + flags + ["-o", exe, src], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode:
            continue
        if subprocess.run([exe], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0:
            return flags, env
        if name == "asan_ubsan":        # the leak check alone may be unavailable (it stops the process from a tracer); the stub counts what is left anyway
            env_nl = dict(env, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0")
            if subprocess.run([exe], env=env_nl, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0:
                return flags, env_nl
    return None, env


@pytest.fixture(scope="module")
def programs():
    """name -> (program, environment of its children), or (None, why not); the three compilations run side by side"""
    os.makedirs(OUT, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "io_host.cpp"), os.path.join(ROOT, "tests", "hip_host_stub", "hip_stub.cpp")]
    inc = ["-I", os.path.join(ROOT, "tests", "hip_host_stub"), "-I", os.path.join(ROOT, "nanosim_amd", "csrc")]
    out, running = {}, {}
    for name in BUILDS:
        flags, env = _probe(name)
        if flags is None:
            assert name != "plain", "g++ cannot build a plain program"
            out[name] = (None, "the %s runtime does not link or start here (g++ %s)" % (name, " ".join(BUILDS[name][-1])))
            continue
        exe = os.path.join(OUT, "io_host_" + name)
        cmd = ["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-pthread"] + inc + ["-o", exe] + srcs
        running[name] = (subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), exe, env)
    for name, (p, exe, env) in running.items():
        text = p.communicate()[0]
        assert p.returncode == 0, "building io_host (%s):\n%s" % (name, text[-4000:])
        out[name] = (exe, env)
    return out


def test_the_program_knows_exactly_these_scenarios(programs):
    exe, env = programs["plain"]
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 2 and r.stdout.split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("build", list(BUILDS))
def test_scenario(programs, tmp_path, build, scenario):
    exe, env = programs[build]
    if exe is None:
        pytest.skip(env)
    try:
        r = subprocess.run([exe, scenario, str(tmp_path), str(LIMIT_S)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=LIMIT_S + 30)
    except subprocess.TimeoutExpired as ex:
        seen = ex.stdout.decode(errors="replace") if isinstance(ex.stdout, bytes) else ex.stdout or ""
        pytest.fail("%s (%s) neither ended nor stopped itself within %d s:\n%s" % (scenario, build, LIMIT_S + 30, seen[-4000:]))
    assert r.returncode == 0, "%s (%s) exited with %d:\n%s" % (scenario, build, r.returncode, r.stdout[-6000:])
    assert not any(w in r.stdout for w in REPORTS), "%s (%s) left a report:\n%s" % (scenario, build, r.stdout[-6000:])
    assert r.stdout.strip().endswith("ok " + scenario)
    assert os.listdir(tmp_path) == []          # every file was compared with its reference and removed


def test_the_product_does_not_see_the_stub():
    """the stub's <hip/hip_runtime.h> must never shadow the real one: neither the library's build nor the benchmark names it"""
    for f in ("__graft_entry__.py", "bench.py"):
        with open(os.path.join(ROOT, f)) as fh:
            text = fh.read()
        assert "hip_host_stub" not in text and "io_host" not in text, f
