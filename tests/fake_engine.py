"""Stand-ins for nanosim_amd.engine.Engine for the CLI's host logic without a GPU: a batch is the text `>read_<i>` / one error row per
read index, so a file's bytes say which read ranges reached it, in which order."""
import os
import threading

import numpy as np


class _FakeInfo:
    def __init__(self, n, rec, err):
        self.n_reads, self.record_bytes, self.errlog_bytes, self.ms_total = n, rec, err, 0.0


class _FakeBatch:
    def __init__(self, first, n, with_err):
        self.rec = [b">read_%d\nACGT\n" % i for i in range(first, first + n)]
        self.err = [b"read_%d\t0\tmis\t1\tA\tC\n" % i for i in range(first, first + n)] if with_err else []
        self.info = _FakeInfo(n, sum(map(len, self.rec)), sum(map(len, self.err)))

    def record_offsets(self, cuts):
        ro = np.array([sum(map(len, self.rec[:c])) for c in cuts], dtype=np.uint64)
        eo = np.array([sum(map(len, self.err[:c])) for c in cuts], dtype=np.uint64)
        return ro, eo


class _FakeSink:
    def __init__(self, eng, fd):
        self.eng, self.fd, self.closed = eng, fd, 0

    def put(self, data):
        os.write(self.fd, data)

    def write(self, which, offset=0, nbytes=None):
        b = self.eng.last
        img = b"".join(b.rec if which == 0 else b.err)
        os.write(self.fd, img[offset:] if nbytes is None else img[offset:offset + nbytes])

    def drain(self):
        return 0

    def close(self):
        self.closed += 1
        assert self.closed == 1, "a sink was closed twice"
        if self.eng.fail_close:
            raise OSError(28, "No space left on device")


class _FakeEngine:
    def __init__(self, fail_close=False, fail_generate_at=None):
        self.fail_close, self.fail_generate_at, self.sinks, self.calls = fail_close, fail_generate_at, [], 0

    def generate(self, p):
        self.calls += 1
        if self.fail_generate_at is not None and self.calls >= self.fail_generate_at:
            raise RuntimeError("device lost")
        self.last = _FakeBatch(int(p.first_read), int(p.n_reads), bool(p.emit_errlog))
        return self.last

    def sink(self, fd):
        s = _FakeSink(self, fd)
        self.sinks.append(s)
        return s

    def io_counters(self):
        return dict(bytes=0, d2h_gbs=None, wait_staging_s=0.0, write_s=0.0)


REQUEST_FIELDS = ("first_read", "n_reads", "kind", "fastq", "chimeric", "kmer_bias", "min_len", "max_len", "emit_errlog", "meta", "trx",
                  "uracil", "model_ir")


class RecordingEngine(_FakeEngine):
    """What simulator.main uses of an Engine, recorded: `setup` = the set_* / load_model / step_engine calls in order, each with the
    names of its keyword arguments; `requests` = REQUEST_FIELDS of every worker call this engine served (a step: the aligned half here,
    the unaligned half on the companion); `world.created` / `world.closed` = every engine and companion, in order."""

    def __init__(self, world, owner=None, fail_generate_at=None):
        super().__init__(fail_generate_at=fail_generate_at)
        self.world, self.owner, self.companion, self.background = world, owner, None, None
        self.setup, self.requests = [], []
        with world.lock:
            self.index = len(world.created)
            world.created.append(self)

    def __getattr__(self, name):
        if not (name.startswith("set_") or name == "load_model"):
            raise AttributeError(name)

        def record(*args, **kw):
            if name == "set_background":
                self.background = args[0]
            self.setup.append((name, tuple(sorted(kw))))
        return record

    def step_engine(self):
        self.setup.append(("step_engine", ()))
        if self.companion is None:
            self.companion = RecordingEngine(self.world, owner=self)
        return self.companion

    def _serve(self, p):
        self.requests.append(tuple(int(getattr(p, f)) for f in REQUEST_FIELDS))
        return super().generate(p)

    def generate(self, p):
        return self._serve(p)

    def generate_step(self, pa, pu):
        b_al = self._serve(pa)
        return b_al, self.companion._serve(pu)

    def close(self):
        with self.world.lock:
            self.world.closed.append(self)


class EngineWorld:
    """`monkeypatch.setattr(engine, "Engine", world)`: every Engine(device) of the run is a RecordingEngine of this world; the first one
    fails its `fail_generate_at`-th worker call"""

    def __init__(self, fail_generate_at=None):
        self.created, self.closed, self.lock, self.fail_generate_at = [], [], threading.Lock(), fail_generate_at

    def __call__(self, device=0):
        return RecordingEngine(self, fail_generate_at=self.fail_generate_at if not self.created else None)
