#!/usr/bin/env python3
"""Host timing of the seven SAM text readers of nanosim_amd.characterize (no GPU): two SAM texts of about 200 000 records each, made
by repeating the records of the fixtures the reader tests use under one header — tests/golden/reference_chimeric_train.json.gz as it
stands (length_records, primary_and_unaligned, chimeric_records, _mapped_records) and the records of
tests/golden/reference_sam_pairs.json.gz, which carry MD:Z and SEQ, with a QUAL of their length (cs_from_sam, quals_from_sam,
sam_records).  Prints one JSON line: per reader the seconds of every run, their median and (max - min) / median.

    python scripts/bench_sam_readers.py [--records 200000] [--runs 5] [--only length_records,_mapped_records]
    python scripts/bench_sam_readers.py --against /path/to/the/parent's/nanosim_amd/characterize.py

With --against the readers of that single-file module are timed in the same process, run for run in turn with the package's (the
level of a shared machine drifts by more than the difference looked for), and every reader gets `parent`, `ratio` (median over median)
and `allowed` = 1 + max(the parent's spread, 0.10).
"""
import argparse
import gc
import gzip
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("NS_PACKAGE_ROOT", ROOT))


def fixture(name):
    with gzip.open(os.path.join(ROOT, "tests", "golden", name), "rt") as f:
        return json.load(f)


def repeated(header, records, n):
    return "".join(header) + "".join(records) * (n // len(records)) + "".join(records[:n % len(records)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated reader names (default: all seven)")
    ap.add_argument("--against", default=None, help="the characterize.py of the parent commit")
    args = ap.parse_args()
    from nanosim_amd import characterize
    parent = None
    if args.against:
        spec = importlib.util.spec_from_file_location("characterize_parent", args.against)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)

    lines = fixture("reference_chimeric_train.json.gz")["sam"].splitlines(True)
    header = [x for x in lines if x.startswith("@")]
    chim_text = repeated(header, [x for x in lines if not x.startswith("@")], args.records)
    pairs = ["\t".join([q, str(flag), rname, str(pos), "60", cigar, "*", "0", "0", seq, "I" * len(seq), "NM:i:0", "MD:Z:" + md]) + "\n"
             for q, flag, rname, pos, cigar, md, seq in fixture("reference_sam_pairs.json.gz")["records"]]
    pairs_text = repeated(header, pairs, args.records)
    readers = (("cs_from_sam", "pairs"), ("quals_from_sam", "pairs"), ("sam_records", "pairs"), ("length_records", "chim"),
               ("primary_and_unaligned", "chim"), ("chimeric_records", "chim"), ("_mapped_records", "chim"))

    def timed(module, name, path):
        reader = getattr(module, name)
        gc.collect()                                        # (what the run before left behind is not this run's to collect)
        t0 = time.perf_counter()
        if name == "_mapped_records":
            sum(1 for _ in reader(path))
        else:
            reader(path)
        return time.perf_counter() - t0

    def figures(runs):
        med = statistics.median(runs)
        return dict(runs=[round(t, 4) for t in runs], median=round(med, 4), spread=round((max(runs) - min(runs)) / med, 4))
    out = {}
    with tempfile.TemporaryDirectory(prefix="nssam_") as work:
        paths = {}
        for key, text in (("chim", chim_text), ("pairs", pairs_text)):
            paths[key] = os.path.join(work, key + ".sam")
            with open(paths[key], "w") as f:
                f.write(text)
        for name, key in readers:
            if args.only and name not in args.only.split(","):
                continue
            runs, parent_runs = [], []
            for _ in range(args.runs):
                if parent is not None:
                    parent_runs.append(timed(parent, name, paths[key]))
                runs.append(timed(characterize, name, paths[key]))
            out[name] = figures(runs)
            if parent is not None:
                out[name]["parent"] = figures(parent_runs)
                out[name]["ratio"] = round(out[name]["median"] / out[name]["parent"]["median"], 4)
                out[name]["allowed"] = round(1 + max(out[name]["parent"]["spread"], 0.10), 4)
    print(json.dumps(dict(records=args.records, package=os.path.dirname(characterize.__file__), readers=out)))


if __name__ == "__main__":
    main()
