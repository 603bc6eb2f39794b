#!/usr/bin/env python3
"""Golden fixture of the SAM text readers (tests/test_sam_text.py): what cs_from_sam, quals_from_sam, sam_records, length_records,
primary_and_unaligned, chimeric_records and _mapped_records of nanosim_amd.characterize return or raise on every variant of the test's
SAM text.  The file in the repository was written by the readers as they stood before they shared one loop; of the package this script
uses nanosim_amd.characterize alone (through the test's `observe`), so it runs against any later state and has to reproduce the file
byte for byte.

    python tests/golden/make_sam_readers_golden.py        -> tests/golden/sam_readers.json
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.test_sam_text import VARIANTS, observe, text_of      # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory(prefix="nssam_") as work:
        for variant in VARIANTS:
            path = os.path.join(work, variant + ".sam")
            with open(path, "w") as f:
                f.write(text_of(variant))
            out[variant] = observe(path)
    target = os.path.join(HERE, "sam_readers.json")
    with open(target, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", target, os.path.getsize(target), "bytes")


if __name__ == "__main__":
    main()
