"""The record kernels at their rare inputs, byte for byte against the oracle: ambiguity codes at every position of a chunk, several in one
sub-run, at the ends of an event sub-run, under / next to substitutions of 1 .. 20 letters, in both parts of a payload cut by a tile end —
on a FASTA and a FASTQ batch, through the scratch pass of -k, in chimeric reads, on a circular reference (wrapped pieces keep their
per-byte path) and in the dense kernel of unaligned reads.  Cases, models, references and the reach check (on the oracle alone) are those
of tests/test_record_rare_paths.py."""
import pytest

from nanosim_amd import engine as E
from tests.test_gpu_parity import compare
from tests.test_record_rare_paths import CASES, build_models, build_refs, check_reach, oracle_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return build_models(tmp_path_factory.mktemp("gpu_record_rare_paths"))


@pytest.fixture(scope="module")
def refs():
    return build_refs()


@pytest.fixture(scope="module")
def engines(refs):
    made = {}

    def get(rname):
        if rname not in made:
            e = E.Engine(0)
            e.set_reference(refs[rname])
            made[rname] = e
        return made[rname]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("cid,rname,mname,case,reach", CASES, ids=[c[0] for c in CASES])
def test_gpu_rare_paths_equal_oracle(engines, models, refs, cid, rname, mname, case, reach):
    p, exp = oracle_case(cid, rname, mname, case, models, refs)
    check_reach(cid, rname, p, exp, reach, refs)
    eng = engines(rname)
    eng.load_model(models[mname])
    compare(eng.generate(p), exp, p)
