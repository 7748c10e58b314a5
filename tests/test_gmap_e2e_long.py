"""End-to-end with long reads: four 20-40-kb spliced transcripts (more than 16 384 distinct 8-mers each)
between ten 2-kb reads (tests/golden/make_e2e_long.py) through the drop-in, byte for byte against the reference
program's SAM.  Before the seeding's long class the engine refused such a query and the shim aborted the run."""
import gzip
import os
import sys

import pytest

from test_gmap_e2e import GOLD, BUILDS, _exe, _run, _stats

sys.path.insert(0, GOLD)
import make_e2e_long  # noqa: E402

ARGS = make_e2e_long.ARGS
REFUSAL = "distinct 8-mers"


def _fixture(build):
    with gzip.open(os.path.join(GOLD, "e2e_long_%s.sam.gz" % build)) as f:
        return f.read().decode()


def _reads():
    return make_e2e_long.read_fasta(os.path.join(GOLD, "e2e_long_reads.fa"))


def test_reads_file_is_the_generators():
    assert _reads() == make_e2e_long.reads()


def test_long_reads_are_long_and_aligned_in_the_fixture():
    """Every long read has more than 16 384 distinct 8-mers and an aligned record (flag 0 or 16, a position, its
    whole sequence) in both builds' fixtures."""
    longs = {n: s for n, s in _reads() if n.startswith("long")}
    assert len(longs) == 4 and sorted(n[-1] for n in longs) == ["+", "+", "-", "-"]
    for n, s in longs.items():
        assert 20000 <= len(s) <= 40000
        assert len({s[i:i + 8] for i in range(len(s) - 7)}) > 16384
    for build in BUILDS:
        recs = [l.split("\t") for l in _fixture(build).splitlines()]
        assert [r[0] for r in recs] == [n for n, _ in _reads()]
        for r in recs:
            if r[0] in longs:
                assert r[1] in ("0", "16") and int(r[3]) > 0 and len(r[9]) == len(longs[r[0]]), r[:9]


@pytest.mark.parametrize("build", BUILDS)
def test_reference_gmap_reproduces_long_fixture(build):
    assert _run(_exe("gmap_" + build), ARGS)[0] == _fixture(build)


@pytest.mark.gpu
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("opts", [[], ["-t", "16", "-O"]], ids=["plain", "t16"])
def test_gpu_gmap_long_reads(build, opts):
    """The fixture byte for byte, the long reads' Stage2_compute calls in the long class, and no refusal (the 8-MB
    fiber stacks of the worker threads hold stage 3 of a 36-kb read: the run ends with exit status 0)."""
    out, err = _run(_exe("gmap_gpu_" + build), opts + ARGS, env={"GMAPDP_SHIM_STATS": "1"})
    assert out == _fixture(build)
    st = _stats(err)
    assert st["Stage2_compute_long"] > 0, st
    assert st["Stage2_compute"] > st["Stage2_compute_long"], st
    assert REFUSAL not in err and "GMAPDP_EINVAL" not in err
