"""End to end under `gmap --cross-species` (Stage2_setup's cross_species_p: canonical scoring of stage 2's
middle links): the drop-in shim on the MI355X engine, byte for byte against the unmodified reference
program's output (tests/golden/make_e2e_xspecies.py), in STANDARD mode on the 200 reads and in cmet-stranded
mode on the 60 converted reads.  The shim sends the option as GMAPDP_S2_CANONICAL_MIDDLE; before that it
refused the first Stage2_compute call.  The fixtures are stored gzipped."""
import gzip
import os

import pytest

from test_gmap_e2e import GOLD, _exe, _run, _stats

TAIL = ["-g", "e2e_genome.fa", "-f", "samse", "--no-sam-headers"]


def _read(name):
    with gzip.open(os.path.join(GOLD, name + ".gz"), "rb") as f:
        return f.read().decode()


@pytest.fixture(scope="module")
def cmet_reads(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("e2e_xspecies") / "e2e_mode_cmet_reads.fa")
    with open(path, "w") as f:
        f.write(_read("e2e_mode_cmet_reads.fa"))
    return path


def _ndiff(a, b):
    a, b = a.splitlines(), b.splitlines()
    assert len(a) == len(b)
    return sum(1 for x, y in zip(a, b) if x != y)


def test_xspecies_fixtures_differ_from_default():
    """The option matters on these reads (29 of 200 and 11 of 60 records were measured)."""
    with open(os.path.join(GOLD, "e2e_nosimd.sam")) as f:
        std = f.read()
    fix = _read("e2e_xspecies_nosimd.sam")
    assert len(fix.splitlines()) == 200
    assert _ndiff(fix, std) >= 20
    cm = _read("e2e_xspecies_cmet_nosimd.sam")
    assert len(cm.splitlines()) == 60
    assert _ndiff(cm, _read("e2e_mode_cmet_nosimd.sam")) >= 8


@pytest.mark.parametrize("build", ("nosimd", "avx2"))
def test_reference_gmap_reproduces_xspecies_fixtures(build, cmet_reads):
    assert _run(_exe("gmap_" + build), ["--cross-species"] + TAIL + ["e2e_reads.fa"])[0] == \
        _read("e2e_xspecies_%s.sam" % build)
    assert _run(_exe("gmap_" + build), ["--mode=cmet-stranded", "--cross-species"] + TAIL + [cmet_reads])[0] == \
        _read("e2e_xspecies_cmet_%s.sam" % build)


def _gpu(build, args, fixture, ordered=True):
    out, err = _run(_exe("gmap_gpu_" + build), args, env={"GMAPDP_SHIM_STATS": "1"})
    exp = _read(fixture)
    if not ordered:
        # several worker threads without -O: gmap writes the records as the threads finish them, so the same
        # records, each byte for byte, in any order
        assert out.endswith("\n") and len(out) == len(exp)
        out, exp = "".join(sorted(out.splitlines(True))), "".join(sorted(exp.splitlines(True)))
    bad = [i for i, (x, y) in enumerate(zip(out.splitlines(), exp.splitlines())) if x != y]
    assert out == exp, "records differing from the reference program's: %s" % bad[:10]
    assert "is not supported by the MI355X" not in err
    st = _stats(err)
    assert st["Stage2_compute"] > 0 and st["Stage2_compute_cross_species"] > 0, st
    assert st["Stage2_compute_cross_species"] == st["Stage2_compute"], st
    assert st["Dynprog_genome_gap"] > 0 and st["Oligoindex_get_mappings"] > 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("build,opts", [("nosimd", []), ("nosimd", ["-t", "16", "-O"]), ("avx2", ["-t", "16"]),
                                        ("avx2", ["-t", "16", "-O"])])
def test_gpu_gmap_cross_species(build, opts):
    _gpu(build, opts + ["--cross-species"] + TAIL + ["e2e_reads.fa"], "e2e_xspecies_%s.sam" % build,
         ordered="-O" in opts or "-t" not in opts)


@pytest.mark.gpu
def test_gpu_gmap_cross_species_cmet(cmet_reads):
    _gpu("nosimd", ["--mode=cmet-stranded", "--cross-species"] + TAIL + [cmet_reads], "e2e_xspecies_cmet_nosimd.sam")
