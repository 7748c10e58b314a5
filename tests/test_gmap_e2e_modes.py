"""End to end in GMAP's stranded bisulfite / RNA-editing modes: `gmap --mode=cmet-stranded`, `atoi-stranded`
and `ttoc-stranded` through the drop-in shim on the MI355X engine, byte for byte against the unmodified
reference program's output (tests/golden/make_e2e_modes.py: 60 converted reads per mode, ten of them with a
lower-case stretch, which pins convert_to_nucleotides' case-sensitive compare of the observed pairs).

Stage 2 in these modes reduces the genome of the seeding (Oligoindex_hr_tally) and marks the pairs whose
query character differs from the genome's with ':'; the engine implements the per-nucleotide rule of the
nosimd tally (count / store_positions_{fwd,rev}_std).  The AVX2 build has no ttoc fixture: the unmodified
AVX2 program crashes in that mode (its SIMD store pass lacks the TTOC arm its count pass has), and the
drop-in of that build refuses the mode.  The fixtures are stored gzipped; the reads are unpacked for gmap."""
import gzip
import os

import pytest

from test_gmap_e2e import GOLD, _exe, _run, _stats

MODES = ("cmet", "atoi", "ttoc")
FIXTURES = [(m, b) for m in MODES for b in ("nosimd", "avx2") if (m, b) != ("ttoc", "avx2")]


def _read(name):
    with gzip.open(os.path.join(GOLD, name + ".gz"), "rb") as f:
        return f.read().decode()


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """The unpacked read files, by mode."""
    d = tmp_path_factory.mktemp("e2e_mode_reads")
    out = {}
    for m in MODES:
        out[m] = str(d / ("e2e_mode_%s_reads.fa" % m))
        with open(out[m], "w") as f:
            f.write(_read("e2e_mode_%s_reads.fa" % m))
    return out


def _args(mode, reads):
    return ["--mode=%s" % mode, "-g", "e2e_genome.fa", "-f", "samse", "--no-sam-headers", reads]


def _same_sam(out, fixture):
    exp = _read(fixture).splitlines()
    got = out.splitlines()
    bad = [i for i, (x, y) in enumerate(zip(got, exp)) if x != y]
    assert out == _read(fixture), "records %d vs %d, differing: %s" % (len(got), len(exp), bad[:10])


@pytest.mark.parametrize("mode,build", FIXTURES)
def test_reference_gmap_reproduces_mode_fixtures(reads, mode, build):
    assert _run(_exe("gmap_" + build), _args(mode + "-stranded", reads[mode]))[0] == \
        _read("e2e_mode_%s_%s.sam" % (mode, build))


@pytest.mark.parametrize("mode", MODES)
def test_mode_fixtures_differ_from_standard(reads, mode):
    """The mode matters on these reads: the same reads in --mode=standard align differently (most of them),
    and the lower-cased reads are among the fixture's records."""
    std = _run(_exe("gmap_nosimd"), _args("standard", reads[mode]))[0].splitlines()
    fix = _read("e2e_mode_%s_nosimd.sam" % mode).splitlines()
    assert len(fix) >= 56
    by_name = {}
    for line in std:
        by_name.setdefault(line.split("\t")[0], []).append(line)
    ndiff = sum(1 for line in fix if line not in by_name.get(line.split("\t")[0], []))
    assert 2 * ndiff >= len(fix), (ndiff, len(fix))
    fa = _read("e2e_mode_%s_reads.fa" % mode)
    assert sum(1 for r in fa.split(">")[1:] if any(c.islower() for c in "".join(r.split("\n")[1:]))) == 10


@pytest.mark.gpu
@pytest.mark.parametrize("mode,build,threads", [(m, "nosimd", t) for m in MODES for t in (1, 16)] +
                         [(m, "avx2", 1) for m in MODES if (m, "avx2") in FIXTURES])
def test_gpu_gmap_stranded_modes(reads, mode, build, threads):
    """The drop-in in the mode: SAM identical to the reference program's, with Stage2_compute and the
    oligoindex pair (stage 3's Stage2_compute_one / _starts / _ends callers) on the engine and no refusal
    (the shim aborts on one)."""
    args = _args(mode + "-stranded", reads[mode])
    if threads > 1:
        args = ["-t", str(threads), "-O"] + args
    out, err = _run(_exe("gmap_gpu_" + build), args, env={"GMAPDP_SHIM_STATS": "1"})
    _same_sam(out, "e2e_mode_%s_%s.sam" % (mode, build))
    assert "is not supported by the MI355X" not in err
    st = _stats(err)
    assert st["Stage2_compute"] > 0 and st["Dynprog_genome_gap"] > 0, st
    assert st["Oligoindex_get_mappings"] > 0, st
