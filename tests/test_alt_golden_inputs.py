"""The alternate-allele goldens (tests/golden/alt_*_golden.npz) by themselves: the committed files contain
every case the GPU test relies on them for -- recounted here from the files, with floors -- and, where the
reference tree and its nosimd objects are present, tests/golden/make_alt_golden.py reproduces them byte for
byte."""
import glob
import importlib.util
import os

import pytest

import altsnp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_TREE = "/root/reference"
FILES = {"single": altsnp.GOLDEN_SINGLE, "end": altsnp.GOLDEN_END}


@pytest.fixture(scope="module", params=["single", "end"])
def recount(request):
    kind = request.param
    ref, alt, calls, outs = altsnp.load(FILES[kind])
    return kind, ref, alt, calls, outs, altsnp.count_cases(ref, alt, kind, calls, outs)


def test_alt_goldens_hold_the_generators_inputs(recount):
    kind, ref, alt, calls, outs, _ = recount
    assert (ref, alt) == altsnp.snp_genomes()
    want = altsnp.single_calls(ref, alt) if kind == "single" else altsnp.end_calls(ref, alt)
    assert calls == want
    assert set(outs) == set(altsnp.TAGS) and all(len(outs[t]) == len(calls) for t in altsnp.TAGS)
    assert 280 <= len(calls) <= 340
    assert os.path.getsize(FILES[kind]) < os.path.getsize(os.path.join(HERE, "golden", "single_gap_golden.npz"))


def test_alt_goldens_contain_every_case(recount):
    kind, ref, alt, calls, outs, k = recount
    print(kind, k)
    assert altsnp.missing_cases(kind, k) == []
    # SNP columns at the matrix edges, on band rows, adjacent; at the word and block boundaries
    for c in ("snp_c1", "snp_cglen", "snp_adjacent", "off15", "off16", "off31", "off32"):
        assert k[c] >= 10, c
    assert k["snp_band_rows"] >= 1000
    # the decode rule's two asymmetries
    assert k["refN_altACGT"] >= 10 and k["altN_refACGT"] >= 10
    # chromosome ends with a SNP beside the '*' columns
    assert k["past_chrhigh_snp"] >= 1 and k["before_chroffset_snp"] >= 1
    # the three-way emission and a path that moves
    assert k["match_alt_only"] >= 500 and k["mismatch_both"] >= 50 and k["mode1_amb_alt_only"] >= 5
    assert k["path_changed"] >= 20
    assert k["R1"] >= 200
    if kind == "single":
        assert k["simple_alt_only"] >= 4
        assert k["R2"] >= 5 and k["R4"] >= 5 and k["Wgt256"] >= 3 and k["dirs_global"] >= 3
    else:
        for c in ("end5_plus", "end5_minus", "end3_plus", "end3_minus", "nogaps", "indels", "gap", "local"):
            assert k[c] >= 30, c
        assert k["null"] >= 10 and k["dirs_global"] >= 3


def test_alt_effective_allele_rule():
    ref, alt = b"ACGTNNAC", b"CCGTAXNX"
    #            A->C SNP; N under ref N (both); alt N reads A (flag ignored): no SNP; alt X reads T
    assert altsnp.effective_alt(ref, alt) == b"CCGTNNAT"


def _ref_objects():
    return glob.glob(os.path.join(ROOT, "oracle", "_ref", "nosimd", "dynprog_single.o"))


@pytest.mark.skipif(not (_ref_objects() and os.path.isdir(os.path.join(REF_TREE, "src"))),
                    reason="needs the reference tree and its nosimd objects (build() where the tree is)")
def test_alt_goldens_regenerate_byte_for_byte(tmp_path):
    spec = importlib.util.spec_from_file_location("make_alt_golden", os.path.join(HERE, "golden", "make_alt_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.generate(REF_TREE, str(tmp_path))
    for path in FILES.values():
        with open(path, "rb") as a, open(os.path.join(str(tmp_path), os.path.basename(path)), "rb") as b:
            assert a.read() == b.read(), os.path.basename(path)
