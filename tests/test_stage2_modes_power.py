"""CPU side of the stranded cmet / atoi / ttoc stage-2 tests: the genome reductions' bit formulas
(csrc/oi_reduce.h, a stand-alone program under the address and undefined-behaviour sanitizers), and the power
of the GPU tests' inputs (tests/s2modes.py): an engine that ignored the mode would compute the oracle's
result on the unreduced genome G, so that result must differ from the expected one, the oracle's on G', in at
least half of each mode's calls, and at least a quarter of the expected pair records must carry ':'."""
import os
import subprocess

import numpy as np
import pytest

import gmapdp
import s2modes
from dpbind import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))


def test_reductions_under_address_and_undefined_sanitizers(tmp_path):
    """tests/oi_reduce_check.cpp: all 2^16 patterns in both halves of a word, each reduction's formula and the
    kernels' masked 64-bit form against a per-nucleotide loop, and the (mode, plusp) selection table."""
    exe = tmp_path / "oi_reduce_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", os.path.join(HERE, "oi_reduce_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith(", 0 bad"), r.stdout


def test_reduced_genome_is_the_word_reduction():
    """s2modes.reduced_genome (letters) is the reduction of the packed genome's codes: A=0 C=1 G=2 T=3."""
    code = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    want = {1: ({1: 3}, {2: 0}), 3: ({3: 1}, {0: 2}), 5: ({0: 2}, {3: 1})}  # ct/ga, tc/ag, ag/tc
    for mode in s2modes.MODES:
        for plusp in (1, 0):
            red = s2modes.reduced_genome(b"ACGT", mode, plusp)
            m = want[mode][0 if plusp else 1]
            assert [code[c] for c in red] == [m.get(c, c) for c in range(4)], (mode, plusp, red)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.mark.parametrize("mode", s2modes.MODES)
def test_seeding_inputs_tell_the_mode_from_standard(oracle, mode):
    g = s2modes.seeding_genome()
    calls = s2modes.seeding_calls(g, mode)
    assert 40 <= len(calls) <= 56
    assert {(c["plusp"], c["minor"]) for c in calls} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(40 <= len(c["quc"]) <= 600 and 300 <= c["chrend"] - c["chrstart"] <= 8000 for c in calls)
    exp = s2modes.seeding_expected(oracle, g, mode, calls)
    std = s2modes.seeding_expected(oracle, g, 0, calls)
    differ = sum(1 for a, b in zip(exp, std) if a != b)
    assert 2 * differ >= len(calls), (differ, len(calls))
    assert sum(1 for e in exp if e[0][0] > 0) >= len(calls) // 2    # and the mode's reads do seed
    # the planted stretch: in the mode the homopolymer 8-mer stands more than 255 times in the window, so its
    # count wraps; in STANDARD it does not occur at all
    for c, e, s in zip(calls[:8], exp[:8], std[:8]):
        at, letter = s2modes.homopolymer_stretch(mode, c["plusp"])
        assert c["chrstart"] <= at and at + s2modes.STRETCH_LEN <= c["chrend"]
        i = c["quc"].find(letter * 8)
        assert i >= 0
        w = s2modes.reduced_genome(g, mode, c["plusp"])[c["chrstart"]:c["chrend"]]
        fw = letter if c["plusp"] else letter.translate(s2modes.COMP)
        n = sum(1 for k in range(len(w) - 7) if w[k:k + 8] == fw * 8)
        assert n > 255 and e[1][i] == (n & 255), (n, e[1][i])
        assert s[1][i] == 0 and g[c["chrstart"]:c["chrend"]].count(fw * 8) == 0


@pytest.mark.parametrize("mode", s2modes.MODES)
def test_stage2_inputs_tell_the_mode_from_standard(oracle, mode):
    g = s2modes.stage2_genome(mode)
    calls = s2modes.stage2_calls(g, mode)
    assert 32 <= len(calls) <= 48
    assert {(c["plusp"], c["splicingp"]) for c in calls} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c["maxintronlen"] for c in calls} == {2000, 500000}
    assert all(300 <= len(c["quc"]) <= 1000 and c["q"] == c["quc"].upper() for c in calls)
    assert all(20000 <= c["chrend"] - c["chrstart"] <= 60000 for c in calls[:-2])
    probs, qb, qub = gmapdp.Engine.build_stage2_batch(calls)
    exp, nrec, ncolon = s2modes.stage2_expected(oracle, g, mode, probs, qb, qub)
    # the oracle on G' before the records are rewritten, against the oracle on G
    red, _, _ = s2modes.stage2_expected(oracle, g, mode, probs, qb, qub, rewrite=False)
    std, _, _ = s2modes.stage2_expected(oracle, g, 0, probs, qb, qub)
    assert np.all(exp[0][:, 0] >= 0) and np.all(std[0][:, 0] >= 0)
    po = exp[3]
    differ = 0
    for i in range(len(calls)):
        a = slice(20 * int(po[i]), 20 * int(po[i + 1]))
        same = (np.array_equal(red[0][i], std[0][i]) and np.array_equal(red[1][i], std[1][i])
                and np.array_equal(red[2][a], std[2][a]))
        differ += 0 if same else 1
    assert 2 * differ >= len(calls), (differ, len(calls))
    assert sum(1 for i in range(len(calls)) if exp[0][i, 0] > 0) >= len(calls) // 2  # the mode's reads do align
    assert nrec > 0 and 4 * ncolon >= nrec, (ncolon, nrec)
