"""Long queries (more than 16 384 distinct 8-mers) on the CPU: the oracle pinned to the reference on the calls
the GPU tests use (tests/longq.py), a stored fixture of the reference's outputs for machines without the
reference tree, and the generator's own promises, checked with the oracle alone."""
import os
import sys

import numpy as np
import pytest

import longq
from dpbind import Oracle, Ref, ref_available

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_long_query import golden_calls, pack  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "long_query_golden.npz")


@pytest.fixture(scope="module")
def world():
    g = longq.genome()
    orc = Oracle()
    orc.set_genome(g)
    return dict(g=g, orc=orc)


@pytest.mark.skipif(not ref_available(), reason="reference harness not built (oracle/_ref)")
def test_oracle_equals_reference_on_long_queries(world):
    """Cases B and D, both strands: every output of Oligoindex_hr_tally + Oligoindex_get_mappings and of
    Stage2_compute."""
    g, orc = world["g"], world["orc"]
    ref = Ref()
    ref.set_genome(g)
    calls = [c for c, _ in longq.spliced_calls(g)] + longq.wrap_calls(g)
    assert {c["plusp"] for c in calls} == {0, 1}
    for i, c in enumerate(calls):
        assert orc.oligo_mappings(c) == ref.oligo_mappings(c), i
        assert orc.stage2_compute(c) == ref.stage2_compute(c), i


def test_oracle_reproduces_the_reference_fixture(world):
    got = pack(world["orc"], golden_calls(world["g"]))
    with np.load(GOLDEN) as exp:
        assert sorted(exp.files) == sorted(got)
        for k in exp.files:
            assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), k


def test_de_bruijn_prefixes_have_the_distinct_counts_they_claim():
    for n in longq.BOUNDARY_N + (1, 60000 - 7):
        q = longq.prefix(n)
        assert len(q) == n + 7 and longq.distinct_8mers(q) == n, n


def test_spliced_reads_chain_and_seed_every_exon(world):
    """Case B: 18 000-24 000 distinct 8-mers, Stage2_compute chains (at least one path), and every exon has a
    good diagonal of its own."""
    g, orc = world["g"], world["orc"]
    for c, exons in longq.spliced_calls(g):
        assert 18000 <= longq.distinct_8mers(c["quc"]) <= 24000
        n, lists = orc.stage2_compute(c)
        assert n >= 1 and len(lists[0]) > 20000
        sc, _, _, dg = orc.oligo_mappings(c)
        assert sc[2] == 1
        qlen, lo = len(c["quc"]), c["chrstart"]
        found = {d[0] for d in dg}
        for qs, gs in exons:
            # the diagonal of an exon: genome offset in the window minus query offset (plus strand); on the
            # minus strand the query runs backwards over the window, which there ends one past chrend
            if c["plusp"]:
                d = (gs - lo) - qs
            else:
                d = (c["chrend"] + 1 - (gs + 3000)) - (qlen - (qs + 3000))
            assert d >= 0 and d in found, (qs, gs, d)


def test_wrap_reads_wrap_on_a_high_id(world):
    """Case D: an 8-mer of the query occurs at least 256 times in the window, and one such 8-mer has an id (its
    rank among the query's distinct 8-mers, in oligo order) of 49 152 or more."""
    g = world["g"]
    code = {65: 0, 67: 1, 71: 2, 84: 3}

    def oligo(k):
        v = 0
        for ch in k:
            v = 4 * v + code[ch]
        return v
    for c in longq.wrap_calls(g):
        q = c["quc"]
        qset = sorted({oligo(q[i:i + 8]) for i in range(len(q) - 7) if b"N" not in q[i:i + 8]})
        w = g[c["chrstart"]:c["chrend"]]
        w = w if c["plusp"] else longq.revcomp(w)
        counts = {}
        for i in range(len(w) - 7):
            k = w[i:i + 8]
            if b"N" not in k:
                counts[k] = counts.get(k, 0) + 1
        rank = {m: i for i, m in enumerate(qset)}
        high = [rank[oligo(k)] for k, n in counts.items() if n >= 256 and oligo(k) in rank]
        assert high and max(high) >= 49152, high
