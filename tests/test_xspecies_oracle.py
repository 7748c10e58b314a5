"""The cross-species chain oracle (tests/xoracle, GMAPDP_S2_CANONICAL_MIDDLE) on the CPU: it has not drifted
from the chain oracle it restates, its canonical-link predicate equals a brute-force form on a grid of edge
cases, and the flag changes the chains of the generated reads (so the GPU tests that compare with it have
power)."""
import importlib.util
import os

import numpy as np

from dpbind import Oracle
import xspecies as X

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_stage2_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.load_stage2(os.path.join(HERE, "golden", "stage2_golden.npz"))


def test_flag_off_equals_chain_oracle_on_golden():
    """Without the flag the copy is the chain oracle: all 300 calls of stage2_golden.npz."""
    g, probs, exp = _load_stage2_golden()
    assert len(probs) == 300
    orc = Oracle()
    xo = X.XOracle(orc)
    xo.set_genome(g)
    bad = [i for i, p in enumerate(probs) if xo.stage2_compute(p, 0) != orc.stage2_compute(p)]
    assert not bad, "calls where the cross-species oracle without the flag differs: %s" % bad[:10]
    assert all(xo.stage2_compute(p, 0) == exp[i] for i, p in enumerate(probs[:40]))


def test_predicate_oracle_vs_brute_force():
    """canonical_link as the reference writes it (two descending walks merged by shift) against the string
    compare per shift, on every pair of the grid, both strands, both chromosomes."""
    g, sites = X.grid_genome()
    maxent, keep = X.grid_maxent()
    xo = X.XOracle()
    xo.set_genome(g)
    seen, total, true = set(), 0, 0
    for chrom in (0, 1):
        for plusp in (1, 0):
            prev, curr, chroffset, chrhigh = X.grid_cases(chrom, plusp)
            got = xo.canonical_links(prev, curr, plusp, chroffset)
            for i in range(len(prev)):
                ans, cls = X.brute_canonical(g, maxent, int(prev[i]), int(curr[i]), plusp, chroffset)
                assert bool(got[i]) == ans, (chrom, plusp, int(prev[i]), int(curr[i]), ans, sorted(cls))
                seen |= {(c, plusp) for c in cls}
                if chrom == 1 and int(min(prev[i], curr[i])) < chroffset + 20:
                    seen.add(("near_chr2_start", plusp))
                total += 1
                true += ans
    print("grid: %d pairs, %d canonical (%.1f %%)" % (total, true, 100.0 * true / total))
    # every case class occurs, on both strands
    for cls in ("early", "n", "past_end", "pair_at_equal_shift", "unequal_shifts", "straddle", "weak_pair", "sense",
                "antisense", "shift_0", "shift_22", "shift_mid", "near_chr2_start"):
        for plusp in (1, 0):
            assert (cls, plusp) in seen, "case class %s never occurs on strand %d" % (cls, plusp)
    assert 0.05 * total <= true <= 0.95 * total, (true, total)
    assert X.GRID_CHR2 % 32 != 0


def test_predicate_window_edges():
    """The two windows' inclusive bounds: a combined site is seen exactly at the seed-end
    offsets that put it at shifts 0 .. 22, and not one past either end."""
    g, sites = X.grid_genome()
    xo = X.XOracle()
    xo.set_genome(g)
    a, b = 100, 227  # two combined sites of the first chromosome
    for plusp, up in ((1, X.MISS_BEHIND), (0, X.GREEDY_ADVANCE)):
        for k in range(-2, 26):
            low, high = a + k - up, b + k - up   # the sites at shift k
            prev, curr = (low, high) if plusp else (high, low)
            got = int(xo.canonical_links([prev], [curr], plusp, 0)[0])
            assert got == int(0 <= k <= 22), (plusp, k, got)


def test_chain_generator_has_power():
    """The flag changes at least a quarter of the generated calls, and both outcomes of a range-2 winner occur
    (penalised, and canonical so unpenalised): a condition on the generator, met by the oracle alone."""
    g, calls = X.chain_calls("spliced")
    off, on, (ncand, npen, ncanon) = X.chain_expected("spliced")
    assert len(calls) == 200
    assert {p["plusp"] for p in calls} == {0, 1}
    nsp0 = sum(1 for p in calls if not p["splicingp"])
    assert 0.08 * len(calls) <= nsp0 <= 0.25 * len(calls)
    assert all(300 <= len(p["quc"]) <= 600 for p in calls)
    differ = sum(1 for a, b in zip(off, on) if a != b)
    print("chains: %d of %d calls differ; range 2: %d candidates, winners %d penalised / %d canonical"
          % (differ, len(calls), ncand, npen, ncanon))
    assert not any(r[0] == "err" for r in off + on)
    assert 4 * differ >= len(calls), differ
    assert npen > 0 and ncanon > 0
    # the flag-off side of the generator is the plain chain oracle's
    orc = Oracle()
    orc.set_genome(g)
    assert all(orc.stage2_compute(p) == off[i] for i, p in enumerate(calls[:50]))


def test_short_and_repeat_generators_differ_too():
    for kind in ("short", "repeat"):
        off, on, (ncand, npen, ncanon) = X.chain_expected(kind, 60)
        differ = sum(1 for a, b in zip(off, on) if a != b)
        print("%s: %d of 60 differ; range 2: %d candidates, %d / %d" % (kind, differ, ncand, npen, ncanon))
        assert differ > 0 and ncand > 0 and npen > 0
