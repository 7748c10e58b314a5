"""GPU parity tests for stage 2 with cross-species canonical scoring (gmap --cross-species,
GMAPDP_S2_CANONICAL_MIDDLE): the device predicate (canon_device.h) against the oracle's reference-shaped
form on the edge-case grid, and the flagged sweep (s2b_canon_kernel) against the cross-species chain oracle
(tests/xoracle) through the batch, the plan (whole and split), the fetch and the compact stream.  Bar:
identical answers; identical result lists and every pair record of every kept path."""
import numpy as np
import pytest

import gmapdp
from dpbind import Oracle
import xspecies as X

pytestmark = pytest.mark.gpu

KINDS = (("spliced", 200), ("short", 60), ("repeat", 30))


@pytest.fixture(scope="module")
def engine():
    e = gmapdp.Engine(0)
    yield e
    e.close()


def _decode(results, paths, pairs):
    """Engine.stage2_batch's format from the raw arrays."""
    out = []
    for r in results:
        lists = []
        for k in range(int(r["nresults"])):
            pr = paths[int(r["path_offset"]) + k]
            o, m = int(pr["pair_offset"]), int(pr["npairs"])
            lists.append([(int(x["querypos"]), int(x["genomepos"]), int(x["queryjump"]), int(x["genomejump"]), 0,
                           bytes(x["cdna"]) or b"\0", bytes(x["comp"]) or b"\0", bytes(x["genome"]) or b"\0",
                           bytes(x["genomealt"]) or b"\0", 1 if x["querypos"] == -1 and x["genomepos"] == -1 else 0)
                          for x in pairs[o:o + m]])
        out.append((int(r["nresults"]), lists))
    return out


def _same(got, exp, what):
    bad = [i for i, (a, b) in enumerate(zip(got, exp)) if a != b]
    assert len(got) == len(exp) and not bad, "%s: calls differing from the oracle: %s" % (what, bad[:10])


def test_gpu_canonical_links_grid(engine):
    """gmapdp_canonical_links on every pair of the grid (both strands, both chromosomes) against the
    oracle's walk-merge form -- which tests/test_xspecies_oracle.py pins to the brute-force form."""
    g, _ = X.grid_genome()
    engine.set_genome(g)
    xo = X.XOracle()
    xo.set_genome(g)
    total = true = 0
    for chrom in (0, 1):
        for plusp in (1, 0):
            prev, curr, chroffset, chrhigh = X.grid_cases(chrom, plusp)
            got = engine.canonical_links(prev, curr, plusp, chroffset, chrhigh)
            exp = xo.canonical_links(prev, curr, plusp, chroffset)
            bad = np.nonzero(got != exp)[0]
            assert not len(bad), (chrom, plusp, [(int(prev[i]), int(curr[i]), int(got[i])) for i in bad[:10]])
            total += len(exp)
            true += int(exp.sum())
    assert 0.05 * total <= true <= 0.95 * total


@pytest.fixture(scope="module")
def runs(engine):
    """Per generator: the flagged batch, the canonical sweep's counters over it, the unflagged batch and the
    counters over that (one run each, shared by the tests below)."""
    out = {}
    for kind, n in KINDS:
        g, calls = X.chain_calls(kind, n)
        engine.set_genome(g)
        engine.canon_counters()
        on = engine.stage2_batch(calls, cross_species=True)
        forms = engine.canon_counters()
        off = engine.stage2_batch(calls, cross_species=False)
        out[kind] = (on, forms, off, engine.canon_counters())
        print("%s: range-2 candidates by form %s, MaxEnt-evaluated shifts %d" % (kind, forms[:7], forms[7]))
    return out


@pytest.mark.parametrize("kind,n", KINDS)
def test_gpu_stage2_batch_cross_species(runs, kind, n):
    g, calls = X.chain_calls(kind, n)
    off, on, _ = X.chain_expected(kind, n)
    got_on, forms, got_off, forms_off = runs[kind]
    _same(got_on, on, kind + " with the flag")
    assert forms_off == [0] * 8          # without the flag the default sweep ran, not the canonical one
    _same(got_off, off, kind + " without the flag")
    orc = Oracle()
    orc.set_genome(g)
    _same(got_off, [orc.stage2_compute(p) for p in calls], kind + " without the flag, chain oracle")
    assert sum(1 for a, b in zip(off, on) if a != b) > 0
    assert sum(forms[:7]) > 0 and forms[7] > 0
    if kind == "short":      # one hit per position: the one-step window of one-hit entries
        assert forms[3] > 0, forms
    if kind == "repeat":     # many active hits per position: _mult, 64-lane chunks, multi-hit windows
        assert forms[5] + forms[6] > 0 and forms[1] + forms[6] > 0 and forms[4] > 0, forms


def test_gpu_every_form_of_range2_ran(runs):
    """Over the three generators every form of the range-2 evaluation tested candidates (the kernels' own
    counters): s2_eval's scalar form and chunks, s2_eval1, the two one-step windows, and _mult's use."""
    tot = [sum(r[1][i] for r in runs.values()) for i in range(8)]
    assert all(t > 0 for t in tot), tot


def test_gpu_stage2_plan_cross_species(engine):
    g, calls = X.chain_calls("spliced", 200)
    off, on, _ = X.chain_expected("spliced", 200)
    engine.set_genome(g)
    probs, qbuf, qucbuf = engine.build_stage2_batch(calls, cross_species=True)
    batch = _decode(*engine.stage2_batch_raw(probs, qbuf, qucbuf))
    _same(batch, on, "batch")
    compact = {}
    r3 = engine.stage2_plan_raw(probs, qbuf, qucbuf, compact_out=compact)
    assert _decode(*r3[:3]) == batch                       # what = 3
    assert _decode(r3[0], r3[1], compact["pairs"]) == batch  # the compact stream of the same run
    rs = engine.stage2_plan_raw(probs, qbuf, qucbuf, whats=(1, 4, 8, 16))
    assert _decode(*rs[:3]) == batch                       # the split chain
    rr = engine.stage2_plan_raw(probs, qbuf, qucbuf, reruns=2)
    assert _decode(*rr[:3]) == batch                       # a plan rerun: the same output
    # the keyword form: the same plan from unflagged descriptors
    p0, _, _ = engine.build_stage2_batch(calls)
    assert _decode(*engine.stage2_plan_raw(p0, qbuf, qucbuf, cross_species=True)[:3]) == batch
    assert _decode(*engine.stage2_plan_raw(p0, qbuf, qucbuf)[:3]) == off


def test_gpu_stage2_flags_validation(engine):
    g, calls = X.chain_calls("short", 60)
    engine.set_genome(g)
    probs, qbuf, qucbuf = engine.build_stage2_batch(calls[:8], cross_species=True)
    mixed = probs.copy()
    mixed["flags"][3] = 0
    unknown = probs.copy()
    unknown["flags"] = 3
    for bad in (mixed, unknown):
        with pytest.raises(gmapdp.GmapdpError, match="flags"):
            engine.stage2_batch_raw(bad, qbuf, qucbuf)
        with pytest.raises(gmapdp.GmapdpError, match="flags"):
            engine.stage2_plan_raw(bad, qbuf, qucbuf)
    engine.stage2_batch_raw(probs, qbuf, qucbuf)
