"""Stage 2 on queries with more than 16 384 distinct 8-mers (the seeding's long launch class) in a context
created with CTX_LONG_QUERIES, against the oracle bit for bit, every output field.  The calls come from
tests/longq.py (cases A-H of the class's test plan); tests/test_long_query_oracle.py pins the oracle to the
reference on the same calls."""
import random

import numpy as np
import pytest

import gmapdp
import longq
import s2modes
from dpbind import Oracle, oracle_stage2_batch, stage2_mismatches
from scanref import ncovered_from_diagonals

pytestmark = pytest.mark.gpu

DISTINCT = "query with more than 16384 distinct 8-mers"


@pytest.fixture(scope="module")
def world():
    g = longq.genome()
    orc = Oracle()
    orc.set_genome(g)
    return dict(g=g, orc=orc)


@pytest.fixture(scope="module")
def engine(world):
    e = gmapdp.Engine(0, flags=gmapdp.CTX_LONG_QUERIES)
    e.set_genome(world["g"])
    yield e
    e.close()


def _seed_batch(engine, calls):
    """gmapdp_oligo_mappings_batch in the oracle's format."""
    probs, qucbuf = gmapdp.Engine.build_oligo_batch(calls)
    return engine._decode_oligo(probs, *engine.oligo_mappings_batch_raw(probs, qucbuf), relative=False)


def _first_diff(got, exp):
    for i, (a, b) in enumerate(zip(got, exp)):
        if a != b:
            what = [k for k, (x, y) in enumerate(zip(a, b)) if x != y]
            return "call %d: fields %s differ (scalars gpu %s, oracle %s)" % (i, what, a[0], b[0])
    return None if len(got) == len(exp) else "lengths"


def _scan_expected(seeds, calls):
    return np.array([(ncovered_from_diagonals(s[3], len(c["quc"])), 1, s[0][0], s[0][1]) for s, c in zip(seeds, calls)],
                    dtype=np.int32)


def _scan_calls(calls):
    return [{k: v for k, v in c.items() if k != "minor"} for c in calls]


def _stage2_check(engine, orc, calls):
    sp, qbuf, qucbuf = gmapdp.Engine.build_stage2_batch(calls)
    exp = oracle_stage2_batch(orc, sp, qbuf, qucbuf)
    res, paths, pairs = engine.stage2_batch_raw(sp, qbuf, qucbuf)
    assert stage2_mismatches(res, paths, pairs, exp) == []
    return sp, qbuf, qucbuf, exp, res


# ---- A: the id boundaries ----
@pytest.mark.parametrize("n", longq.BOUNDARY_N)
def test_id_boundaries(engine, world, n):
    """De Bruijn prefixes with exactly n distinct 8-mers, 5 000- and 70 000-nt windows, both strands, both
    indexes: the synchronous batch and the seeding plan."""
    calls = [c for m, c in longq.boundary_calls() if m == n]
    assert len(calls) == 8
    exp = [world["orc"].oligo_mappings(c) for c in calls]
    assert all(len(e) == 4 for e in exp)
    before = engine.long_query_calls()
    d = _first_diff(_seed_batch(engine, calls), exp)
    assert d is None, d
    assert engine.long_query_calls() - before == (8 if n > 16384 else 0)
    d = _first_diff(engine.oligo_plan_batch(calls), exp)
    assert d is None, d


def test_class_boundary_in_a_stage2_plan(engine, world):
    """16 384 distinct 8-mers still take the LDS classes (a 5 000-nt window: the 16-bit one); 16 385 take the long
    class, which gmapdp_stage2_plan_seeding_classes counts with n32."""
    for n, classes, longs in ((16384, (1, 0), 0), (16385, (0, 1), 1)):
        c = longq.call(longq.prefix(n), 20000, 25000, 1)
        sp, qbuf, qucbuf = gmapdp.Engine.build_stage2_batch([c])
        before = engine.long_query_calls()
        res, paths, pairs, got = engine.stage2_plan_raw(sp, qbuf, qucbuf)
        assert got == classes, n
        assert engine.long_query_calls() - before == longs
        assert stage2_mismatches(res, paths, pairs, oracle_stage2_batch(world["orc"], sp, qbuf, qucbuf)) == []


# ---- B: spliced long reads through the five entry points ----
def test_spliced_reads_every_entry_point(engine, world):
    orc = world["orc"]
    calls = [c for c, _ in longq.spliced_calls(world["g"])]
    seeds = [orc.oligo_mappings(c) for c in calls]
    sp, qbuf, qucbuf, exp, res = _stage2_check(engine, orc, calls)          # gmapdp_stage2_batch
    assert (res["status"] == 2).all()
    pres, ppaths, ppairs, classes = engine.stage2_plan_raw(sp, qbuf, qucbuf)  # the plan, its run and _fetch
    assert classes == (0, len(calls))
    assert stage2_mismatches(pres, ppaths, ppairs, exp) == []
    scan = engine.stage2_scan_batch(_scan_calls(calls))                      # the scan batch
    assert np.array_equal(scan, _scan_expected(seeds, calls))
    with engine.scan_plan(*gmapdp.Engine.build_scan_batch(_scan_calls(calls))) as plan:
        plan.run()
        assert np.array_equal(plan.results(), scan)
    d = _first_diff(_seed_batch(engine, calls), seeds)                       # the seeding batch
    assert d is None, d
    d = _first_diff(engine.oligo_plan_batch(calls), seeds)                   # the seeding plan
    assert d is None, d
    # the five agree with each other (test_gpu_scan.py, check 8)
    assert np.array_equal(scan[:, 0], res["ncovered"]) and np.array_equal(scan[:, 0], pres["ncovered"])


# ---- C: GMAP's allocation bound ----
def test_100k_query(engine, world):
    c = longq.random_call()
    seed = world["orc"].oligo_mappings(c)
    assert len(seed) == 4
    d = _first_diff(_seed_batch(engine, [c]), [seed])
    assert d is None, d
    assert np.array_equal(engine.stage2_scan_batch(_scan_calls([c])), _scan_expected([seed], [c]))


# ---- D: Count_T wraps on a high id ----
def test_count_wrap(engine, world):
    calls = longq.wrap_calls(world["g"])
    seeds = [world["orc"].oligo_mappings(c) for c in calls]
    # (that a count passes 255 on an id of the last quarter: test_long_query_oracle.py, on the same calls)
    d = _first_diff(_seed_batch(engine, calls), seeds)
    assert d is None, d
    d = _first_diff(engine.oligo_plan_batch(calls), seeds)
    assert d is None, d
    _stage2_check(engine, world["orc"], calls)


# ---- E: short and long problems in one synchronous call ----
def test_mixed_batch(engine, world):
    calls = longq.mixed_calls(world["g"])
    assert [longq.distinct_8mers(c["quc"]) > 16384 for c in calls] == [False, True, False, True]
    alone = [_seed_batch(engine, [c])[0] for c in calls]
    assert _seed_batch(engine, calls) == alone
    assert alone == [world["orc"].oligo_mappings(c) for c in calls]
    scan = engine.stage2_scan_batch(_scan_calls(calls))
    for i, c in enumerate(calls):
        assert np.array_equal(engine.stage2_scan_batch(_scan_calls([c]))[0], scan[i]), i
    sp, qbuf, qucbuf, exp, res = _stage2_check(engine, world["orc"], calls)
    for i, c in enumerate(calls):
        sp1, q1, qu1 = gmapdp.Engine.build_stage2_batch([c])
        r1, pa1, pr1 = engine.stage2_batch_raw(sp1, q1, qu1)
        assert stage2_mismatches(r1, pa1, pr1, exp, index=[i]) == [], i


# ---- F: more than 2^18 window starts (the 8-byte hit record) ----
def test_wide_window(engine, world):
    c = longq.wide_call(world["g"])
    assert c["chrend"] - c["chrstart"] > 1 << 18
    seed = world["orc"].oligo_mappings(c)
    d = _first_diff(_seed_batch(engine, [c]), [seed])
    assert d is None, d
    d = _first_diff(engine.oligo_plan_batch([c]), [seed])
    assert d is None, d
    assert np.array_equal(engine.stage2_scan_batch(_scan_calls([c])), _scan_expected([seed], [c]))


# ---- G: a stranded mode ----
def test_cmet_stranded(world):
    g = world["g"]
    calls = [c for c, _ in longq.spliced_calls(g)][:2]
    orc = world["orc"]
    try:
        exp = s2modes.seeding_expected(orc, g, 1, calls)
        plain = s2modes.seeding_expected(orc, g, 0, calls)
    finally:
        orc.set_genome(g)
    assert all(a != b for a, b in zip(exp, plain))  # a mode-blind kernel fails
    eng = gmapdp.Engine(0, mode=1, flags=gmapdp.CTX_LONG_QUERIES)
    try:
        eng.set_genome(g)
        d = _first_diff(_seed_batch(eng, calls), exp)
        assert d is None, d
        d = _first_diff(eng.oligo_plan_batch(calls), exp)
        assert d is None, d
    finally:
        eng.close()


# ---- H: the refusal stays where the flag is not given ----
def test_flag_lifts_the_refusal_only_where_given(engine):
    import test_gpu_seeding_refusals as R
    plain = gmapdp.Engine(0)
    try:
        plain.set_genome(R.random_genome(random.Random(4712), R.GENOME_NT))
        for entry in R.ALL:
            assert entry(plain, [R.BAD_DISTINCT]) == (R.EINVAL, DISTINCT), entry.__name__
    finally:
        plain.close()
    flagged = gmapdp.Engine(0, flags=gmapdp.CTX_LONG_QUERIES)
    try:
        flagged.set_genome(R.random_genome(random.Random(4712), R.GENOME_NT))
        for entry in R.ALL:
            assert entry(flagged, [R.BAD_DISTINCT]) == (0, ""), entry.__name__
        assert flagged.long_query_calls() == len(R.ALL)
        # the other refusals keep their words and their order under the flag
        assert R._oligo_plan(flagged, [R.BAD_WINDOW, R.BAD_DISTINCT]) == (R.EINVAL, R.WINDOW)
        assert R._oligo_plan(flagged, [R.BAD_DISTINCT, R.BAD_SLICE]) == (R.EINVAL, R.SLICE)
    finally:
        flagged.close()
