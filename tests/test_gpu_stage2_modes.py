"""Stage 2 on the engine in GMAP's stranded cmet / atoi / ttoc modes (contexts created with mode 1, 3, 5).

Seeding: Oligoindex_hr_tally reduces the window's genome words before it extracts 8-mers, so the engine in
mode M on the genome G must equal the oracle (STANDARD) on the reduced genome G' of the call's strand:
npositions, the positions of every query position in order (mappings and table slices), totalpositions,
maxnconsecutive, oned_matrix_p and the diagonals, through every seeding path -- the split kernels
(gmapdp_oligo_mappings_batch), their global fallbacks, the seeding plan (oi_kernel + oi_map_kernel, both
counter classes) and the stage-2 plan's sizing and run kernels.  Stage2_compute: the oracle on G' with the
pair characters rewritten as convert_to_nucleotides does outside STANDARD (tests/s2modes.py), through the
synchronous batch, the stage-2 plan (what = 3, and 1 then 4, 8, 16) and the compact pair stream.  A mode-0
context on the same inputs still equals the oracle on G; tests/test_stage2_modes_power.py shows that the two
expectations differ.  The non-stranded modes (2, 4, 6), which GMAP itself refuses, are GMAPDP_EINVAL on all
four stage-2 entry points and still run the DP family."""
import ctypes as C
import random

import numpy as np
import pytest

import gmapdp
import s2modes
from dpbind import Oracle, random_genome, single_gap_problem, stage2_mismatches
from test_gpu_seeding_order import _oligo_plan_raw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def engines():
    es = {m: gmapdp.Engine(0, mode=m) for m in (0,) + s2modes.MODES}
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def seeding(oracle):
    """The seeding inputs of every mode and their expected values (mode 0: the same calls on G)."""
    g = s2modes.seeding_genome()
    out = {}
    for m in s2modes.MODES:
        calls = s2modes.seeding_calls(g, m)
        out[m] = (calls, s2modes.seeding_expected(oracle, g, m, calls), s2modes.seeding_expected(oracle, g, 0, calls))
    return g, out


def _same(got, exp, what):
    assert len(got) == len(exp)
    for i, (a, b) in enumerate(zip(got, exp)):
        assert a == b, "%s, call %d: %s vs oracle %s" % (what, i, a[0], b[0])


@pytest.mark.parametrize("mode", s2modes.MODES)
def test_gpu_seeding_in_mode_equals_oracle_on_reduced_genome(engines, seeding, mode):
    g, cases = seeding
    calls, exp, std = cases[mode]
    eng = engines[mode]
    eng.set_genome(g)
    _same(eng.oligo_mappings_batch(calls), exp, "split seeding, mode %d" % mode)
    _same([x[0] for x in _oligo_plan_raw(eng, calls)], exp, "seeding plan, mode %d" % mode)
    # the STANDARD context on the same inputs: the oracle on G, as before
    engines[0].set_genome(g)
    _same(engines[0].oligo_mappings_batch(calls), std, "split seeding, mode 0")
    _same([x[0] for x in _oligo_plan_raw(engines[0], calls)], std, "seeding plan, mode 0")


@pytest.mark.parametrize("mode", s2modes.MODES)
def test_gpu_seeding_in_mode_global_fallbacks(engines, seeding, mode, monkeypatch):
    """oi_build_kernel with its table image and candidates kept out of LDS (the global event sort), and with a
    small event pool besides (the sequential walk): the calls over the homopolymer stretch and a few more."""
    g, cases = seeding
    calls, exp, _ = cases[mode]
    eng = engines[mode]
    eng.set_genome(g)
    monkeypatch.setenv("GMAPDP_OI_LDS_TABLE", "0")
    _same(eng.oligo_mappings_batch(calls[:12]), exp[:12], "split seeding without the LDS table, mode %d" % mode)
    monkeypatch.setenv("GMAPDP_OLIGO_POOL_SLOTS", "64")
    _same(eng.oligo_mappings_batch(calls[:12]), exp[:12], "split seeding, sequential walk, mode %d" % mode)
    _same([x[0] for x in _oligo_plan_raw(eng, calls[:12])], exp[:12], "seeding plan, sequential walk, mode %d" % mode)


def _dbuf(hip, bufs, nbytes, src=None):
    ptr = C.c_void_p()
    if hip.hipMalloc(C.byref(ptr), max(nbytes, 16)) != 0:
        raise gmapdp.GmapdpError("hipMalloc(%d) failed" % nbytes)
    bufs.append(ptr)
    if src is not None and hip.hipMemcpy(ptr, src, nbytes, 1) != 0:  # hipMemcpyHostToDevice
        raise gmapdp.GmapdpError("hipMemcpy failed")
    return ptr


def _stage2_plan_in_steps(eng, probs, qb, qub):
    """A stage-2 plan run as what = 1, then 4, 8, 16 on the context's stream: (seeding results after the
    first step, results, paths, pairs)."""
    lib, hip, n = eng.lib, gmapdp._hip(), len(probs)
    plan = C.c_void_p()
    eng._check(lib.gmapdp_stage2_plan_create(eng.h, probs.ctypes.data, n, qb, qub, len(qub), C.byref(plan)),
               "gmapdp_stage2_plan_create")
    bufs = []
    try:
        d_q, d_quc = _dbuf(hip, bufs, len(qb), qb), _dbuf(hip, bufs, len(qub), qub)
        d_res = _dbuf(hip, bufs, n * gmapdp.STAGE2_RESULT_DTYPE.itemsize)
        eng._check(lib.gmapdp_stage2_plan_run(eng.h, plan, d_q, d_quc, d_res, 1, None), "gmapdp_stage2_plan_run(1)")
        ores = np.zeros(n, dtype=gmapdp.OLIGO_RESULT_DTYPE)
        eng._check(lib.gmapdp_stage2_plan_seeding_results(eng.h, plan, None, ores.ctypes.data),
                   "gmapdp_stage2_plan_seeding_results")
        for what in (4, 8, 16):
            eng._check(lib.gmapdp_stage2_plan_run(eng.h, plan, d_q, d_quc, d_res, what, None),
                       "gmapdp_stage2_plan_run(%d)" % what)
        results = np.zeros(n, dtype=gmapdp.STAGE2_RESULT_DTYPE)
        pn, qn = C.c_size_t(), C.c_size_t()
        rc = lib.gmapdp_stage2_plan_fetch(eng.h, plan, d_res, None, results.ctypes.data, None, 0, None, 0,
                                          C.byref(pn), C.byref(qn))
        if rc not in (0, -6):
            eng._check(rc, "gmapdp_stage2_plan_fetch")
        paths = np.zeros(max(pn.value, 1), dtype=gmapdp.PATH_DTYPE)
        pairs = np.zeros(max(qn.value, 1), dtype=gmapdp.PATH_PAIR_DTYPE)
        eng._check(lib.gmapdp_stage2_plan_fetch(eng.h, plan, d_res, None, results.ctypes.data, paths.ctypes.data,
                                                len(paths), pairs.ctypes.data, len(pairs), C.byref(pn), C.byref(qn)),
                   "gmapdp_stage2_plan_fetch")
        return ores, results, paths[:pn.value], pairs[:qn.value]
    finally:
        for b in bufs:
            hip.hipFree(b)
        lib.gmapdp_stage2_plan_destroy(plan)


def _check_stage2(eng, probs, qb, qub, exp, seed_exp, what):
    res, paths, pairs = eng.stage2_batch_raw(probs, qb, qub)
    bad = stage2_mismatches(res, paths, pairs, exp)
    assert not bad, (what, "batch", bad[:8])
    compact = {}
    res, paths, pairs, _ = eng.stage2_plan_raw(probs, qb, qub, compact_out=compact)
    bad = stage2_mismatches(res, paths, pairs, exp)
    assert not bad, (what, "plan", bad[:8])
    # the compact stream expanded back: the same records (it carries ':' as it carries '|')
    assert compact["bytes"] <= compact["bound"]
    bad = stage2_mismatches(res, paths, compact["pairs"], exp)
    assert not bad, (what, "compact stream", bad[:8])
    ores, res, paths, pairs = _stage2_plan_in_steps(eng, probs, qb, qub)
    bad = stage2_mismatches(res, paths, pairs, exp)
    assert not bad, (what, "plan in steps", bad[:8])
    got = [(int(r["totalpositions"]), int(r["maxnconsecutive"]), int(r["oned_matrix_p"]), int(r["ndiagonals"]))
           for r in ores]
    assert got == [e[0] for e in seed_exp], (what, "stage-2 plan seeding results")


@pytest.mark.parametrize("mode", s2modes.MODES)
def test_gpu_stage2_in_mode_equals_rewritten_oracle_on_reduced_genome(engines, oracle, mode):
    g = s2modes.stage2_genome(mode)
    calls = s2modes.stage2_calls(g, mode)
    probs, qb, qub = gmapdp.Engine.build_stage2_batch(calls)
    exp, nrec, ncolon = s2modes.stage2_expected(oracle, g, mode, probs, qb, qub)
    assert np.all(exp[0][:, 0] >= 0) and 4 * ncolon >= nrec > 0
    major = [dict(c, minor=0) for c in calls]
    seed_exp = s2modes.seeding_expected(oracle, g, mode, major)
    eng = engines[mode]
    eng.set_genome(g)
    _check_stage2(eng, probs, qb, qub, exp, seed_exp, "mode %d" % mode)
    # the two 70-kb windows: the seeding plan's 32-bit counter class
    wide = [c for c in major if c["chrend"] - c["chrstart"] >= 65536 + 8]
    assert len(wide) == 2 and {c["plusp"] for c in wide} == {0, 1}
    _same([x[0] for x in _oligo_plan_raw(eng, wide)], [seed_exp[major.index(c)] for c in wide],
          "seeding plan, 32-bit counters, mode %d" % mode)
    # the STANDARD context on the same inputs: the oracle on G, byte for byte as before
    std, _, _ = s2modes.stage2_expected(oracle, g, 0, probs, qb, qub)
    engines[0].set_genome(g)
    _check_stage2(engines[0], probs, qb, qub, std, s2modes.seeding_expected(oracle, g, 0, major), "mode 0")


@pytest.mark.parametrize("mode", [2, 4, 6])
def test_gpu_stage2_non_stranded_modes_are_einval(mode):
    """Every stage-2 entry point refuses a non-stranded context (GMAPDP_EINVAL, -1, through the binding's
    exception) instead of answering with STANDARD semantics; the same context still runs a single-gap batch."""
    rng = random.Random(mode)
    g = random_genome(rng, 20000, nfrac=0)
    eng = gmapdp.Engine(0, mode=mode)
    try:
        eng.set_genome(g)
        q = g[3000:3200]
        call = dict(q=q, quc=q, chrstart=2000, chrend=5000, chroffset=0, chrhigh=len(g) - 1, plusp=1, minor=0,
                    splicingp=1, maxintronlen=500000)
        probs, qb, qub = gmapdp.Engine.build_stage2_batch([call])
        for f in (lambda: eng.oligo_mappings_batch([call]), lambda: _oligo_plan_raw(eng, [call]),
                  lambda: eng.stage2_batch_raw(probs, qb, qub), lambda: eng.stage2_plan_raw(probs, qb, qub)):
            with pytest.raises(gmapdp.GmapdpError, match=r"failed \(-1\).*non-stranded"):
                f()
        probs1 = [single_gap_problem(rng, g) for _ in range(16)]
        got = eng.single_gap_batch(probs1)
        assert len(got) == 16 and all(x is not None for x in got)
    finally:
        eng.close()


def test_gpu_stage2_plan_runs_only_in_its_mode(engines):
    """A plan's seeding descriptors carry its context's reductions: run on a context of another mode it is
    refused (GMAPDP_EINVAL) before anything is launched."""
    g = s2modes.stage2_genome(1)
    calls = s2modes.stage2_calls(g, 1, n=2)
    probs, qb, qub = gmapdp.Engine.build_stage2_batch(calls)
    maker, other = engines[1], engines[0]
    maker.set_genome(g)
    other.set_genome(g)
    lib, hip, n = maker.lib, gmapdp._hip(), len(probs)
    plan = C.c_void_p()
    maker._check(lib.gmapdp_stage2_plan_create(maker.h, probs.ctypes.data, n, qb, qub, len(qub), C.byref(plan)),
                 "gmapdp_stage2_plan_create")
    bufs = []
    try:
        d_q, d_quc = _dbuf(hip, bufs, len(qb), qb), _dbuf(hip, bufs, len(qub), qub)
        d_res = _dbuf(hip, bufs, n * gmapdp.STAGE2_RESULT_DTYPE.itemsize)
        for what in (1, 2, 3, 16):
            assert lib.gmapdp_stage2_plan_run(other.h, plan, d_q, d_quc, d_res, what, None) == -1
            assert b"another mode" in lib.gmapdp_last_error(other.h)
        assert lib.gmapdp_stage2_plan_run(maker.h, plan, d_q, d_quc, d_res, 3, None) == 0
        assert hip.hipDeviceSynchronize() == 0
    finally:
        for b in bufs:
            hip.hipFree(b)
        lib.gmapdp_stage2_plan_destroy(plan)
