"""The stage-2 chaining's output pools (s2c_kernel.hip: two atomicAdds per call on the batch's path and pair pools,
in the order the waves finish) where they overflow, fit exactly and miss by one record:

  * the synchronous batches (gmapdp_stage2_batch, gmapdp_stage2x_batch ENDS / STARTS; s2_batch_core), which grow the
    pools and run the chaining again: equal to the oracle after the regrow, and gmapdp_stage2_pool_regrows tells a
    regrown batch from one that fitted;
  * the device-resident plan (gmapdp_stage2_plan_*), whose pools are fixed: a call that does not fit reports
    status -2, every other call equals the oracle, and nothing of an overflowed run -- counters past the
    capacities, reserved but unwritten slots -- reaches the fetch, the compact stream or the next run.

Inputs and their demands: tests/s2pools.py (every demand is the oracle's; tests/test_stage2_pools_inputs.py checks
each against the capacity it is aimed at).  Every comparison is exact: results field by field, pair records byte
for byte (dpbind.stage2_mismatches), or field by field where a call outgrows the oracle's batch format."""
import ctypes as C

import numpy as np
import pytest

import gmapdp
import s2pools as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = gmapdp.Engine(0)
    e.set_genome(P.genome())
    yield e
    e.close()


@pytest.fixture(scope="module")
def xeng():
    e = gmapdp.Engine(0)
    e.set_genome(P.x_genome())
    yield e
    e.close()


def _batch_once(e, c, path_cap, pair_cap):
    """One gmapdp_stage2_batch / gmapdp_stage2x_batch call with host arenas of path_cap / pair_cap records:
    (rc, paths needed, pairs needed, results, paths, pairs)."""
    results = np.zeros(c.n, dtype=gmapdp.STAGE2_RESULT_DTYPE)
    paths = np.zeros(max(path_cap, 1), dtype=gmapdp.PATH_DTYPE)
    pairs = np.zeros(max(pair_cap, 1), dtype=gmapdp.PATH_PAIR_DTYPE)
    pn, qn = C.c_size_t(), C.c_size_t()
    f = e.lib.gmapdp_stage2x_batch if c.kind else e.lib.gmapdp_stage2_batch
    rc = f(e.h, c.probs.ctypes.data, c.n, c.qbuf, c.qucbuf, len(c.qucbuf), results.ctypes.data, paths.ctypes.data,
           path_cap, pairs.ctypes.data, pair_cap, C.byref(pn), C.byref(qn))
    return rc, pn.value, qn.value, results, paths[:path_cap], pairs[:pair_cap]


def _sync(e, c):
    """The case's batch in one call, the host arenas sized by the oracle's demand (a second call would count its
    own regrows): (results, paths, pairs, regrows it took)."""
    before = e.stage2_pool_regrows()
    rc, pn, qn, res, paths, pairs = _batch_once(e, c, c.paths, c.pairs)
    assert (rc, pn, qn) == (0, c.paths, c.pairs), (rc, pn, qn, e.lib.gmapdp_last_error(e.h))
    return res, paths, pairs, e.stage2_pool_regrows() - before


def _check_sync(e, name):
    c = P.case(name)
    res, paths, pairs, regrows = _sync(e, c)
    bad = c.mismatches(res, paths, pairs)
    assert not bad, bad[:8]
    return regrows


# ---------------------------------------------------------------------------------------------------------
# Synchronous batches
# ---------------------------------------------------------------------------------------------------------
def test_gpu_stage2_pools_regrow(eng):
    assert _check_sync(eng, "regrow") >= 1


def _records(out):
    res, paths, pairs = out[:3]
    recs = []
    for r in res:
        for k in range(int(r["nresults"])):
            pr = paths[int(r["path_offset"]) + k]
            o = int(pr["pair_offset"])
            recs.append(pairs[o:o + int(pr["npairs"])].tobytes())
    return recs


def test_gpu_stage2_pools_deep_regrow_leaves_other_batches_alone(eng):
    """`deep` takes two extra attempts at the least (tests/test_stage2_pools_inputs.py); an ordinary batch on the
    same context before and after it fits its first guess, equals the oracle and gives the same records."""
    o = P.case("ordinary")
    before = _sync(eng, o)
    assert before[3] == 0 and not o.mismatches(*before[:3])
    assert _check_sync(eng, "deep") >= 2
    after = _sync(eng, o)
    assert after[3] == 0
    bad = o.mismatches(*after[:3])
    assert not bad, bad[:8]
    # (path_offset / pair_offset follow the order the waves finish; everything else is compared byte for byte)
    for f in ("nresults", "npaths", "ncovered", "status", "diag_querystart", "diag_queryend", "npairs"):
        assert before[0][f].tobytes() == after[0][f].tobytes(), f
    assert _records(before) == _records(after) and len(_records(before)) == o.paths


@pytest.mark.parametrize("name", ["ends_regrow", "starts_regrow"])
def test_gpu_stage2_pools_regrow_ends_starts(xeng, name):
    assert _check_sync(xeng, name) >= 1


def test_gpu_stage2_pools_pair_pool_exact_fit_and_over(eng):
    assert _check_sync(eng, "pair_fit") == 0          # 128 records = 64 + 2 x 32
    assert _check_sync(eng, "pair_copy_over") == 1    # 160
    assert _check_sync(eng, "pair_one_over") == 1     # 195 records = 64 + 2 x 65 + 1


def test_gpu_stage2_pools_path_pool_exact_fit_and_over(eng):
    assert _check_sync(eng, "path_fit") == 0          # 36 path records = 16 + 2 x 10
    assert _check_sync(eng, "path_one_over") == 1     # 37


def test_gpu_stage2_pools_both_path_kernel_launches_share_the_pools(eng):
    """s2c's first launch (the call with more than 4 096 hits) leaves one path record and ~2 000 pair records in
    the pools; the second launch's calls reserve after them and overflow."""
    assert _check_sync(eng, "launches") >= 1


def test_gpu_stage2_pools_caller_arenas_after_a_regrow(eng):
    """The caller's host arenas are checked against the counters of the attempt that fitted: one record short on
    either side is GMAPDP_ESPACE (-6) with the oracle's totals as the sizes needed; the exact sizes succeed."""
    c = P.case("regrow")
    before = eng.stage2_pool_regrows()
    assert _batch_once(eng, c, c.paths - 1, c.pairs)[:3] == (-6, c.paths, c.pairs)
    assert _batch_once(eng, c, c.paths, c.pairs - 1)[:3] == (-6, c.paths, c.pairs)
    rc, pn, qn, res, paths, pairs = _batch_once(eng, c, c.paths, c.pairs)
    assert (rc, pn, qn) == (0, c.paths, c.pairs)
    assert not c.mismatches(res, paths, pairs)
    assert eng.stage2_pool_regrows() - before >= 3   # each of the three calls regrew


# ---------------------------------------------------------------------------------------------------------
# The plan
# ---------------------------------------------------------------------------------------------------------
def _ranges_disjoint(ranges, limit):
    """[lo, hi) ranges lie within [0, limit) and do not overlap."""
    end = 0
    for lo, hi in sorted(r for r in ranges if r[1] > r[0]):
        if lo < end or hi > limit:
            return False
        end = hi
    return True


def _check_plan(c, res, paths, pairs, path_cap, pair_cap):
    """What holds of a plan run whatever overflowed; returns the calls with status -2."""
    assert len(paths) <= path_cap and len(pairs) <= pair_cap    # paths_needed / pairs_needed of the fetch
    over = [i for i in range(c.n) if int(res[i]["status"]) == -2]
    bad = c.mismatches(res, paths, pairs, skip=over)
    assert not bad, bad[:8]
    kept = [i for i in range(c.n) if i not in over]
    owned = [(int(res[i]["path_offset"]), int(res[i]["path_offset"]) + int(res[i]["nresults"])) for i in kept]
    assert _ranges_disjoint(owned, len(paths)), owned
    slots = sorted(k for lo, hi in owned for k in range(lo, hi))
    lists = [(int(paths[k]["pair_offset"]), int(paths[k]["pair_offset"]) + int(paths[k]["npairs"])) for k in slots]
    assert _ranges_disjoint(lists, len(pairs)), lists
    # the other slots of the pool (a status -2 call's): an empty record, or a list the call wrote before its pair
    # reservation failed -- within the pool and apart from every other list (include/gmapdp.h)
    others = [(int(p["pair_offset"]), int(p["pair_offset"]) + int(p["npairs"]))
              for k, p in enumerate(paths) if not any(lo <= k < hi for lo, hi in owned)]
    assert all(hi >= lo >= 0 for lo, hi in others), others
    assert all(lo == 0 for lo, hi in others if hi == lo), others
    assert _ranges_disjoint(lists + others, len(pairs)), others
    return over


@pytest.mark.parametrize("reruns", [0, 2])
def test_gpu_stage2_pools_plan_overflow_is_reported_and_contained(eng, reruns):
    """76 path records against 64 and 3 480 pair records against 2 824: which calls overflow depends on the order
    of the waves, so only what must hold is asserted.  At least one call reports -2 (the demand exceeds the
    pools).  At least one does not: the first path reservation fits, and a pair reservation can fail only once more
    than capacity - 150 records are reserved (150: the longest list here); the calls that passed the path check
    hold at most 64 path slots, so at most seven of them have nine lists of 40, and as long as none of them has
    all its lists they hold at most 7 x (360 - 40) records, which is less."""
    c = P.case("plan_overflow")
    pcap, qcap = P.plan_path_cap(c.n), P.plan_pair_cap(c.qsum)
    assert c.paths > pcap and c.pairs > qcap
    assert sorted(set(c.nresults)) == [1, 9] and max(len(x["quc"]) for x in c.calls) == 150
    assert 7 * 9 <= pcap < 8 * 9 and 7 * (360 - 40) <= qcap - 150
    res, paths, pairs, _ = eng.stage2_plan_raw(c.probs, c.qbuf, c.qucbuf, reruns=reruns)
    over = _check_plan(c, res, paths, pairs, pcap, qcap)
    assert 1 <= len(over) < c.n, over


@pytest.mark.parametrize("fit,one_over", [("plan_path_fit", "plan_path_one_over"),
                                          ("plan_pair_fit", "plan_pair_one_over")])
def test_gpu_stage2_pools_plan_exact_fit_and_one_over(eng, fit, one_over):
    c = P.case(fit)
    pcap, qcap = P.plan_path_cap(c.n), P.plan_pair_cap(c.qsum)
    assert c.paths == pcap or c.pairs == qcap
    res, paths, pairs, _ = eng.stage2_plan_raw(c.probs, c.qbuf, c.qucbuf)
    assert _check_plan(c, res, paths, pairs, pcap, qcap) == []
    assert (len(paths), len(pairs)) == (c.paths, c.pairs)
    c = P.case(one_over)
    pcap, qcap = P.plan_path_cap(c.n), P.plan_pair_cap(c.qsum)
    assert c.paths == pcap + 1 or c.pairs == qcap + 1
    res, paths, pairs, _ = eng.stage2_plan_raw(c.probs, c.qbuf, c.qucbuf)
    assert len(_check_plan(c, res, paths, pairs, pcap, qcap)) >= 1


def test_gpu_stage2_pools_plan_nothing_stale_survives(eng):
    """One plan, run on the arena that overflows its pools and then on an arena of the same layout that fits (one
    result per call): the second run equals the oracle on its arena, no call reports -2."""
    c = P.case("plan_overflow")
    a = P.alt_case("plan_overflow")
    pcap, qcap = P.plan_path_cap(c.n), P.plan_pair_cap(c.qsum)
    res, paths, pairs, _ = eng.stage2_plan_raw(c.probs, c.qbuf, c.qucbuf, run_qbuf=a.qbuf, run_qucbuf=a.qucbuf,
                                               prior_runs=[(c.qbuf, c.qucbuf)])
    assert _check_plan(a, res, paths, pairs, pcap, qcap) == []
    assert (len(paths), len(pairs)) == (a.paths, a.pairs)


@pytest.mark.parametrize("reruns", [0, 2])
def test_gpu_stage2_pools_plan_compact_stream_over_an_overflowed_pool(eng, reruns):
    """The compact stream counts its lists from the device counter, which an overflow leaves past the pool's size,
    and reads every path record below it, written or not: the stream stays within its bound, and every list of a
    call that did not overflow expands to the fetched records."""
    c = P.case("plan_overflow")
    pcap, qcap = P.plan_path_cap(c.n), P.plan_pair_cap(c.qsum)
    co = {}
    res, paths, pairs, _ = eng.stage2_plan_raw(c.probs, c.qbuf, c.qucbuf, compact_out=co, reruns=reruns)
    over = _check_plan(c, res, paths, pairs, pcap, qcap)
    assert over
    assert co["bound"] == 21 * qcap + 64 and co["bytes"] <= co["bound"]
    assert co["bytes"] <= 21 * len(pairs)     # (no list is counted twice)
    nlists = 0
    for i in range(c.n):
        if i in over:
            continue
        for k in range(int(res[i]["nresults"])):
            pr = paths[int(res[i]["path_offset"]) + k]
            o, m = int(pr["pair_offset"]), int(pr["npairs"])
            assert co["pairs"][o:o + m].tobytes() == pairs[o:o + m].tobytes(), (i, k)
            nlists += 1
    assert nlists >= 1
