"""Stage2_compute_one / _ends / _starts on segments of 65 536 and 65 537 query positions (tests/s2long.py), against
the chain oracles byte for byte: the path kernel's three walks -- the LDS link table, the diagonal walk over the
global arrays, the walk on lane 0 alone past 65 536 positions -- with a hit on a path at the first and at the last
query position, the long seeding class (CTX_LONG_QUERIES) as the input of all three kinds, several returned
lists, long and short calls in one batch, a context without the flag, a stranded mode and arenas too small.
tests/test_stage2x_long_inputs.py shows on the CPU that the calls reach these classes."""
import ctypes as C

import numpy as np
import pytest

import gmapdp
import s2long as L
import s2x
from dpbind import Oracle, stage2_mismatches

pytestmark = pytest.mark.gpu

KIND_IDS = {L.ONE: "one", L.ENDS: "ends", L.STARTS: "starts"}
kinds = pytest.mark.parametrize("kind", L.KINDS, ids=[KIND_IDS[k] for k in L.KINDS])
DISTINCT = "query with more than 16384 distinct 8-mers"


@pytest.fixture(scope="module")
def eng():
    e = gmapdp.Engine(0, flags=gmapdp.CTX_LONG_QUERIES)
    e.set_genome(s2x.genome())
    yield e
    e.close()


@pytest.fixture(scope="module")
def _orcs():
    seed = Oracle()
    return seed, {k: L.oracle_for(k, seed) for k in L.KINDS}


@pytest.fixture
def batch_of(_orcs):
    """{kind: the kind's oracle batch(probs, qbuf, qucbuf)} on s2x.genome() (the oracle library's genome is the
    process's: other tests set their own)."""
    _orcs[0].set_genome(s2x.genome())
    return {k: v[1] for k, v in _orcs[1].items()}


def _against_oracle(e, batch, calls, kind):
    probs, qbuf, qucbuf = e.build_stage2x_batch(calls, kind)
    results, paths, pairs = e.stage2x_batch_raw(probs, qbuf, qucbuf)
    exp = batch(probs, qbuf, qucbuf)
    bad = stage2_mismatches(results, paths, pairs, exp)
    assert not bad, bad[:10]
    return results, paths, pairs


@kinds
def test_boundary_calls(eng, batch_of, kind):
    calls, tags = L.boundary_calls(kind)
    before = eng.long_query_calls()
    results, paths, pairs = _against_oracle(eng, batch_of[kind], list(calls), kind)
    assert eng.long_query_calls() - before == sum(t[3] == L.IID for t in tags) == len(calls) // 2
    assert all(int(r["status"]) == 2 and int(r["nresults"]) >= 1 for r in results)
    # a path through the first and one through the last query position, at both lengths
    for ql in L.LENGTHS:
        pos = set()
        for p, t, (n, lists) in zip(calls, tags, s2x.engine_lists(results, paths, pairs)):
            if t[0] == ql:
                pos |= {k[0] - p["query_offset"] for lst in lists for k in lst if not k[9]}
        assert {0, ql - 1} <= pos
    # the periodic fill alone: the seeding's LDS classes, none counted as long
    periodic = [p for p, t in zip(calls, tags) if t[3] == L.PERIODIC]
    before = eng.long_query_calls()
    _against_oracle(eng, batch_of[kind], periodic, kind)
    assert eng.long_query_calls() == before


@pytest.mark.parametrize("kind", (L.ENDS, L.STARTS), ids=("ends", "starts"))
def test_several_lists(eng, batch_of, kind):
    calls = list(L.several_lists_calls(kind))
    results, _, _ = _against_oracle(eng, batch_of[kind], calls, kind)
    assert all(int(r["nresults"]) >= 2 and int(r["npaths"]) > int(r["nresults"]) for r in results)


@kinds
def test_mixed_batch(eng, batch_of, kind):
    calls, tags = L.mixed_batch(kind)
    calls = list(calls)
    together = s2x.engine_lists(*_against_oracle(eng, batch_of[kind], calls, kind))
    assert sum(n >= 1 for (n, _), t in zip(together, tags) if t is None) >= 2
    # (path and pair offsets differ between runs; the lists do not)
    for i, p in enumerate(calls):
        probs, qbuf, qucbuf = eng.build_stage2x_batch([p], kind)
        assert s2x.engine_lists(*eng.stage2x_batch_raw(probs, qbuf, qucbuf)) == [together[i]], i


@kinds
def test_plain_context(batch_of, kind):
    """Without CTX_LONG_QUERIES: the periodic 65 544-nt calls (at most 16 384 distinct 8-mers) run and match; an
    i.i.d.-fill call is refused before any kernel is launched."""
    calls, tags = L.boundary_calls(kind)
    periodic = [p for p, t in zip(calls, tags) if t[0] == 65544 and t[3] == L.PERIODIC]
    iid = [p for p, t in zip(calls, tags) if t[0] == 65544 and t[3] == L.IID][:1]
    assert len(periodic) == 4 and len(iid) == 1
    e = gmapdp.Engine(0)
    try:
        e.set_genome(s2x.genome())
        _against_oracle(e, batch_of[kind], periodic, kind)
        assert e.long_query_calls() == 0
        probs, qbuf, qucbuf = e.build_stage2x_batch(iid, kind)
        results = np.zeros(1, dtype=gmapdp.STAGE2_RESULT_DTYPE)
        paths = np.zeros(64, dtype=gmapdp.PATH_DTYPE)
        pairs = np.zeros(4096, dtype=gmapdp.PATH_PAIR_DTYPE)
        pn, qn = C.c_size_t(), C.c_size_t()
        rc = e.lib.gmapdp_stage2x_batch(e.h, probs.ctypes.data, 1, qbuf, qucbuf, len(qucbuf), results.ctypes.data,
                                        paths.ctypes.data, len(paths), pairs.ctypes.data, len(pairs), C.byref(pn),
                                        C.byref(qn))
        assert (rc, e.lib.gmapdp_last_error(e.h).decode()) == (-1, DISTINCT)   # GMAPDP_EINVAL
    finally:
        e.close()


@kinds
def test_stranded_mode(_orcs, kind):
    """A mode-1 (cmet-stranded) context with the flag: the boundary calls with upper-case queries against the oracle
    on each strand's reduced genome (s2long.stranded_expected)."""
    mode = 1
    g = s2x.genome()
    calls = [dict(p, q=p["quc"]) for p in L.boundary_calls(kind)[0]]
    e = gmapdp.Engine(0, mode=mode, flags=gmapdp.CTX_LONG_QUERIES)
    try:
        e.set_genome(g)
        probs, qbuf, qucbuf = e.build_stage2x_batch(calls, kind)
        results, paths, pairs = e.stage2x_batch_raw(probs, qbuf, qucbuf)
    finally:
        e.close()
    seed, orcs = _orcs
    exp, ncolon, nlists = L.stranded_expected(seed.set_genome, orcs[kind][1], g, mode, probs, qbuf, qucbuf)
    bad = stage2_mismatches(results, paths, pairs, exp)
    assert not bad, bad[:10]
    assert ncolon > 0 and nlists >= len(calls)


@kinds
def test_small_arenas(eng, kind):
    """One 65 544-nt call (the lane-0 walk; ENDS and STARTS: three traced paths, two lists): arenas one record short
    are refused with the need, arenas of exactly the need return the same lists."""
    if kind == L.ONE:
        calls, tags = L.boundary_calls(kind)
        p = calls[tags.index((65544, L.LARGE, 0, L.IID))]
    else:
        p = L.several_lists_calls(kind)[0]
    assert len(p["quc"]) == 65544
    probs, qbuf, qucbuf = eng.build_stage2x_batch([p], kind)
    results, paths, pairs = eng.stage2x_batch_raw(probs, qbuf, qucbuf)
    np_, nq = len(paths), len(pairs)
    assert np_ == (1 if kind == L.ONE else 2) and nq > 1
    assert eng.stage2x_batch_raw(probs, qbuf, qucbuf, path_cap=np_ - 1, pair_cap=nq) == (-6, np_, nq)
    assert eng.stage2x_batch_raw(probs, qbuf, qucbuf, path_cap=np_, pair_cap=nq - 1) == (-6, np_, nq)
    r2, p2, q2 = eng.stage2x_batch_raw(probs, qbuf, qucbuf, path_cap=np_, pair_cap=nq)
    assert s2x.engine_lists(r2, p2, q2) == s2x.engine_lists(results, paths, pairs)
