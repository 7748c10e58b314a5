"""Stage2_compute_one / Stage2_compute_ends on the engine (gmapdp_stage2x_batch): bit-exact against the
goldens of the reference's own functions (tests/golden/stage2x_golden.npz), against the CPU oracle
(tests/s2xoracle) on the edge shapes and a few hundred random calls per kind, in a stranded-mode context,
with arenas too small, on every refusal the header lists, and beside gmapdp_stage2_batch on one context."""
import ctypes as C

import numpy as np
import pytest

import gmapdp
import s2modes
import s2x
from dpbind import stage2_mismatches, stage2_problem, repeat_genome

pytestmark = pytest.mark.gpu
KINDS = (s2x.ONE, s2x.ENDS)


@pytest.fixture(scope="module")
def eng():
    e = gmapdp.Engine(0)
    e.set_genome(s2x.genome())
    yield e
    e.close()


@pytest.fixture(scope="module")
def _orc():
    return s2x.S2XOracle()


@pytest.fixture
def orc(_orc):
    _orc.set_genome(s2x.genome())  # (the oracle library's genome is the process's: other tests set their own)
    return _orc


def _strip(lists):
    """The oracle's / golden's pair keys without dynprogindex (the engine's records carry none)."""
    return [[(x[0], x[1], x[2], x[3], 0, x[5], x[6], x[7], x[8], x[9]) for x in lst] for lst in lists]


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_stage2x_goldens_bit_exact(eng, kind):
    g, calls, expected, _ = s2x.golden()
    assert g == s2x.genome()
    idx = s2x.by_kind(calls)[kind]
    assert len(idx) >= 60
    got = eng.stage2x_batch([calls[i] for i in idx], kind)
    bad = [i for i, r in zip(idx, got) if (r[0], r[1]) != (expected[i][0], _strip(expected[i][1]))]
    assert not bad, "calls %s differ from the reference's lists" % bad[:10]


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_stage2x_edge_shapes(eng, orc, kind):
    calls = s2x.edge_calls(kind)
    probs, qbuf, qucbuf = eng.build_stage2x_batch(calls, kind)
    results, paths, pairs = eng.stage2x_batch_raw(probs, qbuf, qucbuf)
    exp = orc.batch(kind, probs, qbuf, qucbuf, nthreads=4)
    assert not stage2_mismatches(results, paths, pairs, exp)
    # what the shapes are there for, by the oracle: status 0 and 2, one hit, 99 / 100 hits, ties, offsets
    assert {int(s) for s in exp[0][:, 3]} == {0, 2} and {int(s) for s in results["status"]} == {0, 2}
    cnt = [orc.counters(p) for p in calls]
    assert any(c["big_position"] for c in cnt) and any(c["tied_cells"] for c in cnt)
    ql = [len(p["quc"]) for p in calls]
    assert {9, 10, 64} <= set(ql)
    assert any(p["chrend"] == p["chrstart"] for p in calls) and any(p["chrend"] + 1 == p["chrstart"] for p in calls)
    for r, p in zip(results, calls):
        if int(r["status"]) == 2:
            assert (int(r["diag_querystart"]), int(r["diag_queryend"])) == (0, len(p["quc"]) - 1)
    if kind == s2x.ENDS:
        assert all(c["restart"] >= 1 for c, r in zip(cnt, results) if int(r["status"]) == 2)
        assert max(int(r["nresults"]) for r in results) >= 2
    else:
        assert max(int(r["nresults"]) for r in results) == 1


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_stage2x_random_calls_against_oracle(eng, orc, kind):
    calls = s2x.random_calls(kind, 300, seed=11)
    probs, qbuf, qucbuf = eng.build_stage2x_batch(calls, kind)
    results, paths, pairs = eng.stage2x_batch_raw(probs, qbuf, qucbuf)
    exp = orc.batch(kind, probs, qbuf, qucbuf)
    bad = stage2_mismatches(results, paths, pairs, exp)
    assert not bad, bad[:10]
    assert int((exp[0][:, 0] > 0).sum()) > 150


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_stage2x_stranded_mode(kind):
    """A mode-1 (cmet-stranded) context: the oracle on the reduced genome of each call's strand, the pair
    characters rewritten from the real genome as convert_to_nucleotides does outside STANDARD."""
    mode = 1
    g = s2x.genome()
    # (upper-case queries, as in tests/s2modes.py: the observed pair of an oligomer is compared with the query as
    # given, the fill pairs with queryuc, and the rewrite below takes queryuc for both)
    calls = [dict(p, q=p["quc"]) for p in s2x.random_calls(kind, 60, seed=23)]
    e = gmapdp.Engine(0, mode=mode)
    try:
        e.set_genome(g)
        probs, qbuf, qucbuf = e.build_stage2x_batch(calls, kind)
        results, paths, pairs = e.stage2x_batch_raw(probs, qbuf, qucbuf)
    finally:
        e.close()
    o = s2x.S2XOracle()
    scal = opaths = opairs = pair_off = None
    for plusp in (1, 0):
        o.set_genome(s2modes.reduced_genome(g, mode, plusp))
        s, pa, pr, po = o.batch(kind, probs, qbuf, qucbuf, nthreads=4)
        if scal is None:
            scal, opaths, opairs, pair_off = s.copy(), pa.copy(), pr.copy(), po
        for i in np.nonzero(probs["plusp"] == plusp)[0]:
            scal[i], opaths[i] = s[i], pa[i]
            opairs[20 * int(po[i]):20 * int(po[i + 1])] = pr[20 * int(po[i]):20 * int(po[i + 1])]
    gv = np.frombuffer(g, dtype=np.uint8)
    comp = np.frombuffer(s2modes.COMP, dtype=np.uint8)
    quc = np.frombuffer(qucbuf, dtype=np.uint8)
    rec = opairs[:20 * int(pair_off[-1])].view(gmapdp.PATH_PAIR_DTYPE)
    raw = opairs[:20 * int(pair_off[-1])].reshape(-1, 20)
    ncolon = 0
    for i in range(len(probs)):
        p = probs[i]
        for k in range(max(int(scal[i, 0]), 0)):
            a = int(pair_off[i]) + int(opaths[i, k, 0])
            r = rec[a:a + int(opaths[i, k, 1])]
            real = np.nonzero(~((r["querypos"] == -1) & (r["genomepos"] == -1)))[0]
            gp = r["genomepos"][real].astype(np.int64)
            c = gv[int(p["chroffset"]) + gp] if int(p["plusp"]) else comp[gv[int(p["chrhigh"]) - gp]]
            qc = quc[int(p["qoff"]) + r["querypos"][real] - int(p["query_offset"])]
            mark = np.where(qc == c, ord("|"), ord(":")).astype(np.uint8)
            raw[a + real, 17] = mark
            raw[a + real, 18] = c
            raw[a + real, 19] = c
            ncolon += int(np.count_nonzero(mark == ord(":")))
    bad = stage2_mismatches(results, paths, pairs, (scal, opaths, opairs, pair_off))
    assert not bad, bad[:10]
    assert ncolon > 0


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_stage2x_small_arenas(eng, kind):
    calls = s2x.random_calls(kind, 40, seed=31)
    probs, qbuf, qucbuf = eng.build_stage2x_batch(calls, kind)
    results, paths, pairs = eng.stage2x_batch_raw(probs, qbuf, qucbuf)
    np_, nq = len(paths), len(pairs)
    assert np_ > 1 and nq > 1
    assert eng.stage2x_batch_raw(probs, qbuf, qucbuf, path_cap=np_ - 1, pair_cap=nq) == (-6, np_, nq)
    assert eng.stage2x_batch_raw(probs, qbuf, qucbuf, path_cap=np_, pair_cap=nq - 1) == (-6, np_, nq)
    r2, p2, q2 = eng.stage2x_batch_raw(probs, qbuf, qucbuf, path_cap=np_, pair_cap=nq)
    assert s2x.engine_lists(r2, p2, q2) == s2x.engine_lists(results, paths, pairs)


def _rc(e, probs, qbuf, qucbuf):
    n = len(probs)
    results = np.zeros(n, dtype=gmapdp.STAGE2_RESULT_DTYPE)
    paths = np.zeros(64, dtype=gmapdp.PATH_DTYPE)
    pairs = np.zeros(4096, dtype=gmapdp.PATH_PAIR_DTYPE)
    pn, qn = C.c_size_t(), C.c_size_t()
    rc = e.lib.gmapdp_stage2x_batch(e.h, probs.ctypes.data, n, qbuf, qucbuf, len(qucbuf), results.ctypes.data,
                                    paths.ctypes.data, len(paths), pairs.ctypes.data, len(pairs), C.byref(pn),
                                    C.byref(qn))
    return rc, e.lib.gmapdp_last_error(e.h).decode()


def test_gpu_stage2x_refusals(eng):
    calls = s2x.random_calls(s2x.ONE, 4, seed=41)

    def batch(**edit):
        probs, qbuf, qucbuf = eng.build_stage2x_batch(calls, s2x.ONE)
        for k, (i, v) in edit.items():
            probs[k][i] = v
        return probs, qbuf, qucbuf

    assert _rc(eng, *batch())[0] == 0
    for what, edit in (("mixed", dict(kind=(2, s2x.ENDS))), ("kind", dict(kind=(0, 3))), ("kind", dict(kind=(0, 0))),
                       ("flags", dict(flags=(1, 1))), ("querylength", dict(querylength=(3, 8))),
                       ("maxintronlen", dict(maxintronlen=(0, -1)))):
        rc, msg = _rc(eng, *batch(**edit))
        assert rc == -1 and what in msg, (what, rc, msg)   # GMAPDP_EINVAL
    for mode in (2, 4, 6):
        e = gmapdp.Engine(0, mode=mode)
        try:
            e.set_genome(s2x.genome())
            rc, msg = _rc(e, *batch())
            assert rc == -1 and "non-stranded" in msg, (mode, rc, msg)
        finally:
            e.close()
    e = gmapdp.Engine(0)
    try:
        rc, msg = _rc(e, *batch())
        assert rc == -5 and "genome" in msg, (rc, msg)      # GMAPDP_ENOGENOME
    finally:
        e.close()


def test_gpu_stage2x_leaves_stage2_batch_alone():
    """The context's grow-only buffers are shared: a Stage2_compute batch returns the same results and the same
    pair records before and after batches of both kinds."""
    import random
    rng = random.Random(5)
    g = repeat_genome(rng, 120000)
    s2 = [stage2_problem(rng, g, edge=(i % 5 == 0)) for i in range(24)]
    e = gmapdp.Engine(0)
    try:
        e.set_genome(g)
        probs, qbuf, qucbuf = e.build_stage2_batch(s2)
        before = e.stage2_batch_raw(probs, qbuf, qucbuf)
        xs = []
        for kind in KINDS:
            calls = [dict(c, kind=kind, query_offset=7) for c in s2[:12]]
            xs.append(e.stage2x_batch(calls, kind))
        after = e.stage2_batch_raw(probs, qbuf, qucbuf)
        # (the kernels take their path and pair slots from the batch's pools in the order the waves finish, so
        # path_offset / pair_offset differ from run to run; everything else is compared byte for byte)
        for f in ("nresults", "npaths", "ncovered", "status", "diag_querystart", "diag_queryend", "npairs"):
            assert before[0][f].tobytes() == after[0][f].tobytes(), f

        def records(out):
            res, paths, pairs = out
            recs = []
            for r in res:
                for k in range(int(r["nresults"])):
                    pr = paths[int(r["path_offset"]) + k]
                    o = int(pr["pair_offset"])
                    recs.append(pairs[o:o + int(pr["npairs"])].tobytes())
            return recs
        assert records(before) == records(after)
        assert len(records(before)) > 10
        o = s2x.S2XOracle()
        o.set_genome(g)
        for kind, got in zip(KINDS, xs):
            calls = [dict(c, kind=kind, query_offset=7) for c in s2[:12]]
            for p, r in zip(calls, got):
                x = o.compute(p)
                assert (r[0], r[1]) == (x[0], _strip(x[1]))
    finally:
        e.close()
