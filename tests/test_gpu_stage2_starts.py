"""Stage2_compute_starts on the engine (gmapdp_stage2x_batch, kind GMAPDP_S2X_STARTS): bit-exact against the
goldens of the reference's own function (tests/golden/stage2_starts_golden.npz), against the CPU oracle
(tests/s2soracle, a direct lookforward) on the edge shapes and 300 random calls, in a stranded-mode context, with
arenas too small, in both walk classes of the path kernel, on every refusal the header lists, and beside
gmapdp_stage2_batch and an ENDS batch on one context.  Every comparison is byte-exact."""
import ctypes as C

import numpy as np
import pytest

import gmapdp
import s2modes
import s2starts
import s2x
from dpbind import Oracle, stage2_mismatches, stage2_problem, repeat_genome

pytestmark = pytest.mark.gpu
STARTS = gmapdp.S2X_STARTS


@pytest.fixture(scope="module")
def eng():
    e = gmapdp.Engine(0)
    e.set_genome(s2starts.genome())
    yield e
    e.close()


@pytest.fixture(scope="module")
def _orc():
    return s2starts.S2SOracle()


@pytest.fixture
def orc(_orc):
    _orc.set_genome(s2starts.genome())  # (the oracle library's genome is the process's: other tests set their own)
    return _orc


def test_gpu_stage2_starts_goldens_bit_exact(eng):
    g, calls, expected, _ = s2starts.golden()
    assert g == s2starts.genome() and len(calls) >= 100
    got = eng.stage2x_batch(list(calls), STARTS)
    bad = [i for i, (r, e) in enumerate(zip(got, expected)) if (r[0], r[1]) != s2starts.strip_dynprogindex(e)]
    assert not bad, "calls %s differ from the reference's lists" % bad[:10]


def test_gpu_stage2_starts_edge_shapes(eng, orc):
    calls, tags = s2starts.edge_calls()
    calls = list(calls)
    probs, qbuf, qucbuf = eng.build_stage2x_batch(calls, STARTS)
    results, paths, pairs = eng.stage2x_batch_raw(probs, qbuf, qucbuf)
    exp = orc.batch(probs, qbuf, qucbuf, nthreads=4)
    assert not stage2_mismatches(results, paths, pairs, exp)
    # what the shapes are there for, by the oracle and the seeding (tests/test_stage2_starts_oracle.py checks the
    # per-position hit counts of each tagged shape on the CPU)
    assert {int(s) for s in exp[0][:, 3]} == {0, 2} and {int(s) for s in results["status"]} == {0, 2}
    cnt = [orc.counters(p) for p in calls]
    for name in ("restart", "zero_early", "big_position", "tied_cells", "eliminated", "first_kept"):
        assert any(c[name] for c in cnt), name
    assert not any(c["pruned"] for c in cnt)   # unreachable for these arguments
    assert {9, 10, 64} <= {len(p["quc"]) for p in calls}
    assert any(p["chrend"] == p["chrstart"] for p in calls) and any(p["chrend"] + 1 == p["chrstart"] for p in calls)
    assert {"hits64", "hits70", "tail_nohit", "head_nohit", "chrstart0", "chrlast", "intron_long_1", "intron_long_0",
            "intron_short_1", "intron_short_0"} <= set(tags)
    for t in ("chrstart0", "chrlast"):
        assert {p["plusp"] for p, x in zip(calls, tags) if x == t} == {0, 1}
        assert all(int(r["nresults"]) >= 1 for r, x in zip(results, tags) if x == t)
    assert any(p["query_offset"] and int(r["nresults"]) for p, r in zip(calls, results))
    for r, p, c in zip(results, calls, cnt):
        if int(r["status"]) == 2:
            assert (int(r["diag_querystart"]), int(r["diag_queryend"])) == (0, len(p["quc"]) - 1)
            assert c["restart"] >= 1
    assert max(int(r["nresults"]) for r in results) >= 2
    # each list 3' end first, the lists by their first pair's genomepos descending
    for n, lists in s2starts.engine_lists(results, paths, pairs):
        for lst in lists:
            assert [x[0] for x in lst] == sorted((x[0] for x in lst), reverse=True)
        assert [lst[0][1] for lst in lists] == sorted((lst[0][1] for lst in lists), reverse=True)


def test_gpu_stage2_starts_random_calls_against_oracle(eng, orc):
    calls = s2starts.random_calls(300, seed=11)
    probs, qbuf, qucbuf = eng.build_stage2x_batch(calls, STARTS)
    results, paths, pairs = eng.stage2x_batch_raw(probs, qbuf, qucbuf)
    exp = orc.batch(probs, qbuf, qucbuf)
    bad = stage2_mismatches(results, paths, pairs, exp)
    assert not bad, bad[:10]
    assert int((exp[0][:, 0] > 0).sum()) > 150


def test_gpu_stage2_starts_stranded_mode():
    """A mode-1 (cmet-stranded) context: the oracle on the reduced genome of each call's strand, the pair
    characters rewritten from the real genome as convert_to_nucleotides does outside STANDARD."""
    mode = 1
    g = s2starts.genome()
    # (upper-case queries, as in tests/s2modes.py: the observed pair of an oligomer is compared with the query as
    # given, the fill pairs with queryuc, and the rewrite below takes queryuc for both)
    calls = [dict(p, q=p["quc"]) for p in s2starts.random_calls(60, seed=23)]
    e = gmapdp.Engine(0, mode=mode)
    try:
        e.set_genome(g)
        probs, qbuf, qucbuf = e.build_stage2x_batch(calls, STARTS)
        results, paths, pairs = e.stage2x_batch_raw(probs, qbuf, qucbuf)
    finally:
        e.close()
    o = s2starts.S2SOracle()
    scal = opaths = opairs = pair_off = None
    for plusp in (1, 0):
        o.set_genome(s2modes.reduced_genome(g, mode, plusp))
        s, pa, pr, po = o.batch(probs, qbuf, qucbuf, nthreads=4)
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
    ncolon = nlists = 0
    for i in range(len(probs)):
        p = probs[i]
        for k in range(max(int(scal[i, 0]), 0)):
            a = int(pair_off[i]) + int(opaths[i, k, 0])
            r = rec[a:a + int(opaths[i, k, 1])]
            gp = r["genomepos"].astype(np.int64)
            c = gv[int(p["chroffset"]) + gp] if int(p["plusp"]) else comp[gv[int(p["chrhigh"]) - gp]]
            qc = quc[int(p["qoff"]) + r["querypos"] - int(p["query_offset"])]
            mark = np.where(qc == c, ord("|"), ord(":")).astype(np.uint8)
            raw[a:a + len(r), 17] = mark
            raw[a:a + len(r), 18] = c
            raw[a:a + len(r), 19] = c
            ncolon += int(np.count_nonzero(mark == ord(":")))
            nlists += 1
    bad = stage2_mismatches(results, paths, pairs, (scal, opaths, opairs, pair_off))
    assert not bad, bad[:10]
    assert ncolon > 0 and nlists > 20


def test_gpu_stage2_starts_small_arenas(eng):
    calls = s2starts.random_calls(40, seed=31)
    probs, qbuf, qucbuf = eng.build_stage2x_batch(calls, STARTS)
    results, paths, pairs = eng.stage2x_batch_raw(probs, qbuf, qucbuf)
    np_, nq = len(paths), len(pairs)
    assert np_ > 1 and nq > 1
    assert eng.stage2x_batch_raw(probs, qbuf, qucbuf, path_cap=np_ - 1, pair_cap=nq) == (-6, np_, nq)
    assert eng.stage2x_batch_raw(probs, qbuf, qucbuf, path_cap=np_, pair_cap=nq - 1) == (-6, np_, nq)
    r2, p2, q2 = eng.stage2x_batch_raw(probs, qbuf, qucbuf, path_cap=np_, pair_cap=nq)
    assert s2starts.engine_lists(r2, p2, q2) == s2starts.engine_lists(results, paths, pairs)


def test_gpu_stage2_starts_both_walk_classes(eng, orc):
    """launch_s2c sends a call to the path kernel with the LDS link table when the seeding found at most 4 096
    hits (kS2cCap, s2c_lds_class) and the query has at most 65 536 positions, else to the one that walks the
    global arrays.  One call on each side of 4 096 hits, several traced paths each, both strands."""
    g = s2starts.genome()
    at, unit, c = s2x.REPEATS[0]            # unit 5, 180 copies, on the first chromosome
    co, end = s2x.CHROMS[0]
    import random
    rng = random.Random(7)
    calls = []
    for plusp in (1, 0):
        # 14 positions of ~175 hits; 38 positions of ~175 hits
        calls.append(s2starts._edge(g, g[at + 10:at + 31], co, end - 1, at - 200, at + unit * c + 200, plusp, rng, 5))
        calls.append(s2starts._edge(g, g[at + 10:at + 55], co, end - 1, at - 200, at + unit * c + 200, plusp, rng))
    seed = Oracle()
    seed.set_genome(g)
    tot = [seed.oligo_mappings(dict(p, minor=1))[0][0] for p in calls]
    assert all(1000 < t <= 4096 for t in tot[0::2]) and all(t > 4096 for t in tot[1::2]), tot
    probs, qbuf, qucbuf = eng.build_stage2x_batch(calls, STARTS)
    results, paths, pairs = eng.stage2x_batch_raw(probs, qbuf, qucbuf)
    exp = orc.batch(probs, qbuf, qucbuf, nthreads=4)
    assert not stage2_mismatches(results, paths, pairs, exp)
    assert all(int(r["npaths"]) > 10 and int(r["nresults"]) >= 1 for r in results)


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


def test_gpu_stage2_starts_refusals(eng):
    calls = s2starts.random_calls(4, seed=41)

    def batch(**edit):
        probs, qbuf, qucbuf = eng.build_stage2x_batch(calls, STARTS)
        for k, (i, v) in edit.items():
            probs[k][i] = v
        return probs, qbuf, qucbuf

    assert _rc(eng, *batch())[0] == 0
    for what, edit in (("one kind", dict(kind=(2, s2x.ENDS))), ("one kind", dict(kind=(1, s2x.ONE))),
                       ("kind", dict(kind=(0, 4))), ("kind", dict(kind=(0, 0))), ("flags", dict(flags=(1, 1))),
                       ("querylength", dict(querylength=(3, 8))), ("maxintronlen", dict(maxintronlen=(0, -1)))):
        rc, msg = _rc(eng, *batch(**edit))
        assert rc == -1 and what in msg, (what, rc, msg)   # GMAPDP_EINVAL
    for mode in (2, 4, 6):
        e = gmapdp.Engine(0, mode=mode)
        try:
            e.set_genome(s2starts.genome())
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


def test_gpu_stage2_starts_leaves_other_batches_alone():
    """The context's grow-only buffers are shared: a Stage2_compute batch and an ENDS batch return the same
    records before and after a STARTS batch, and the STARTS batch between them equals the oracle."""
    import random
    rng = random.Random(5)
    g = repeat_genome(rng, 120000)
    s2 = [stage2_problem(rng, g, edge=(i % 5 == 0)) for i in range(24)]
    xcalls = [dict(c, query_offset=7) for c in s2[:12]]

    def records(out):
        res, paths, pairs = out
        recs = []
        for r in res:
            for k in range(int(r["nresults"])):
                pr = paths[int(r["path_offset"]) + k]
                o = int(pr["pair_offset"])
                recs.append(pairs[o:o + int(pr["npairs"])].tobytes())
        return recs

    e = gmapdp.Engine(0)
    try:
        e.set_genome(g)
        probs, qbuf, qucbuf = e.build_stage2_batch(s2)
        eprobs, eqbuf, equcbuf = e.build_stage2x_batch(xcalls, gmapdp.S2X_ENDS)
        before = e.stage2_batch_raw(probs, qbuf, qucbuf)
        ends_before = e.stage2x_batch_raw(eprobs, eqbuf, equcbuf)
        got = e.stage2x_batch(xcalls, STARTS)
        after = e.stage2_batch_raw(probs, qbuf, qucbuf)
        ends_after = e.stage2x_batch_raw(eprobs, eqbuf, equcbuf)
        # (the kernels take their path and pair slots from the batch's pools in the order the waves finish, so
        # path_offset / pair_offset differ from run to run; everything else is compared byte for byte)
        for a, b in ((before, after), (ends_before, ends_after)):
            for f in ("nresults", "npaths", "ncovered", "status", "diag_querystart", "diag_queryend", "npairs"):
                assert a[0][f].tobytes() == b[0][f].tobytes(), f
            assert records(a) == records(b)
        assert len(records(before)) > 10 and len(records(ends_before)) > 5
        o = s2starts.S2SOracle()
        o.set_genome(g)
        for p, r in zip(xcalls, got):
            assert (r[0], r[1]) == s2starts.strip_dynprogindex(o.compute(p))
        assert sum(r[0] for r in got) > 5
    finally:
        e.close()
