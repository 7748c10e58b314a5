"""The CPU oracle of Stage2_compute_one / Stage2_compute_ends (tests/s2xoracle) against the goldens the
reference's own two functions produced (tests/golden/stage2x_golden.npz, tests/golden/make_stage2x.py), and
the goldens' power: every rule in which the two calls part from Stage2_compute fires in the set."""
import functools

import numpy as np

import s2x
from dpbind import Oracle


@functools.lru_cache(maxsize=None)
def _oracle_on_goldens():
    g, calls, expected, counters = s2x.golden()
    orc = s2x.S2XOracle()
    orc.set_genome(g)
    got, cnt = [], []
    for p in calls:
        r = orc.compute(p)
        got.append(r)
        cnt.append([orc.counters(p)[k] for k in s2x.COUNTERS])
    return got, np.array(cnt, dtype=np.int64)


def test_oracle_equals_every_golden():
    g, calls, expected, counters = s2x.golden()
    got, _ = _oracle_on_goldens()
    assert len(calls) >= 150
    bad = [i for i, (r, e) in enumerate(zip(got, expected)) if r[0] == "err" or (r[0], r[1]) != e]
    assert not bad, "oracle differs from the reference's lists in calls %s" % bad[:10]
    for r, p in zip(got, calls):  # status 0 / 2, the bounds of Diag_max_bounds
        n, lists, sc = r
        assert sc[3] in (0, 2) and (sc[3] == 2 or n == 0)
        if sc[3] == 2:
            assert (sc[4], sc[5]) == (0, len(p["quc"]) - 1)


def test_goldens_reach_every_rule():
    g, calls, expected, counters = s2x.golden()
    _, cnt = _oracle_on_goldens()
    assert np.array_equal(cnt, counters), "the stored counters are not the oracle's"
    kinds = np.array([p["kind"] for p in calls])
    for j, name in enumerate(s2x.COUNTERS):
        for kind in s2x.COUNTER_KINDS[name]:
            assert counters[kinds == kind, j].sum() > 0, (name, s2x.KIND_NAMES[kind])
    # what cannot fire stays zero: ONE neither restarts nor takes the zero-score branch nor filters, ENDS emits
    # no gap holder
    for j, name in enumerate(s2x.COUNTERS):
        for kind in (s2x.ONE, s2x.ENDS):
            if kind not in s2x.COUNTER_KINDS[name]:
                assert counters[kinds == kind, j].sum() == 0, (name, s2x.KIND_NAMES[kind])
    for kind in (s2x.ONE, s2x.ENDS):
        sel = [p for p in calls if p["kind"] == kind]
        assert {p["plusp"] for p in sel} == {0, 1}
        assert {p["splicingp"] for p in sel} == {0, 1}
        assert any(p["query_offset"] for p in sel) and any(not p["query_offset"] for p in sel)
        assert any(n == 0 for (n, _), p in zip(expected, calls) if p["kind"] == kind)
        assert any(n >= 1 for (n, _), p in zip(expected, calls) if p["kind"] == kind)
    # ONE returns at most one list, 3' end first; ENDS' lists run 5' end first and carry no gap holder
    for (n, lists), p in zip(expected, calls):
        for lst in lists:
            real = [x[0] for x in lst if not x[9]]
            if p["kind"] == s2x.ONE:
                assert n <= 1 and real == sorted(real, reverse=True)
            else:
                assert real == sorted(real) and not any(x[9] for x in lst)
    assert any(n > 1 for (n, _), p in zip(expected, calls) if p["kind"] == s2x.ENDS)


def test_ends_differs_from_stage2_compute():
    """The variant is observable: Stage2_compute's restatement (major index, localp, the coverage and
    repetitive-position rules, gap holders, Stage2_filter_unique) returns something else for some ENDS golden."""
    g, calls, expected, _ = s2x.golden()
    orc = Oracle()
    orc.set_genome(g)
    differ = same = 0
    for p, e in zip(calls, expected):
        if p["kind"] != s2x.ENDS or p["query_offset"] != 0:
            continue
        r = orc.stage2_compute(p)
        if r[0] == "err" or (r[0], r[1]) != e:
            differ += 1
        else:
            same += 1
    assert differ >= 1, (differ, same)


def test_oracle_batch_equals_single_calls():
    """orc_stage2x_batch (threads, the engine's 20-byte pair records) returns what the single calls return."""
    import gmapdp
    g = s2x.genome()
    orc = s2x.S2XOracle()
    orc.set_genome(g)
    for kind in (s2x.ONE, s2x.ENDS):
        calls = s2x.edge_calls(kind) + s2x.random_calls(kind, 40, seed=5)
        probs, qbuf, qucbuf = gmapdp.Engine.build_stage2x_batch(calls, kind)
        scal, paths, pairs, pair_off = orc.batch(kind, probs, qbuf, qucbuf, nthreads=4)
        rec = pairs[:20 * int(pair_off[-1])].view(gmapdp.PATH_PAIR_DTYPE)
        for i, p in enumerate(calls):
            n, lists, sc = orc.compute(p)
            assert int(scal[i, 0]) == n and tuple(int(x) for x in scal[i, 1:6]) == sc[1:6]
            for k in range(n):
                o = int(pair_off[i]) + int(paths[i, k, 0])
                got = [(int(x["querypos"]), int(x["genomepos"]), int(x["queryjump"]), int(x["genomejump"]),
                        bytes(x["cdna"]), bytes(x["comp"]), bytes(x["genome"]), bytes(x["genomealt"]))
                       for x in rec[o:o + int(paths[i, k, 1])]]
                assert got == [(x[0], x[1], x[2], x[3], x[5], x[6], x[7], x[8]) for x in lists[k]]


def test_edge_shapes_are_what_they_claim():
    """The edge shapes of the GPU tests by the seeding itself: a call with exactly one hit, a position with
    exactly 99 and one with exactly 100 hits, windows without hits, query lengths 9, 10 and 64."""
    orc = Oracle()
    orc.set_genome(s2x.genome())
    for kind in (s2x.ONE, s2x.ENDS):
        calls = s2x.edge_calls(kind)
        tot, mx = [], []
        for p in calls:
            sc, npos = orc.oligo_mappings(dict(p, minor=1))[:2]
            tot.append(sc[0])
            mx.append(max(npos))
        assert 0 in tot and 1 in tot and 99 in mx and 100 in mx, (sorted(set(tot))[:5], sorted(set(mx)))
        assert {9, 10, 64} <= {len(p["quc"]) for p in calls}
        assert any(p["chrend"] == p["chrstart"] for p in calls) and any(p["chrend"] + 1 == p["chrstart"] for p in calls)
        assert any(p["chrend"] - p["chrstart"] == 8 for p in calls)
        assert any(not p["plusp"] and p["chrend"] + p["chroffset"] == p["chrhigh"] for p in calls)
