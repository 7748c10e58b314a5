"""The CPU oracle of Stage2_compute_starts (tests/s2soracle) against the goldens the reference's own function
produced (tests/golden/stage2_starts_golden.npz, tests/golden/make_stage2_starts.py), the goldens' power, and the
mirror property the engine's route rests on: a STARTS call is the ENDS call on the reverse-complemented query
and the opposite strand, seen from the other end."""
import functools

import numpy as np

import s2starts
import s2x
from dpbind import Oracle


@functools.lru_cache(maxsize=None)
def _oracle_on_goldens():
    g, calls, expected, counters = s2starts.golden()
    orc = s2starts.S2SOracle()
    orc.set_genome(g)
    got, cnt = [], []
    for p in calls:
        got.append(orc.compute(p))
        cnt.append([orc.counters(p)[k] for k in s2starts.COUNTERS])
    return got, np.array(cnt, dtype=np.int64)


def test_oracle_equals_every_golden():
    """Every golden call's lists exactly, dynprogindex included."""
    g, calls, expected, counters = s2starts.golden()
    got, _ = _oracle_on_goldens()
    assert len(calls) >= 100
    bad = [i for i, (r, e) in enumerate(zip(got, expected)) if r[0] == "err" or (r[0], r[1]) != e]
    assert not bad, "oracle differs from the reference's lists in calls %s" % bad[:10]
    for r, p in zip(got, calls):  # status 0 / 2, the bounds of Diag_max_bounds
        n, lists, sc = r
        assert sc[3] in (0, 2) and (sc[3] == 2 or n == 0)
        if sc[3] == 2:
            assert (sc[4], sc[5]) == (0, len(p["quc"]) - 1)


def test_goldens_reach_every_rule():
    g, calls, expected, counters = s2starts.golden()
    _, cnt = _oracle_on_goldens()
    assert np.array_equal(cnt, counters), "the stored counters are not the oracle's"
    for j, name in enumerate(s2starts.COUNTERS):
        if name == "pruned":
            # unreachable with localp and middlep false (only adjacent hits ever link, so every chain
            # counts at least MIN_TERMINAL_NCONSECUTIVE matches at each hit)
            assert counters[:, j].sum() == 0
        else:
            assert counters[:, j].sum() > 0, name
    assert {p["plusp"] for p in calls} == {0, 1}
    assert {p["splicingp"] for p in calls} == {0, 1}
    assert any(p["query_offset"] for p in calls) and any(not p["query_offset"] for p in calls)
    assert any(n == 0 for n, _ in expected) and any(n == 1 for n, _ in expected) and any(n > 1 for n, _ in expected)
    # every list runs 3' end first and carries no gap holder; the returned lists descend in their first pair's
    # genomepos, then in their last pair's (stage2pairs_start_cmp)
    for (n, lists), p in zip(expected, calls):
        for lst in lists:
            qp = [x[0] for x in lst]
            assert qp == sorted(qp, reverse=True) and not any(x[9] for x in lst)
            assert min(qp) >= p["query_offset"]
        keys = [(lst[0][1], lst[-1][1]) for lst in lists]
        assert keys == sorted(keys, reverse=True)


def test_starts_differs_from_ends():
    """The direction is observable: Stage2_compute_ends' oracle on the same call returns other lists (even with
    each list reversed) for some golden."""
    g, calls, expected, _ = s2starts.golden()
    xo = s2x.S2XOracle()
    xo.set_genome(g)
    differ = 0
    for p, e in zip(calls, expected):
        r = xo.compute(dict(p, kind=s2x.ENDS))
        differ += r[0] == "err" or (r[0], [lst[::-1] for lst in r[1]]) != e
    assert differ >= 10, differ


def test_mirror_property():
    """A STARTS call against the ENDS oracle (tests/s2xoracle, a lookback) on the reverse-complemented query and
    the opposite strand of the same window, its lists taken back pair by pair (s2starts.unmirror_lists).

    The chain is the mirror image; the *seeding* is not always: Oligoindex_hr_tally takes mappingend one further
    on the minus strand (stage2.c:6977-6987), so a hit at the window's edge can exist on one strand only.  Here
    on the CPU, 225 of the 246 calls (the edge shapes and 200 random ones) agree as sets of lists, and every one
    of those also in list order; all 21 others have per-position hit counts that are not each other's mirror
    image.  So the set equality is not asserted over all calls (recorded instead); it is asserted, with the list
    order, for every call whose seeding mirrors -- the statement route (a) of the engine needs."""
    orc = Oracle()
    orc.set_genome(s2starts.genome())
    so, xo = s2starts.S2SOracle(orc), s2x.S2XOracle(orc)
    calls = list(s2starts.edge_calls()[0]) + s2starts.random_calls(200, seed=11)
    as_set = in_order = mirrored_seeding = with_lists = 0
    for p in calls:
        a = so.compute(p)
        m = s2starts.mirrored_ends_call(p)
        b = xo.compute(m)
        assert a[0] != "err" and b[0] != "err"
        back = s2starts.unmirror_lists(p, b[1])
        same_set = sorted(map(tuple, a[1])) == sorted(map(tuple, back))
        same_order = a[1] == back
        as_set += same_set
        in_order += same_order
        nq = len(p["quc"]) - 7
        n1 = list(orc.oligo_mappings(dict(p, minor=1))[1][:nq])
        n2 = list(orc.oligo_mappings(dict(m, minor=1))[1][:nq])
        if n1 == n2[::-1]:
            mirrored_seeding += 1
            with_lists += a[0] > 0
            assert same_set and same_order, (p["chrstart"], p["chrend"], p["plusp"], len(p["quc"]))
    print("mirror property: %d calls, %d equal as sets, %d also in list order, %d with mirrored seeding"
          % (len(calls), as_set, in_order, mirrored_seeding))
    assert mirrored_seeding >= 200 and with_lists >= 150
    assert as_set >= mirrored_seeding and in_order >= mirrored_seeding


def test_oracle_batch_equals_single_calls():
    """orc_stage2s_batch (threads, the engine's 20-byte pair records) returns what the single calls return."""
    import gmapdp
    orc = s2starts.S2SOracle()
    orc.set_genome(s2starts.genome())
    calls = list(s2starts.edge_calls()[0]) + s2starts.random_calls(40, seed=5)
    probs, qbuf, qucbuf = gmapdp.Engine.build_stage2x_batch(calls, gmapdp.S2X_STARTS)
    assert set(probs["kind"]) == {3}
    scal, paths, pairs, pair_off = orc.batch(probs, qbuf, qucbuf, nthreads=4)
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
    """The edge shapes of the GPU tests by the seeding itself and by the oracle's counters."""
    orc = Oracle()
    orc.set_genome(s2starts.genome())
    so = s2starts.S2SOracle(orc)
    calls, tags = s2starts.edge_calls()
    tot, mx, npos = [], [], []
    for p in calls:
        sc, n = orc.oligo_mappings(dict(p, minor=1))[:2]
        tot.append(sc[0])
        mx.append(max(n))
        npos.append(list(n[:len(p["quc"]) - 7]))
    assert 0 in tot and 1 in tot and {64, 70, 99, 100} <= set(mx), (sorted(set(tot))[:5], sorted(set(mx)))
    assert {9, 10, 64} <= {len(p["quc"]) for p in calls}
    assert any(p["chrend"] == p["chrstart"] for p in calls) and any(p["chrend"] + 1 == p["chrstart"] for p in calls)
    for p, t, n in zip(calls, tags, npos):
        if t == "tail_nohit":   # the sweep's first position is not querylength - 8
            assert n[-3:] == [0, 0, 0] and n[-4] > 0
        if t == "head_nohit":
            assert n[:8] == [0] * 8 and n[8] > 0
        if t.startswith("hits"):
            assert max(n) == int(t[4:])
    for t in ("chrstart0", "chrlast"):   # both strands at both ends of the chromosome, each returning a list
        sel = [p for p, x in zip(calls, tags) if x == t]
        assert {p["plusp"] for p in sel} == {0, 1}
        assert all(so.compute(p)[0] >= 1 for p in sel)
        if t == "chrstart0":
            assert all(p["chrstart"] == 0 for p in sel)
        else:
            assert all(p["chrend"] + p["chroffset"] == p["chrhigh"] for p in sel)
    cn = [so.counters(p) for p in calls]
    for name in s2starts.COUNTERS:
        assert (sum(c[name] for c in cn) > 0) == (name != "pruned"), name
    assert any(c["big_position"] == 0 and m == 99 for c, m in zip(cn, mx))
    assert any(c["big_position"] > 0 and m == 100 for c, m in zip(cn, mx))
    # lists that overlap (one eliminated) and lists that do not (several returned)
    assert any(c["eliminated"] > 0 for c in cn) and any(so.compute(p)[0] > 1 for p in calls)
    intr = [(t, so.compute(p)) for p, t in zip(calls, tags) if t.startswith("intron")]
    assert {t for t, _ in intr} == {"intron_long_1", "intron_long_0", "intron_short_1", "intron_short_0"}
    assert all(r[0] >= 1 for _, r in intr)
    assert any(p["query_offset"] for p in calls)
