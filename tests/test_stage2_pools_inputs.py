"""The inputs of tests/test_gpu_stage2_pools.py, checked on the CPU: every case's demand on the stage-2 output pools
-- the sum of nresults and the kept pair records, from the oracle alone -- stands in the relation to the pool
capacity that the case is there for (tests/s2pools.py: over, equal, one over).  Each test prints the figures."""
import pytest

import s2pools as P

# case: (which pools, path relation, pair relation); a relation is "over", "over_twice" (more than twice the
# capacity), "fit" (equal), "one_over" or "under"
AIMS = {
    "regrow": ("sync", "over_twice", "over_twice"),
    "deep": ("sync", "over", "over"),
    "ordinary": ("sync", "under", "under"),
    "ends_regrow": ("sync", "over", "over"),
    "starts_regrow": ("sync", "over", "over"),
    "pair_fit": ("sync", "under", "fit"),
    "pair_copy_over": ("sync", "under", "over"),
    "pair_one_over": ("sync", "under", "one_over"),
    "path_fit": ("sync", "fit", "under"),
    "path_one_over": ("sync", "one_over", "under"),
    "launches": ("sync", "over", "over"),
    "plan_overflow": ("plan", "over", "over"),
    "plan_path_fit": ("plan", "fit", "under"),
    "plan_path_one_over": ("plan", "one_over", "under"),
    "plan_pair_fit": ("plan", "under", "fit"),
    "plan_pair_one_over": ("plan", "under", "one_over"),
}
RELATION = {"over": lambda d, c: d > c + 1, "over_twice": lambda d, c: d > 2 * c, "fit": lambda d, c: d == c,
            "one_over": lambda d, c: d == c + 1, "under": lambda d, c: d < c}


def caps(c, pools):
    if pools == "sync":
        return P.sync_path_cap(c.n), P.sync_pair_cap(c.qsum)
    return P.plan_path_cap(c.n), P.plan_pair_cap(c.qsum)


def test_every_case_has_an_aim():
    assert set(AIMS) == set(P.CASES)


@pytest.mark.parametrize("name", sorted(AIMS))
def test_stage2_pools_case_demand(name):
    pools, path_rel, pair_rel = AIMS[name]
    c = P.case(name)
    pcap, qcap = caps(c, pools)
    print("%s: n %d, qsum %d; oracle demand %d path / %d pair records; %s capacity %d / %d (%s / %s)"
          % (name, c.n, c.qsum, c.paths, c.pairs, pools, pcap, qcap, path_rel, pair_rel))
    assert RELATION[path_rel](c.paths, pcap), (c.paths, pcap)
    assert RELATION[pair_rel](c.pairs, qcap), (c.pairs, qcap)


def test_stage2_pools_call_shapes():
    """What the building blocks promise: K results of L records on both strands, one result, none."""
    orc = P._oracles()[0]
    orc.set_genome(P.genome())
    for slot, (K, L) in enumerate(P.COPIES):
        for plusp in (1, 0):
            r = orc.stage2_compute(P.copies_call(slot, plusp))
            assert r[0] == K and [len(x) for x in r[1]] == [L] * K, (slot, plusp, r[0])
    for c in P.ordinary_batch() + [P.ordinary_call(40), P.ordinary_call(41, n=110)]:
        assert orc.stage2_compute(c)[0] == 1
    for c in [P.filler_call(i) for i in (0, 1, 2, 3, 4, 6)] + [P.filler_call(i, n=110) for i in range(5)]:
        assert orc.stage2_compute(c)[0] == 0
    assert P.nhits(P.large_call()) > 4096          # s2c's first launch (the walk over global memory)


def test_stage2_pools_deep_case_needs_two_extra_attempts():
    """The regrow rule (s2_batch_core): max(2 * capacity, counted + slack).  In the first attempt of `deep` neither
    call passes the path check (40 results against 20 slots), and a wave that stops there adds nothing to the pair
    count: the second attempt's pair pool is max(2 x 224, 0 + 64) = 448 records, short of 3 200, whatever the order
    of the waves.  So the batch takes two extra attempts at the least."""
    c = P.case("deep")
    assert c.nresults == [40, 40] and c.paths == 80 and c.pairs == 3200
    cap0 = P.sync_path_cap(c.n)
    assert cap0 < 40    # neither call fits the first attempt: no pair record is counted in it
    assert max(2 * P.sync_pair_cap(c.qsum), 0 + 64) < c.pairs   # so the second attempt's pair pool is short


def test_stage2_pools_x_calls_both_strands_and_offsets():
    for name in ("ends_regrow", "starts_regrow"):
        c = P.case(name)
        assert c.nresults == [P.X_K + 1] * c.n
        assert {int(p) for p in c.probs["plusp"]} == {0, 1}
        assert 0 in c.probs["query_offset"] and max(c.probs["query_offset"]) > 0
        assert c.pairs == 36 * (P.X_K + 1) * c.n


def test_stage2_pools_alt_arena_fits_the_plan():
    """The second arena of the plan's stale-record test: the same layout, one result per call."""
    base, alt = P.case("plan_overflow"), P.alt_case("plan_overflow")
    assert len(alt.qucbuf) == len(base.qucbuf)
    assert [int(x) for x in alt.exp[0][:, 0]] == [1] * base.n
    assert alt.paths < P.plan_path_cap(base.n) and alt.pairs < P.plan_pair_cap(base.qsum)
