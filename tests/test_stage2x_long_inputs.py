"""The inputs of tests/test_gpu_stage2x_long.py, checked on the CPU: by the chain oracles and the seeding oracle
alone, every call of tests/s2long.py reaches what it is there for -- 65 536 or 65 537 query positions, a seeded hit
count well on its side of 4 096, the seeding class its fill is meant for, a path through the first and through the
last query position, two traced paths --, and the random calls of the existing stage-2x tests keep reaching the path
kernel's global-walk class.  These are conditions on the generators, with floors well under what they give today
(DESIGN 5.8); each test prints the figures."""
import pytest

import longq
import s2long as L
import s2x
from dpbind import Oracle

MARGIN = 500      # hits between a call's seeded total and kS2cCap = 4 096, either way
KIND_IDS = {L.ONE: "one", L.ENDS: "ends", L.STARTS: "starts"}
kinds = pytest.mark.parametrize("kind", L.KINDS, ids=[KIND_IDS[k] for k in L.KINDS])


@pytest.fixture(scope="module")
def seed():
    return Oracle()


@pytest.fixture
def orcs(seed):
    """{kind: chain oracle}, all on s2x.genome() (the oracle library's genome is the process's)."""
    seed.set_genome(s2x.genome())
    return {k: L.oracle_for(k, seed)[0] for k in L.KINDS}


def _compute(orcs, p):
    o = orcs[p["kind"]]
    r = o.compute(p)
    assert r[0] != "err", r
    return r   # (number of lists, lists, (nkept, npaths, ncovered, status, querystart, queryend))


_ROWS = {}


@pytest.fixture
def boundary(orcs, seed):
    """{kind: [(tag, call, seeded hits, oracle result)]}, computed once"""
    if not _ROWS:
        for kind in L.KINDS:
            calls, tags = L.boundary_calls(kind)
            _ROWS[kind] = [(t, p, L.seeded_hits(seed, p), _compute(orcs, p)) for t, p in zip(tags, calls)]
    return _ROWS


@kinds
def test_boundary_calls_reach_their_classes(boundary, kind):
    rows = boundary[kind]
    assert {t for t, _, _, _ in rows} == {(ql, hc, plusp, fill) for ql in L.LENGTHS for hc in (L.SMALL, L.LARGE)
                                          for plusp in (1, 0) for fill in (L.IID, L.PERIODIC)}
    assert any(p["query_offset"] for _, p, _, _ in rows) and any(not p["query_offset"] for _, p, _, _ in rows)
    for (ql, hc, plusp, fill), p, hits, r in rows:
        d8 = longq.distinct_8mers(p["quc"])
        print("%s %s: querylength %d, %d seeded hits (%s walk), %d distinct 8-mers, npaths %d, %d list(s) of %s pairs"
              % (KIND_IDS[kind], (ql, hc, plusp, fill), len(p["quc"]), hits, L.walk_of(hits, ql), d8, r[2][1], r[0],
                 [len(x) for x in r[1]]))
        assert len(p["quc"]) == ql and ql - 7 in (65536, 65537)
        assert p["plusp"] == plusp and p["splicingp"] == 1 and p["maxintronlen"] == 500000
        assert hits <= 4096 - MARGIN if hc == L.SMALL else hits >= 4096 + MARGIN, hits
        assert d8 > 16384 if fill == L.IID else d8 <= 16384, d8
        assert r[2][3] == 2 and r[0] >= 1, r[2]


@kinds
def test_boundary_calls_touch_both_ends_of_the_position_field(boundary, kind):
    """Per length, over the two strands: a returned list through query position 0 and one through querylength - 1,
    whose 8-mer starts at nq - 1: 65 535, the 16-bit field's top value, or 65 536, the first that does not fit."""
    for ql in L.LENGTHS:
        lo = hi = 0
        for t, p, _, r in boundary[kind]:
            if t[0] != ql:
                continue
            pos = {k[0] - p["query_offset"] for lst in r[1] for k in lst if not k[9]}
            lo += 0 in pos
            hi += ql - 1 in pos
        print("%s querylength %d: %d calls with a list through position 0, %d through %d"
              % (KIND_IDS[kind], ql, lo, hi, ql - 1))
        assert lo >= 1 and hi >= 1


@kinds
def test_boundary_calls_trace_several_paths_in_every_cell(boundary, kind):
    for ql in L.LENGTHS:
        for hc in (L.SMALL, L.LARGE):
            npaths = [r[2][1] for t, _, _, r in boundary[kind] if t[:2] == (ql, hc)]
            print("%s %d %s: npaths %s" % (KIND_IDS[kind], ql, hc, npaths))
            assert len(npaths) == 4 and max(npaths) >= 2


@pytest.mark.parametrize("kind", (L.ENDS, L.STARTS), ids=("ends", "starts"))
def test_several_lists_calls(orcs, seed, kind):
    calls = L.several_lists_calls(kind)
    n = 0
    for p in calls:
        r = _compute(orcs, p)
        elim = orcs[kind].counters(p)["eliminated"]
        print("%s querylength %d: %d seeded hits, npaths %d, %d lists, %d eliminated"
              % (KIND_IDS[kind], len(p["quc"]), L.seeded_hits(seed, p), r[2][1], r[0], elim))
        assert p["kind"] == kind and r[0] >= 2 and elim >= 1
        n += len(p["quc"]) == 65544
    assert n >= 1


@kinds
def test_mixed_batch_has_every_walk(orcs, seed, kind):
    calls, tags = L.mixed_batch(kind)
    walks = {L.walk_of(L.seeded_hits(seed, p), len(p["quc"])) for p, t in zip(calls, tags) if t is not None}
    assert walks == {"lds", "diag", "lane0"}
    short = [p for p, t in zip(calls, tags) if t is None]
    assert len(short) >= 3 and all(9 <= len(p["quc"]) <= 300 and p["kind"] == kind for p in short)
    assert [t is None for t in tags] == [False, True] * (len(tags) // 2)   # interleaved
    assert sum(_compute(orcs, p)[0] >= 1 for p in short) >= 2


@pytest.mark.parametrize("kind", (L.ONE, L.ENDS), ids=("one", "ends"))
def test_random_calls_reach_the_global_walk(orcs, seed, kind):
    """tests/test_gpu_stage2x.py's 300 random calls: the path kernel's over-4 096-hit instantiation of the kind runs
    there, on single and on several traced paths."""
    over = [p for p in s2x.random_calls(kind, 300, 11) if L.seeded_hits(seed, p) > 4096]
    res = [_compute(orcs, p) for p in over]
    several = sum(r[2][1] >= 2 for r in res)
    print("%s: %d of 300 calls seed more than 4 096 hits, %d of them with npaths >= 2" % (KIND_IDS[kind], len(over), several))
    assert len(over) >= 10 and several >= 3
    assert all(r[0] >= 1 for r in res)


@pytest.mark.parametrize("kind", (L.ONE, L.ENDS), ids=("one", "ends"))
def test_stranded_set_reaches_the_global_walk(seed, kind):
    """test_gpu_stage2x_stranded_mode's 60 calls (seed 23), as seeded on the plain genome."""
    seed.set_genome(s2x.genome())
    over = sum(L.seeded_hits(seed, p) > 4096 for p in s2x.random_calls(kind, 60, 23))
    print("%s: %d of 60 calls seed more than 4 096 hits" % (KIND_IDS[kind], over))
    assert over >= 3
