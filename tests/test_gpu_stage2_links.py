"""Stage2_compute's link records at the edges of their 16-byte form (s2c_kernel.hip: S2Hit {consec, root,
tracei, pred}; the score only in the score array, a hit's query position from off[]), bit for bit against
the oracle restatement (oracle/stage2_chain_oracle.c) the way test_gpu_stage2.py compares:

  * both walk classes: a 2-kb read against a 30-kb window (at most 4 096 hits: s2c's LDS link table, whose
    loader finds each hit's position from the offsets) and against a 250-kb window (more: s2_walk_diag);
  * real links: two exons 40 kb apart and a 3-nt deletion inside an exon, where the walk leaves the
    diagonal and has to find the predecessor's query position in off[];
  * a path from the first query position with hits (no predecessor), and a read whose last 8-mers sit 3 nt
    off the diagonal (the chain's best cell has fewer than MIN_TERMINAL_NCONSECUTIVE matches: the 3'-end
    prune loop);
  * several kept results on a repeat-rich genome (the second walk, Stage2_filter_unique, candidates that
    share a query position or a root);
  * a 66 000-nt query (query positions past 2^16: the one-lane walk, which steps the position down off[]),
    through the plan (the synchronous batch's seeding launch does not take a query of that many 8-mers);
  * a stage-2 plan run on a second arena of shorter reads after its sizing run on longer ones: nothing of
    the first run's npositions may show (the plan does not clear them; the seeding writes every position).
"""
import random

import numpy as np
import pytest

import gmapdp
from dpbind import (Oracle, oracle_stage2_batch, random_genome, repeat_genome, stage2_mismatches,
                    stage2_problem)

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
SMALL = (90000, 120000)   # the LDS link table's class for a 2-kb read (~2 700 hits)
LARGE = (20000, 270000)   # ~9 000 hits: the global walk


@pytest.fixture(scope="module")
def engine():
    e = gmapdp.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def genome():
    return random_genome(random.Random(7100), 300000)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def _subs(rng, s, rate, head=0):
    q = bytearray(s)
    for i in range(head, len(q)):
        if rng.random() < rate:
            q[i] = rng.choice(b"ACGT")
    return bytes(q)


def _call(g, quc, window, plusp=1):
    if not plusp:
        quc = quc.translate(COMP)[::-1]
    return dict(q=quc, quc=quc, chrstart=window[0], chrend=window[1], chroffset=0, chrhigh=len(g), plusp=plusp,
                splicingp=1, maxintronlen=500000)


def _nhits(g, c):
    """The seeding's hits of a call, one per (query position, window position) with the same 8-mer."""
    q = c["quc"]
    cnt = {}
    for i in range(len(q) - 7):
        cnt[q[i:i + 8]] = cnt.get(q[i:i + 8], 0) + 1
    lo, hi = c["chrstart"], c["chrend"] - 8 + (0 if c["plusp"] else 1)
    n = 0
    for p in range(lo, hi + 1):
        k = g[p:p + 8]
        n += cnt.get(k if c["plusp"] else k.translate(COMP)[::-1], 0)
    return n


def _run(engine, oracle, genome, calls):
    engine.set_genome(genome)
    oracle.set_genome(genome)  # (the oracle library holds one genome: the last one set)
    exp = [oracle.stage2_compute(c) for c in calls]
    got = engine.stage2_batch(calls)
    for i, (a, b) in enumerate(zip(got, exp)):  # (number of results, each result's pair records)
        if a != b:
            where = ""
            if a[0] == b[0]:
                k = next(k for k in range(a[0]) if a[1][k] != b[1][k])
                x, y = a[1][k], b[1][k]
                j = next((j for j, (u, v) in enumerate(zip(x, y)) if u != v), min(len(x), len(y)))
                where = "; result %d (%d vs %d records) differs first at record %d: %s vs %s" % (
                    k, len(x), len(y), j, x[j] if j < len(x) else None, y[j] if j < len(y) else None)
            raise AssertionError("call %d (window %d..%d, plusp %d, %d nt): gpu %s results vs oracle %s%s" % (
                i, calls[i]["chrstart"], calls[i]["chrend"], calls[i]["plusp"], len(calls[i]["quc"]), a[0], b[0], where))
    return exp


def test_gpu_stage2_links_both_walk_classes(engine, oracle, genome):
    rng = random.Random(7101)
    read = _subs(rng, genome[100000:102000], 0.02, head=20)
    calls = [_call(genome, read, w, pl) for pl in (1, 0) for w in (SMALL, LARGE)]
    nh = [_nhits(genome, c) for c in calls]
    assert nh[0] <= 4096 < nh[1] and nh[2] <= 4096 < nh[3], nh
    exp = _run(engine, oracle, genome, calls)
    # one path per call from the read's first position (the first position with hits: no predecessor)
    assert all(r[0] == 1 and r[1][0][0][0] == 0 for r in exp)


def test_gpu_stage2_links_real_links(engine, oracle, genome):
    rng = random.Random(7102)
    two = _subs(rng, genome[100000:101000] + genome[141000:142000], 0.02)
    dele = _subs(rng, genome[100000:101000] + genome[101003:102000], 0.01)
    calls = [_call(genome, two, (99000, 143000)), _call(genome, two, (30000, 280000)),
             _call(genome, dele, (95000, 110000)), _call(genome, dele, LARGE),
             _call(genome, two, (30000, 280000), 0), _call(genome, dele, (95000, 110000), 0)]
    nh = [_nhits(genome, c) for c in calls[:4]]
    assert nh[0] <= 4096 < nh[1] and nh[2] <= 4096 < nh[3], nh
    exp = _run(engine, oracle, genome, calls)
    # the two-exon path spans the 40-kb intron; the deletion's path covers both sides of it
    assert exp[1][1][0][0][1] == 100000 and exp[1][1][0][-1][1] == 141999
    assert exp[3][1][0][0][1] == 100000 and exp[3][1][0][-1][1] == 101999


def test_gpu_stage2_links_three_prime_prune(engine, oracle, genome):
    # the last ten nucleotides follow a 3-nt deletion: their 8-mers link to the chain with no consecutive
    # matches and a better score, so the best cell is one of them and traceback_one prunes it away
    near = genome[100000:101985] + genome[101988:101998]
    # the last ten nucleotides copied from 48 kb downstream
    far = genome[100000:101990] + genome[150000:150010]
    calls = [_call(genome, near, (95000, 110000)), _call(genome, near, LARGE),
             _call(genome, far, (98000, 152000)), _call(genome, far, LARGE)]
    nh = [_nhits(genome, c) for c in calls]
    assert nh[0] <= 4096 < nh[1] and nh[2] <= 4096 < nh[3], nh
    exp = _run(engine, oracle, genome, calls)
    assert [r[1][0][-1][:2] for r in exp] == [(1985, 101985)] * 2 + [(1989, 101989)] * 2


def test_gpu_stage2_links_several_results(engine, oracle):
    rng = random.Random(7200)
    g = repeat_genome(rng, 200000)
    calls = [stage2_problem(rng, g, edge=(i % 5 == 0)) for i in range(200)]
    exp = _run(engine, oracle, g, calls)
    assert sum(1 for r in exp if r[0] > 1) > 0


def test_gpu_stage2_links_query_past_65536(engine, oracle):
    # the seeding takes at most 16 384 distinct 8-mers per query, so the 66 000-nt read comes from six
    # copies of a 12-kb unit that differ in 0.3 % of their positions (six hits per query position)
    rng = random.Random(7105)
    unit = random_genome(rng, 12000, nfrac=0.0)
    g = random_genome(rng, 2000) + b"".join(_subs(rng, unit, 0.003) for _ in range(6)) + random_genome(rng, 2000)
    read = g[2500:68500]
    assert len({read[i:i + 8] for i in range(len(read) - 7)}) <= 16384
    oracle.set_genome(g)
    engine.set_genome(g)
    probs, qb, qub = gmapdp.Engine.build_stage2_batch([_call(g, read, (1000, len(g) - 1000))])
    exp = oracle_stage2_batch(oracle, probs, qb, qub)
    assert exp[0][0, 0] == 1 and exp[1][0, 0, 1] == 66000  # one path, a record per nucleotide
    res, paths, pairs, _ = engine.stage2_plan_raw(probs, qb, qub)
    bad = stage2_mismatches(res, paths, pairs, exp)
    assert not bad, bad


def test_gpu_stage2_links_plan_rerun_shorter_reads(engine, oracle, genome):
    """The plan's sizing run seeds arena A (2-kb reads); its run then seeds arena B of the same layout, whose
    reads come from other loci of the windows and are 600 to 1 500 nt long (the slices' remainders hold N:
    no 8-mer).  Equal to the oracle on B, as a fresh plan made on B is."""
    rng = random.Random(7104)
    calls_a, reads_b = [], []
    for k in range(12):
        at = 60000 + 15000 * k
        window = LARGE if k % 4 == 0 else (at - 10000, at + 20000)
        calls_a.append(_call(genome, _subs(rng, genome[at:at + 2000], 0.02), window, k % 2))
        n = rng.randint(600, 1500)
        b = _subs(rng, genome[at + 700:at + 700 + n], 0.02) + b"N" * (2000 - n)
        reads_b.append(b if k % 2 else b.translate(COMP)[::-1])
    engine.set_genome(genome)
    oracle.set_genome(genome)
    probs, qa, _ = gmapdp.Engine.build_stage2_batch(calls_a)
    qb = b"".join(reads_b)
    assert len(qb) == len(qa)
    exp = oracle_stage2_batch(oracle, probs, qb, qb)
    assert np.all(exp[0][:, 0] >= 1)
    res, paths, pairs, _ = engine.stage2_plan_raw(probs, qa, qa, run_qbuf=qb, run_qucbuf=qb)
    bad = stage2_mismatches(res, paths, pairs, exp)
    assert not bad, bad[:8]
    res2, paths2, pairs2, _ = engine.stage2_plan_raw(probs, qb, qb)
    bad = stage2_mismatches(res2, paths2, pairs2, exp)
    assert not bad, bad[:8]
    for k in ("nresults", "npaths", "ncovered", "status", "npairs"):
        assert np.array_equal(res[k], res2[k]), k
