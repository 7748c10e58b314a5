"""Stage2_compute's compact hit layout (s2c_kernel.hip: s2a_kernel lays out only the hits of each query
position inside [minactive, maxactive], and every hit of the first position with hits), bit for bit
against the oracle restatement (oracle/stage2_chain_oracle.c), through the synchronous batch and through
the plan, on both strands.  Each case's premise is asserted on the host from the oracle's seeding and
bounds (`_layout`): T is the seeding's hit count, `laid` the hits the kernel lays out.

  * positions with hits and none in range, in mid-read, and a first position with hits most of whose hits
    are out of range (a 2-kb two-exon read over a 250-kb window: random far hits);
  * calls whose best score stays below 8 + FINAL_SCORE_TOLERANCE: the reference gives every hit of the
    first position with hits fwd_score = 8 (stage2.c:3792-3815), in range or not, and get_cells_fwd
    (:3450) takes every positive score, so those out-of-range hits are kept results of such a call (this
    is why that one position keeps all its hits in the layout);
  * a 2-kb read with one short matching stretch (stops at the coverage test) and a 120-nt one (chains
    with a handful of hits laid out of thousands seeded);
  * MAX_NACTIVE: 120 copies of a 12-mer of the read inside the intron, so five query positions in a row
    have >= 100 hits in range: four are skipped, then the most specific one is re-run;
  * the LDS link table's capacity: 4 096 and 4 097 laid-out hits (a ~4 200-nt read over a small window,
    trimmed), and more than 4 096 seeded hits with fewer laid out (a 2-kb read over 250 kb): both s2c
    launches, whichever count selects them.

A call whose only hits at chrpos >= 2^31 are out of range (kS2Domain) is not covered here: it takes a
chromosome longer than 2^31 nt with chroffset 0 (a 2-Gnt genome to build and pack per run), and the oracle
has no such status to compare with.  s2a_kernel decides it from the window's end where that is below 2^31,
else from each position's largest seeded hit, in range or not.
"""
import ctypes as C
import random

import numpy as np
import pytest

import gmapdp
from dpbind import Oracle, oracle_stage2_batch, random_genome, stage2_mismatches

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
CAP = 4096            # kS2cCap
LARGE = (20000, 270000)


@pytest.fixture(scope="module")
def engine():
    e = gmapdp.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def genome():
    return random_genome(random.Random(8100), 300000, nfrac=0.0)


def _subs(rng, s, rate):
    q = bytearray(s)
    for i in range(len(q)):
        if rng.random() < rate:
            q[i] = rng.choice(b"ACGT")
    return bytes(q)


def _call(g, quc, window, plusp=1):
    if not plusp:
        quc = quc.translate(COMP)[::-1]
    return dict(q=quc, quc=quc, chrstart=window[0], chrend=window[1], chroffset=0, chrhigh=len(g), plusp=plusp,
                splicingp=1, maxintronlen=500000)


def _layout(oracle, c):
    """The oracle's seeding and bounds of a call (the oracle's genome already set): dict with T, status, and
    for a chained call npos, low, high (per query position, the hits inside [minactive, maxactive]), q0 (the
    first position with hits at or after querystart), laid (the hits s2a_kernel lays out)."""
    sc, npos, pos, _ = oracle.oligo_mappings(dict(c, minor=0))
    T, ql = sc[0], len(c["quc"])
    buf = (C.c_int * (2 * ql + 8 * T + 16))()
    oracle.lib.orc_stage2_debug(buf)
    res = oracle.stage2_compute(c)
    oracle.lib.orc_stage2_debug(None)
    status, qstart, qend = (int(oracle._s2_sc[k]) for k in (3, 4, 5))
    out = dict(T=T, status=status, res=res)
    if status != 2:
        return out
    b = np.frombuffer(buf, dtype=np.int32)
    mn, mx = b[:ql].view(np.uint32), b[ql:2 * ql].view(np.uint32)
    npos, pos = np.array(npos), np.array(pos, dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(npos)])
    low, high = np.zeros(ql, dtype=np.int64), np.zeros(ql, dtype=np.int64)
    for q in range(min(qend, ql - 1) + 1):
        s = pos[off[q]:off[q + 1]]
        low[q] = np.searchsorted(s, mn[q], side="left")
        high[q] = max(low[q], np.searchsorted(s, mx[q], side="right"))
    has = np.nonzero(npos[qstart:qend + 1] > 0)[0]
    q0 = qstart + int(has[0]) if len(has) else -1
    laid = int((high - low).sum())
    if q0 >= 0:
        laid += int(npos[q0] - (high[q0] - low[q0]))
    out.update(npos=npos, low=low, high=high, q0=q0, laid=laid, qstart=qstart, qend=qend)
    return out


def _run(engine, oracle, g, calls):
    """The calls through the synchronous batch and through the plan, each against the oracle."""
    engine.set_genome(g)
    oracle.set_genome(g)
    exp = [oracle.stage2_compute(c) for c in calls]
    got = engine.stage2_batch(calls)
    bad = [i for i, (a, b) in enumerate(zip(got, exp)) if a != b]
    assert not bad, ("batch", bad, [(got[i][0], exp[i][0]) for i in bad])
    probs, qb, qub = gmapdp.Engine.build_stage2_batch(calls)
    orc = oracle_stage2_batch(oracle, probs, qb, qub)
    res, paths, pairs, _ = engine.stage2_plan_raw(probs, qb, qub)
    bad = stage2_mismatches(res, paths, pairs, orc)
    assert not bad, ("plan", bad)
    return exp


def test_gpu_stage2_compact_empty_ranges(engine, oracle, genome):
    rng = random.Random(8101)
    two = _subs(rng, genome[100000:101000] + genome[141000:142000], 0.02)
    one = _subs(rng, genome[150000:152000], 0.03)
    calls = [_call(genome, r, LARGE, pl) for r in (two, one) for pl in (1, 0)]
    oracle.set_genome(genome)
    g8 = {}
    for p in range(LARGE[0], LARGE[1] - 7):
        g8.setdefault(genome[p:p + 8], []).append(p)
    for c in calls:
        L = _layout(oracle, c)
        assert L["status"] == 2 and L["T"] > CAP >= L["laid"], (L["T"], L["laid"])
        mid = [q for q in range(L["q0"] + 1, L["qend"]) if L["npos"][q] > 0 and L["high"][q] == L["low"][q]]
        assert len(mid) >= 10, len(mid)
        assert L["npos"][L["q0"]] > L["high"][L["q0"]] - L["low"][L["q0"]] >= 1  # q0: hits out of range too
    # the plus-strand two-exon call, by the sequences alone: 8-mers of mid-read positions that occur in the
    # window but nowhere within the locus span (the two exons and the intron, with the bounds' slack)
    far = [q for q in range(20, 1980) if two[q:q + 8] in g8 and not any(99900 <= p <= 142100 for p in g8[two[q:q + 8]])]
    assert len(far) >= 10, len(far)
    exp = _run(engine, oracle, genome, calls)
    assert all(r[0] >= 1 for r in exp)


def test_gpu_stage2_compact_low_scores(engine, oracle, genome):
    """Calls with hardly a hit in range.  The 120-nt reads chain (no coverage test up to 150 nt) with a best
    score below 28, so the first position's out-of-range hits (score 8) are within the tolerance: several
    kept results, all but one a lone 8-mer far from the locus."""
    rng = random.Random(8102)
    calls, want_many = [], []
    for k, (n, keep) in enumerate([(120, 18), (120, 22), (140, 16), (2000, 20), (120, 18), (2000, 40)]):
        at = 60000 + 20000 * k
        read = bytearray(random_genome(rng, n, nfrac=0.0))
        s = n // 3
        read[s:s + keep] = genome[at + s:at + s + keep]
        calls.append(_call(genome, bytes(read), LARGE, 0 if k == 4 else 1))
        want_many.append(n <= 150)
    oracle.set_genome(genome)
    many = 0
    for c, w in zip(calls, want_many):
        L = _layout(oracle, c)
        if not w:
            assert L["T"] > 2000, L["T"]
            continue
        assert L["status"] == 2 and L["laid"] < L["T"] // 2, (L["status"], L["T"], L.get("laid"))
        many += L["res"][0] > 1
    assert many >= 2, many
    _run(engine, oracle, genome, calls)


def test_gpu_stage2_compact_max_nactive(engine, oracle):
    rng = random.Random(8103)
    g = bytearray(random_genome(rng, 120000, nfrac=0.0))
    ex1, ex2 = (30000, 31000), (60000, 61000)
    motif = bytes(g[30500:30512])  # a 12-mer of exon 1: five 8-mers in a row
    for i in range(120):
        at = 35000 + 150 * i
        g[at:at + 12] = motif
    g = bytes(g)
    planted = sum(1 for p in range(ex1[0], ex2[1]) if g[p:p + 12] == motif)
    assert planted >= 121, planted
    read = g[ex1[0]:ex1[1]] + g[ex2[0]:ex2[1]]
    calls = [_call(g, read, (20000, 80000), pl) for pl in (1, 0)] + [_call(g, read, (1000, 119000), 1)]
    oracle.set_genome(g)
    for c in calls:
        L = _layout(oracle, c)
        assert L["status"] == 2
        wide = L["high"] - L["low"] >= 100  # kS2MaxNactive
        runs = np.flatnonzero(wide)
        assert len(runs) >= 5 and runs[4] - runs[0] == 4, runs  # more than kS2MaxSkipped in a row
    exp = _run(engine, oracle, g, calls)
    assert all(r[0] >= 1 for r in exp)


def test_gpu_stage2_compact_class_boundary(engine, oracle, genome):
    """4 096 and 4 097 laid-out hits (the read trimmed to the lengths a host search over `_layout` found; about
    4 500 seeded), and a 2-kb read over 250 kb: more than 4 096 seeded, fewer laid out."""
    oracle.set_genome(genome)
    base = genome[100000:104300]
    calls = [_call(genome, base[:n], BOUNDARY_WINDOW) for n in BOUNDARY_READS]
    laid = [_layout(oracle, c)["laid"] for c in calls]
    assert laid == [CAP, CAP + 1], laid
    rng = random.Random(8104)
    calls.append(_call(genome, _subs(rng, genome[200000:202000], 0.02), LARGE))
    L = _layout(oracle, calls[-1])
    assert L["T"] > CAP >= L["laid"], (L["T"], L["laid"])
    exp = _run(engine, oracle, genome, calls)
    assert all(r[0] >= 1 for r in exp)


BOUNDARY_WINDOW = (99000, 105000)
BOUNDARY_READS = (4103, 4104)  # read lengths with 4 096 and 4 097 hits laid out
