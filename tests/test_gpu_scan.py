"""GPU parity tests for Stage2_scan (stage2.c:5610): gmapdp_stage2_scan_batch and the
device-resident scan plan (s2scan_kernel.hip) against the oracle's seeding with the major index and
Diag_update_coverage's rule restated in tests/scanref.py.  Every check compares all four result fields
(ncovered, stage2_source, totalpositions, maxnconsecutive).  Shapes stay within querylength <= 6000 and
windows <= 60 000 nt, where the oracle's capacities hold (scanref.expected_scan asserts its status)."""
import ctypes as C
import random

import numpy as np
import pytest

import gmapdp
import s2modes
from dpbind import Oracle, oligo_problem, random_genome, repeat_genome, single_gap_problem, stage2_problem
from scanref import expected_scan, expected_scans, ncovered_from_diagonals

pytestmark = pytest.mark.gpu

POLYA = (200000, 2500)   # an A-rich stretch: 8-mer counts pass Count_T's 255
QLENS = (9, 10, 63, 64, 65, 71, 72, 200, 700, 2000)
WINDOWS = (0, 8, 9, 300, 5000, 40000)
# the size thresholds of the scan path: s2scan_kernel's LDS coverage bitmap holds 4096 query positions
# (kScanBitmapBits; longer queries take the global difference array), and oi_mappings_sorted switches its
# event key from 32-bit (diagi << 12 | t) to 64-bit past nq = querylength - 7 = 4096 query 8-mers
BITMAP_POSITIONS = 4096
KEY_SWITCH_QLEN = 4096 + 7


def _genome():
    rng = random.Random(9100)
    g = bytearray(repeat_genome(rng, 400000))
    g[POLYA[0]:POLYA[0] + POLYA[1]] = b"A" * POLYA[1]
    return bytes(g)


def _call(g, quc, chrstart, chrend, plusp, chroffset=0, chrhigh=None):
    return dict(quc=bytes(quc), chrstart=chrstart, chrend=chrend, chroffset=chroffset,
                chrhigh=len(g) if chrhigh is None else chrhigh, plusp=int(plusp))


COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _read(g, s, n, plusp, rng=None, sub=0.0):
    q = bytearray(g[s:s + n])
    if rng is not None:
        for i in range(len(q)):
            if rng.random() < sub:
                q[i] = rng.choice(b"ACGT")
    return bytes(q) if plusp else bytes(q).translate(COMP)[::-1]


def _problems(g):
    """The 600 problems of check 1 and a tag per forced category."""
    rng = random.Random(9101)
    probs, tags = [], []

    def add(p, tag=None):
        p = dict(p)
        p.pop("minor", None)
        probs.append(p)
        tags.append(tag)

    chrlen = len(g)
    for ql in QLENS:                      # query lengths, both strands, the read inside its window
        for plusp in (1, 0):
            s = rng.randint(1000, chrlen - 5000)
            add(_call(g, _read(g, s, ql, plusp, rng, 0.01), max(0, s - 150), s + ql + 150, plusp), "qlen%d" % ql)
    for w in WINDOWS:                     # window lengths
        for plusp in (1, 0):
            s = rng.randint(1000, chrlen - 50000)
            add(_call(g, _read(g, s, 600, plusp, rng, 0.01), s, s + w, plusp), "win%d" % w)
    for plusp in (1, 0):                  # windows at the chromosome's start and end
        add(_call(g, _read(g, 200, 500, plusp, rng, 0.02), 0, 3000, plusp), "chrstart")
        add(_call(g, _read(g, chrlen - 900, 500, plusp, rng, 0.02), chrlen - 3000, chrlen - 1, plusp), "chrend")
    for plusp in (1, 0):                  # N runs in the query
        q = bytearray(_read(g, 50000, 800, plusp, rng, 0.01))
        q[100:140] = b"N" * 40
        q[400:409] = b"N" * 9
        add(_call(g, q, 49000, 52000, plusp), "nrun")
    for plusp in (1, 0):                  # counts past 255: a poly-A / poly-T query head over the A-rich stretch
        head = b"A" * 300 if plusp else b"T" * 300
        q = _read(g, POLYA[0] + POLYA[1], 400, plusp, rng, 0.01)
        add(_call(g, (head + q) if plusp else (q + head), POLYA[0] - 1000, POLYA[0] + POLYA[1] + 2000, plusp), "polya")
    for plusp in (1, 0):                  # the fallback diagonal: a 17-nt match (10 consecutive 8-mers) only
        s = 120000
        q = bytearray(rng.choice(b"ACGT") for _ in range(60))
        q[20:37] = _read(g, s + 100, 17, plusp)
        add(_call(g, q, s, s + 300, plusp), "fallback")
    for plusp in (1, 0):                  # no hits at all
        add(_call(g, b"ACGTTGCA" * 5 + b"N" * 10, 130000, 130300, plusp), "nohits")
    while len(probs) < 600:               # GMAP-shaped calls: spliced reads, repeats, edges
        p = stage2_problem(rng, g, edge=(len(probs) % 5 == 0)) if len(probs) % 2 else oligo_problem(rng, g, edge=(len(probs) % 7 == 0))
        if p["chrend"] - p["chrstart"] > 60000:  # (the generator's widest edge case: keep the far 30-60 kb)
            p["chrstart"] = p["chrend"] - rng.randint(30000, 60000)
        add(dict(quc=p["quc"], chrstart=p["chrstart"], chrend=p["chrend"], chroffset=p["chroffset"],
                 chrhigh=p["chrhigh"], plusp=p["plusp"]))
    return probs, tags


@pytest.fixture(scope="module")
def world():
    """The genome, the 600 problems, their oracle seedings and expected results: computed once, never changed."""
    g = _genome()
    probs, tags = _problems(g)
    orc = Oracle()
    orc.set_genome(g)
    seeds = [orc.oligo_mappings(dict(p, minor=0)) for p in probs]
    assert all(len(s) == 4 for s in seeds), "a problem outside the oracle's capacities"
    exp = np.array([(ncovered_from_diagonals(s[3], len(p["quc"])), 1, s[0][0], s[0][1]) for s, p in zip(seeds, probs)],
                   dtype=np.int32)
    exp.setflags(write=False)
    return dict(g=g, probs=probs, tags=tags, seeds=seeds, exp=exp, orc=orc)


@pytest.fixture(scope="module")
def engine(world):
    e = gmapdp.Engine(0)
    e.set_genome(world["g"])
    yield e
    e.close()


def _diff(got, exp, probs):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    if len(bad) == 0:
        return None
    i = int(bad[0])
    p = {k: v for k, v in probs[i].items() if k != "quc"}
    return "%d of %d differ; first: problem %d (%s, qlen %d): gpu %s vs oracle %s" % (
        len(bad), len(exp), i, p, len(probs[i]["quc"]), got[i].tolist(), exp[i].tolist())


def test_scan_categories_present(world):
    """The generator's promises, checked on the oracle's outputs."""
    probs, tags, seeds, exp = world["probs"], world["tags"], world["seeds"], world["exp"]
    assert len(probs) == 600
    assert {p["plusp"] for p in probs} == {0, 1}
    assert all(p["quc"] == p["quc"].upper() for p in probs)
    assert all(len(p["quc"]) <= 6000 and p["chrend"] - p["chrstart"] <= 60000 for p in probs)
    for ql in QLENS:
        assert any(len(p["quc"]) == ql for p in probs), ql
    for w in WINDOWS:
        assert any(p["chrend"] - p["chrstart"] == w for p in probs), w
    assert any(p["chrstart"] == 0 for p in probs)
    assert any(p["chroffset"] + p["chrend"] >= len(world["g"]) - 1 for p in probs)
    assert any(b"NNNNNNNNN" in p["quc"] for p in probs)
    # Count_T wrap: the poly-A problems see more than 255 occurrences of AAAAAAAA in their window
    for i, t in enumerate(tags):
        if t == "polya":
            assert world["g"][probs[i]["chrstart"]:probs[i]["chrend"]].count(b"A" * 263) >= 1
            assert max(seeds[i][1]) <= 255
    # many good diagonals whose ranges overlap or touch
    many = [i for i, s in enumerate(seeds) if len(s[3]) >= 4]
    assert len(many) >= 10
    overl = 0
    for i in many:
        iv = sorted((d[1], d[2]) for d in seeds[i][3])
        overl += any(b[0] <= a[1] for a, b in zip(iv, iv[1:]))
    assert overl >= 5
    fb = [i for i, t in enumerate(tags) if t == "fallback"]
    assert fb and all(0 < seeds[i][0][1] < 20 and seeds[i][0][3] == 1 for i in fb)
    nh = [i for i, t in enumerate(tags) if t == "nohits"]
    assert nh and all(seeds[i][0][0] == 0 and exp[i][0] == 0 for i in nh)
    assert (exp[:, 0] > 0).sum() > 400


def test_scan_batch_matches_oracle(engine, world):
    """Check 1: the 600 problems, all four fields."""
    got = engine.stage2_scan_batch(world["probs"])
    assert got.shape == (600, 4) and got.dtype == np.int32
    d = _diff(got, world["exp"], world["probs"])
    assert d is None, d


def test_scan_shared_query_slices(engine, world):
    """Check 2: 40 reads x 6 windows, the six problems of a read on one query slice (the same qoff),
    interleaved with the other reads' problems.  Fails on an implementation that keeps npositions / mappings
    in arrays indexed like the query arena."""
    g, orc = world["g"], world["orc"]
    rng = random.Random(9102)
    reads = []
    for r in range(40):
        plusp = r % 2
        s = rng.randint(5000, len(g) - 60000)
        ql = rng.randint(300, 1500)
        reads.append((_read(g, s, ql, plusp, rng, 0.02), s, ql, plusp))
    calls = []
    for w in range(6):  # window-major: a read's problems lie 40 apart
        for quc, s, ql, plusp in reads:
            if w == 0:
                lo, hi = s - 200, s + ql + 200                    # the true window
            elif w == 1:
                lo, hi = s + ql // 2, s + ql // 2 + 3000          # half of the locus
            elif w == 2:
                lo, hi = s - 2500, s + ql // 3                    # the first third
            else:
                lo = rng.randint(0, len(g) - 30000)               # decoys elsewhere
                hi = lo + rng.choice((ql + 400, 5000, 20000))
            calls.append(_call(g, quc, max(lo, 0), hi, plusp))
    probs, qucbuf = gmapdp.Engine.build_scan_batch(calls)
    assert len(qucbuf) == sum(len(r[0]) for r in reads)
    for r in range(40):
        assert len({int(probs[w * 40 + r]["qoff"]) for w in range(6)}) == 1
    exp = expected_scans(orc, calls)
    assert len({tuple(exp[w * 40 + 0]) for w in range(6)}) >= 3  # a read's windows give different answers
    got = engine.stage2_scan_batch_raw(probs, qucbuf)
    d = _diff(got, exp, calls)
    assert d is None, d


def test_scan_sub_batches(world, monkeypatch):
    """Check 3: GMAPDP_SCAN_ARENA_MB (read when a plan is made; set here before the engine exists) small
    enough for at least 3 sub-batches gives identical results; one problem whose worst-case capacity alone
    exceeds the budget still runs, in a sub-batch of its own."""
    probs, qucbuf = gmapdp.Engine.build_scan_batch(world["probs"])
    monkeypatch.delenv("GMAPDP_SCAN_ARENA_MB", raising=False)
    eng = gmapdp.Engine(0)
    try:
        eng.set_genome(world["g"])
        with eng.scan_plan(probs, qucbuf) as plan:
            n_default, bytes_default = plan.nlaunches, plan.scratch_bytes
    finally:
        eng.close()
    monkeypatch.setenv("GMAPDP_SCAN_ARENA_MB", "8")
    eng = gmapdp.Engine(0)
    try:
        eng.set_genome(world["g"])
        with eng.scan_plan(probs, qucbuf) as plan:
            assert plan.nlaunches >= 3 and plan.nlaunches > n_default
            assert plan.scratch_bytes <= 8 << 20 < bytes_default
            plan.run()
            got_plan = plan.results()
        got = eng.stage2_scan_batch_raw(probs, qucbuf)
        d = _diff(got, world["exp"], world["probs"])
        assert d is None, d
        assert np.array_equal(got_plan, got)
        # one problem beyond the budget: a 2-kb read on a 40-kb window against 1 MB
        monkeypatch.setenv("GMAPDP_SCAN_ARENA_MB", "1")
        g = world["g"]
        big = [_call(g, _read(g, 300000, 2000, 1), 290000, 330000, 1)]
        bp, bq = gmapdp.Engine.build_scan_batch(big)
        with eng.scan_plan(bp, bq) as plan:
            assert plan.nlaunches == 1 and plan.scratch_bytes > 1 << 20
            plan.run()
            got_big = plan.results()
        exp_big = expected_scans(world["orc"], big)
        assert exp_big[0][0] > 1900
        d = _diff(got_big, exp_big, big)
        assert d is None, d
    finally:
        eng.close()


def test_scan_size_thresholds(engine, world):
    """Check 4: both sides of the LDS-bitmap threshold (querylength 4096 | 4097: s2scan_kernel's bitmap versus
    its global difference array) and of oi_mappings_sorted's key-format switch at nq 4096 (querylength
    4103 | 4104), spliced and contiguous reads on both strands."""
    g, orc = world["g"], world["orc"]
    rng = random.Random(9103)
    calls = []
    for ql in (BITMAP_POSITIONS - 1, BITMAP_POSITIONS, BITMAP_POSITIONS + 1, KEY_SWITCH_QLEN - 1, KEY_SWITCH_QLEN,
               KEY_SWITCH_QLEN + 1, 5000, 6000):
        for plusp in (1, 0):
            s = rng.randint(10000, len(g) - 40000)
            calls.append(_call(g, _read(g, s, ql, plusp, rng, 0.02), s - 300, s + ql + 300, plusp))
            # three exons 2 kb apart: several diagonals, a gap in the coverage where substitutions cluster
            a, b = ql // 3, ql // 3
            parts = [g[s:s + a], g[s + a + 2000:s + a + 2000 + b], g[s + a + b + 4000:s + a + b + 4000 + (ql - a - b)]]
            q = bytearray(b"".join(parts))
            q[a - 30:a + 30] = bytes(rng.choice(b"ACGT") for _ in range(60))
            q = bytes(q) if plusp else bytes(q).translate(COMP)[::-1]
            assert len(q) == ql
            calls.append(_call(g, q, s - 300, s + ql + 4300, plusp))
    # a 150-nt unit of the window repeated 27 / 30 times in the read: one good diagonal per copy, their query
    # ranges side by side, on the bitmap path (4050 nt) and on the difference-array path (4500 nt)
    for copies in (27, 30):
        for plusp in (1, 0):
            calls.append(_call(g, _read(g, 60000, 150, plusp) * copies, 59000, 62000, plusp))
    exp = expected_scans(orc, calls)
    assert all(len(orc.oligo_mappings(dict(c, minor=0))[3]) >= 27 for c in calls[-4:])
    lens = [len(c["quc"]) for c in calls]
    for ql in (BITMAP_POSITIONS, BITMAP_POSITIONS + 1, KEY_SWITCH_QLEN, KEY_SWITCH_QLEN + 1):
        assert ql in lens
    assert (exp[:, 0] > 3000).all()
    assert any(e[0] < ql - 40 for e, ql in zip(exp, lens))  # some coverage has a hole
    got = engine.stage2_scan_batch(calls)
    d = _diff(got, exp, calls)
    assert d is None, d


def _hip_stream(hip):
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    return s


def test_scan_plan_equals_batch(engine, world):
    """Check 5: the plan path on the 600 problems: run twice, and two plans back to back on one stream
    (each plan owns its scratch; the runs are ordered by the stream)."""
    probs, qucbuf = gmapdp.Engine.build_scan_batch(world["probs"])
    batch = engine.stage2_scan_batch_raw(probs, qucbuf)
    hip = gmapdp._hip()
    st = _hip_stream(hip)
    try:
        with engine.scan_plan(probs, qucbuf) as a, engine.scan_plan(probs[::-1].copy(), qucbuf) as b:
            assert a.nlaunches >= 1
            a.run()
            first = a.results()
            a.run()
            second = a.results()
            a.run(stream=st)
            b.run(stream=st)
            a.run(stream=st)
            third, rev = a.results(), b.results()
    finally:
        hip.hipStreamDestroy(st)
    d = _diff(first, world["exp"], world["probs"])
    assert d is None, d
    assert np.array_equal(first, batch) and np.array_equal(second, batch) and np.array_equal(third, batch)
    assert np.array_equal(rev[::-1], batch)


def test_scan_plan_beside_dp_plan(engine, world):
    """Check 5, second half: a scan plan on one stream beside a DP plan (Dynprog_single_gap) on another; the
    DP outputs equal the same DP plan run alone, the scan results the oracle's."""
    g = world["g"]
    rng = random.Random(9104)
    sp, qbuf, qucbuf_dp = gmapdp.Engine.build_single_batch([single_gap_problem(rng, g) for _ in range(3000)])
    probs, qucbuf = gmapdp.Engine.build_scan_batch(world["probs"])
    lib, hip = engine.lib, gmapdp._hip()
    host_res = np.zeros(len(sp), dtype=gmapdp.RESULT_DTYPE)
    gres = np.zeros(1, dtype=gmapdp.GENOME_RESULT_DTYPE)
    dp = C.c_void_p()
    engine._check(lib.gmapdp_plan_create_all(engine.h, sp.ctypes.data, len(sp), None, 0, None, 0, host_res.ctypes.data,
                                             gres.ctypes.data, C.byref(dp)), "gmapdp_plan_create_all")
    ngpu, cap = lib.gmapdp_plan_gpu_problems(dp), lib.gmapdp_plan_pair_capacity(dp)
    assert ngpu > 2000
    bufs = []

    def dbuf(nbytes, src=None):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(nbytes, 16)) == 0
        bufs.append(p)
        if src is not None:
            assert hip.hipMemcpy(p, src, nbytes, 1) == 0
        return p

    def fetch(d_res, d_pairs):
        assert hip.hipDeviceSynchronize() == 0
        r = np.zeros(ngpu, dtype=gmapdp.RESULT_DTYPE)
        p = np.zeros(max(cap, 1), dtype=gmapdp.PAIR_DTYPE)
        assert hip.hipMemcpy(r.ctypes.data, d_res, r.nbytes, 2) == 0
        assert hip.hipMemcpy(p.ctypes.data, d_pairs, p.nbytes, 2) == 0
        used = [p[int(x["pair_offset"]):int(x["pair_offset"]) + max(int(x["npairs"]), 0)].tobytes() for x in r]
        return r.tobytes(), used

    s1, s2 = _hip_stream(hip), _hip_stream(hip)
    try:
        d_q, d_quc = dbuf(len(qbuf), qbuf), dbuf(len(qucbuf_dp), qucbuf_dp)
        d_res, d_pairs = dbuf(32 * max(ngpu, 1)), dbuf(16 * max(cap, 1))
        engine._check(lib.gmapdp_plan_run(engine.h, dp, d_q, d_quc, d_res, d_pairs, s1), "gmapdp_plan_run")
        alone = fetch(d_res, d_pairs)
        assert hip.hipMemset(d_res, 0, 32 * max(ngpu, 1)) == 0
        with engine.scan_plan(probs, qucbuf) as plan:
            plan.run(stream=s2)
            engine._check(lib.gmapdp_plan_run(engine.h, dp, d_q, d_quc, d_res, d_pairs, s1), "gmapdp_plan_run")
            plan.run(stream=s2)
            beside = fetch(d_res, d_pairs)
            got = plan.results()
    finally:
        assert hip.hipDeviceSynchronize() == 0
        for b in bufs:
            hip.hipFree(b)
        lib.gmapdp_plan_destroy(dp)
        hip.hipStreamDestroy(s1)
        hip.hipStreamDestroy(s2)
    assert beside[0] == alone[0] and beside[1] == alone[1]
    d = _diff(got, world["exp"], world["probs"])
    assert d is None, d


def test_scan_stranded_mode(world):
    """Check 6: cmet-stranded (mode 1) on 100 problems against the oracle over the reduced genome of each
    call's strand; a context of mode 2 gets GMAPDP_EINVAL."""
    g = s2modes.seeding_genome()
    calls = [{k: v for k, v in c.items() if k != "minor"} for c in s2modes.seeding_calls(g, 1, n=100)]
    orc = world["orc"]  # (the oracle library holds one genome per process: put the module's back afterwards)
    try:
        exp = np.array(s2modes.oracle_by_strand(orc, g, 1, calls, expected_scan), dtype=np.int32)
        plain = np.array(s2modes.oracle_by_strand(orc, g, 0, calls, expected_scan), dtype=np.int32)
    finally:
        orc.set_genome(world["g"])
    assert (exp != plain).any(axis=1).sum() > 50  # a mode-blind engine fails
    eng = gmapdp.Engine(0, mode=1)
    try:
        eng.set_genome(g)
        got = eng.stage2_scan_batch(calls)
    finally:
        eng.close()
    d = _diff(got, exp, calls)
    assert d is None, d
    eng = gmapdp.Engine(0, mode=2)
    try:
        eng.set_genome(g)
        probs, qucbuf = gmapdp.Engine.build_scan_batch(calls[:4])
        out = np.zeros((4, 4), dtype=np.int32)
        assert eng.lib.gmapdp_stage2_scan_batch(eng.h, probs.ctypes.data, 4, qucbuf, len(qucbuf), out.ctypes.data) == -1
    finally:
        eng.close()


def test_scan_domain(engine, world):
    """Check 7: minor = 1 and querylength = 8 get GMAPDP_EINVAL (-1); n = 0 is OK and writes nothing; no
    genome gets GMAPDP_ENOGENOME (-5)."""
    g = world["g"]
    lib = engine.lib
    ok = _call(g, _read(g, 3000, 400, 1), 2000, 6000, 1)
    probs, qucbuf = gmapdp.Engine.build_scan_batch([ok, ok])
    out = np.full((2, 4), 77, dtype=np.int32)
    call = lambda p, n: lib.gmapdp_stage2_scan_batch(engine.h, p.ctypes.data, n, qucbuf, len(qucbuf), out.ctypes.data)  # noqa: E731
    bad = probs.copy()
    bad[1]["minor"] = 1
    assert call(bad, 2) == -1
    bad = probs.copy()
    bad[1]["querylength"] = 8
    assert call(bad, 2) == -1
    assert call(probs, 0) == 0
    assert (out == 77).all()
    plan = C.c_void_p()
    assert lib.gmapdp_scan_plan_create(engine.h, probs.ctypes.data, 0, qucbuf, len(qucbuf), C.byref(plan)) == 0
    assert lib.gmapdp_scan_plan_nlaunches(plan) == 0
    assert lib.gmapdp_scan_plan_run(engine.h, plan, None, None, None) == 0
    lib.gmapdp_scan_plan_destroy(plan)
    assert call(probs, 2) == 0
    assert np.array_equal(out, expected_scans(world["orc"], [ok, ok]))
    bare = gmapdp.Engine(0)
    try:
        assert lib.gmapdp_stage2_scan_batch(bare.h, probs.ctypes.data, 2, qucbuf, len(qucbuf), out.ctypes.data) == -5
    finally:
        bare.close()


def test_scan_consistent_with_existing_entry_points(engine, world):
    """Check 8: on 100 problems with distinct slices, ncovered equals gmapdp_stage2_batch's result.ncovered
    where its status is at least 1, and the helper over gmapdp_oligo_mappings_batch's diagonals."""
    g = world["g"]
    rng = random.Random(9105)
    s2 = [stage2_problem(rng, g, edge=(i % 5 == 0)) for i in range(100)]
    calls = [dict(quc=p["quc"], chrstart=p["chrstart"], chrend=p["chrend"], chroffset=p["chroffset"],
                  chrhigh=p["chrhigh"], plusp=p["plusp"]) for p in s2]
    got = engine.stage2_scan_batch(calls)
    sp, qbuf, qucbuf = gmapdp.Engine.build_stage2_batch(s2)
    res, _, _ = engine.stage2_batch_raw(sp, qbuf, qucbuf)
    sel = np.nonzero(res["status"] >= 1)[0]
    assert len(sel) > 50
    assert np.array_equal(got[sel, 0], res["ncovered"][sel])
    om = engine.oligo_mappings_batch([dict(c, minor=0) for c in calls])
    for i, (sc, _, _, dg) in enumerate(om):
        assert got[i].tolist() == [ncovered_from_diagonals(dg, len(calls[i]["quc"])), 1, sc[0], sc[1]], i
