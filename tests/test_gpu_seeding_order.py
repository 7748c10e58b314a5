"""The stage-2 seeding's position table in query order (oi_kernel / oi_size_kernel), and its
consumers on either order.

oi_kernel places each 8-mer's table slice where the query first uses it.  The contract, checked here through
the raw arrays of the device-resident seeding plan (gmapdp_oligo_plan_*): among the query positions with
hits, the table offsets of first occurrences ascend strictly with the query position (the slices do not
overlap), and a repeated 8-mer's position carries the offset of its first occurrence.  The split seeding
(oi_scan_kernel / oi_build_kernel: gmapdp_oligo_mappings_batch) keeps oligo order; the consumers
(oi_map_kernel, s2a_kernel) take either, so every case runs through the seeding plan, the split seeding, the
synchronous Stage2_compute batch and the stage-2 plan, each against the oracle, bit for bit.

A query of 8 nt or fewer is outside the seeding's domain (Oligoindex_set_inquery leaves stale state there):
the engine refuses it, which is what the short-query case checks, beside the shortest query it takes."""
import ctypes as C

import numpy as np
import pytest

import gmapdp
from dpbind import Oracle, oracle_stage2_batch, stage2_mismatches

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def _genome(rng, n):
    return bytearray(ACGT[rng.integers(0, 4, n)].tobytes())


def _scrub(g, kmer, sub):
    """No occurrence of kmer (nor of its reverse complement) left in g."""
    for k, s in ((kmer, sub), (_revcomp(kmer), _revcomp(sub))):
        while True:
            i = g.find(k)
            if i < 0:
                break
            g[i:i + 8] = s


@pytest.fixture(scope="module")
def engine():
    e = gmapdp.Engine(0)
    yield e
    e.close()


def _oligo_plan_raw(engine, calls):
    """The device-resident seeding plan (oi_kernel + oi_map_kernel) on `calls`: per call the oracle-format
    tuple of Engine.oligo_mappings_batch, and its raw npositions / mappings slices (the mappings relative to
    the call's table)."""
    lib, hip = engine.lib, gmapdp._hip()
    probs, qucbuf = gmapdp.Engine.build_oligo_batch(calls)
    n = len(probs)
    plan = C.c_void_p()
    engine._check(lib.gmapdp_oligo_plan_create(engine.h, probs.ctypes.data, n, qucbuf, len(qucbuf), C.byref(plan)),
                  "gmapdp_oligo_plan_create")
    bufs = []
    try:
        pc = max(lib.gmapdp_oligo_plan_positions_capacity(plan), 1)
        dc = max(lib.gmapdp_oligo_plan_diagonal_capacity(plan), 1)
        results = np.zeros(n, dtype=gmapdp.OLIGO_RESULT_DTYPE)
        npos = np.zeros(len(qucbuf), dtype=np.int32)
        maps = np.zeros(len(qucbuf), dtype=np.int32)
        positions = np.zeros(pc, dtype=np.uint32)
        diags = np.zeros(4 * dc, dtype=np.int32)

        def dbuf(arr):
            ptr = C.c_void_p()
            nbytes = len(arr) if isinstance(arr, bytes) else arr.nbytes
            src = arr if isinstance(arr, bytes) else arr.ctypes.data
            if hip.hipMalloc(C.byref(ptr), max(nbytes, 16)) != 0:
                raise gmapdp.GmapdpError("hipMalloc(%d) failed" % nbytes)
            bufs.append(ptr)
            if hip.hipMemcpy(ptr, src, nbytes, 1) != 0:  # hipMemcpyHostToDevice
                raise gmapdp.GmapdpError("hipMemcpy failed")
            return ptr
        d_quc, d_res, d_np, d_mp, d_pos, d_dg = (dbuf(a) for a in (qucbuf, results, npos, maps, positions, diags))
        engine._check(lib.gmapdp_oligo_plan_run(engine.h, plan, d_quc, d_res, d_np, d_mp, d_pos, d_dg, None),
                      "gmapdp_oligo_plan_run")
        if hip.hipDeviceSynchronize() != 0:
            raise gmapdp.GmapdpError("hipDeviceSynchronize failed")
        for arr, d in ((results, d_res), (npos, d_np), (maps, d_mp), (positions, d_pos), (diags, d_dg)):
            if hip.hipMemcpy(arr.ctypes.data, d, arr.nbytes, 2) != 0:  # hipMemcpyDeviceToHost
                raise gmapdp.GmapdpError("hipMemcpy failed")
    finally:
        for b in bufs:
            hip.hipFree(b)
        lib.gmapdp_oligo_plan_destroy(plan)
    out = []
    for i, r in enumerate(results):
        o, ql = int(probs[i]["qoff"]), int(probs[i]["querylength"])
        t0 = int(r["table_offset"])
        np_ = [int(x) for x in npos[o:o + ql]]
        mp_ = [int(x) for x in maps[o:o + ql]]
        plist = []
        for q in range(ql):
            if np_[q] > 0:
                plist.extend(int(x) for x in positions[t0 + mp_[q]:t0 + mp_[q] + np_[q]])
        d0, nd = int(r["diag_offset"]), int(r["ndiagonals"])
        dg = [tuple(int(x) for x in diags[4 * (d0 + k):4 * (d0 + k) + 4]) for k in range(nd)]
        out.append((((int(r["totalpositions"]), int(r["maxnconsecutive"]), int(r["oned_matrix_p"]), nd),
                     np_, plist, dg), np_, mp_))
    return out


def _layout_errors(quc, npos, maps):
    """Violations of the query-order layout contract of one call."""
    bad, first, end = [], {}, 0
    for q in range(len(quc) - 7):
        if npos[q] <= 0:
            continue
        k = quc[q:q + 8]
        if k in first:
            if maps[q] != first[k]:
                bad.append("position %d repeats an 8-mer at offset %d, its first occurrence is at %d"
                           % (q, maps[q], first[k]))
        else:
            if maps[q] < end:
                bad.append("position %d: offset %d below the end %d of the slices before it" % (q, maps[q], end))
            first[k] = maps[q]
            end = max(end, maps[q] + npos[q])
    return bad


def _check_seeding(engine, orc, calls, layout=True):
    """The seeding plan (query order; its layout contract) and the split seeding against the oracle."""
    exp = [orc.oligo_mappings(c) for c in calls]
    got = _oligo_plan_raw(engine, calls)
    for i, (c, (g, npos, maps)) in enumerate(zip(calls, got)):
        assert g == exp[i], "seeding plan, call %d: %s vs oracle %s" % (i, g[0], exp[i][0])
        if layout:
            bad = _layout_errors(c["quc"], npos, maps)
            assert not bad, "call %d: %s" % (i, bad[:4])
    got2 = engine.oligo_mappings_batch(calls)
    for i in range(len(calls)):
        assert got2[i] == exp[i], "split seeding, call %d: %s vs oracle %s" % (i, got2[i][0], exp[i][0])
    return exp


def _check_stage2(engine, orc, calls):
    """Stage2_compute through the synchronous batch and the stage-2 plan against the oracle: results, paths
    and pair records."""
    calls = [dict(c, splicingp=1, maxintronlen=500000) for c in calls]
    probs, qb, qub = gmapdp.Engine.build_stage2_batch(calls)
    exp = oracle_stage2_batch(orc, probs, qb, qub, nthreads=4)
    assert np.all(exp[0][:, 0] >= 0), exp[0][:, 0]
    res, paths, pairs = engine.stage2_batch_raw(probs, qb, qub)
    bad = stage2_mismatches(res, paths, pairs, exp)
    assert not bad, ("batch", bad[:8])
    res, paths, pairs, classes = engine.stage2_plan_raw(probs, qb, qub)
    bad = stage2_mismatches(res, paths, pairs, exp)
    assert not bad, ("plan", bad[:8])
    return exp, res, classes


def _both_strands(calls):
    return calls + [dict(c, quc=_revcomp(c["quc"]), plusp=0) for c in calls]


def _window_call(g, start, wlen, quc, plusp=1):
    return dict(quc=bytes(quc), chrstart=start, chrend=start + wlen, chroffset=0, chrhigh=len(g) - 1, plusp=plusp,
                minor=0)


def _mutate(rng, q, rate=0.02):
    q = bytearray(q)
    for i in np.nonzero(rng.random(len(q)) < rate)[0]:
        q[i] = int(ACGT[rng.integers(0, 4)])
    return bytes(q)


def test_gpu_seeding_order_repeated_8mers(engine):
    """A tandem repeat inside the query (several positions share an 8-mer, within one 64-position step and
    across steps) and a late position repeating 8-mers first seen near the query's start (a slice far behind
    its chunk's span); the repeat also stands in the window several times, so its positions hold more than
    4 hits inside the active range (the lay-out loop's binary searches)."""
    rng = np.random.default_rng(101)
    g = _genome(rng, 24000)
    unit = bytes(_genome(rng, 11))
    calls = []
    for k, start in enumerate((1000, 9000)):
        loc = start + 1200
        g[loc + 90:loc + 90 + 8 * 11] = unit * 8                 # the locus' tandem stretch
        for extra in (300, 700, 1500, 2100, 2600):               # and more copies across the window
            g[start + extra:start + extra + 3 * 11] = unit * 3
        locus = bytes(g[loc:loc + 260])
        tandem = _mutate(rng, locus)
        late = _mutate(rng, locus[:230]) + locus[8:48]            # positions 230.. repeat the 8-mers of 8..40
        calls += [_window_call(g, start, 3000 + 500 * k, tandem), _window_call(g, start, 3000 + 500 * k, late)]
    calls = _both_strands(calls)
    g = bytes(g)
    engine.set_genome(g)
    orc = Oracle()
    orc.set_genome(g)
    exp = _check_seeding(engine, orc, calls)
    for c, e in zip(calls, exp):  # the cases are what they claim: repeated 8-mers with hits, long slices
        q, npos = c["quc"], e[1]
        kmers = [q[i:i + 8] for i in range(len(q) - 7) if npos[i] > 0]
        assert len(set(kmers)) < len(kmers) and max(npos) > 4
    _check_stage2(engine, orc, calls)


@pytest.mark.parametrize("count", [255, 256, 300])
def test_gpu_seeding_order_count_wrap(engine, count):
    """A window holding AAAAAAAA exactly `count` times (one poly-A stretch; none elsewhere): Count_T wraps, so
    the query's AAAAAAAA position keeps the count & 255 occurrences nearest the walk's start -- none at 256 --
    and its npositions is the kept count (rebuilt after the placement has counted it down)."""
    rng = np.random.default_rng(200 + count)
    g = _genome(rng, 12000)
    _scrub(g, b"AAAAAAAA", b"AAACGAAA")
    start, loc, at = 2000, 3500, 2600
    g[at - 1:at + count + 8] = b"C" + b"A" * (count + 7) + b"G"   # count starts of AAAAAAAA
    locus = bytes(g[loc:loc + 200])
    q = _mutate(rng, locus[:120]) + b"C" + b"A" * 8 + b"G" + locus[120:]
    calls = _both_strands([_window_call(g, start, 3000, q)])
    g = bytes(g)
    assert g[start:start + 3000].count(b"A" * (count + 7)) == 1
    engine.set_genome(g)
    orc = Oracle()
    orc.set_genome(g)
    exp = _check_seeding(engine, orc, calls)
    for c, e in zip(calls, exp):
        i = c["quc"].find(b"AAAAAAAA" if c["plusp"] else b"TTTTTTTT")
        assert e[1][i] == (count & 255), (e[1][i], count)
    for (got, npos, maps), c in zip(_oligo_plan_raw(engine, calls), calls):
        i = c["quc"].find(b"AAAAAAAA" if c["plusp"] else b"TTTTTTTT")
        assert npos[i] == (count & 255) and (maps[i] >= 0) == (count != 256)
    _check_stage2(engine, orc, calls)


def test_gpu_seeding_order_edges(engine):
    """Positions without a full 8-mer (an N in the query), the shortest query the seeding takes (9 nt; 8 nt and
    fewer are refused: outside the domain), an empty window, and a query none of whose 8-mers occur."""
    rng = np.random.default_rng(301)
    g = bytes(_genome(rng, 12000))
    loc = 3000
    locus = g[loc:loc + 220]
    with_n = bytearray(_mutate(rng, locus))
    with_n[60] = with_n[61] = with_n[150] = ord("N")
    stranger = bytes(_genome(rng, 180))
    window8 = {g[i:i + 8] for i in range(2000, 5000)} | {_revcomp(g[i:i + 8]) for i in range(2000, 5000)}
    stranger = bytearray(stranger)
    for i in range(len(stranger) - 7):  # break every 8-mer the window happens to hold
        while bytes(stranger[i:i + 8]) in window8:
            stranger[i + 7] = int(ACGT[rng.integers(0, 4)])
    assert not any(bytes(stranger[i:i + 8]) in window8 for i in range(len(stranger) - 7))
    calls = _both_strands([_window_call(g, 2000, 3000, with_n), _window_call(g, 2000, 3000, locus[:9]),
                           _window_call(g, 2000, 0, locus), _window_call(g, 2000, 5, locus),
                           _window_call(g, 2000, 3000, stranger)])
    engine.set_genome(g)
    orc = Oracle()
    orc.set_genome(g)
    exp = _check_seeding(engine, orc, calls)
    assert exp[0][1][60] == 0 and exp[0][1][54] == 0 and exp[0][0][0] > 0   # the N's positions carry nothing
    assert exp[2][0][0] == 0 and exp[4][0][0] == 0                          # empty window, stranger: no hits
    _check_stage2(engine, orc, calls)
    for short in (locus[:8], locus[:5]):
        with pytest.raises(gmapdp.GmapdpError):
            _oligo_plan_raw(engine, [_window_call(g, 2000, 3000, short)])


@pytest.mark.parametrize("wlen", [66000, (1 << 18) + 600])
def test_gpu_seeding_order_counter_and_hitlist_classes(engine, wlen):
    """One call (each strand) in the 32-bit counter class (a window of 65 536 starts or more), and one with the
    8-byte hit-list entries (a window above 2^18 starts), on a genome just large enough for the window.  The
    seeding plan runs them with 32-bit counters; the stage-2 plan sizes them so and then runs them with the
    16-bit counters (hit lists far below 2^16)."""
    rng = np.random.default_rng(400 + (wlen >> 10))
    g = _genome(rng, wlen + 3000)
    loc = 1000 + wlen // 2
    unit = bytes(_genome(rng, 9))
    g[loc + 40:loc + 40 + 54] = unit * 6
    locus = bytes(g[loc:loc + 240])
    q = _mutate(rng, locus[:200]) + locus[10:50]
    calls = _both_strands([_window_call(g, 1000, wlen, q)])
    g = bytes(g)
    engine.set_genome(g)
    orc = Oracle()
    orc.set_genome(g)
    _check_seeding(engine, orc, calls)
    _, _, (n16, n32) = _check_stage2(engine, orc, calls)
    assert (n16, n32) == (len(calls), 0)


def test_gpu_seeding_order_wide_span(engine):
    """A chunk of 64 query positions whose slices span well over a thousand table entries: the query runs through
    a tandem stretch that stands in the window some forty times over, so every position of it holds ~40 hits
    (also past 4 inside the active range)."""
    rng = np.random.default_rng(501)
    g = _genome(rng, 16000)
    unit = bytes(_genome(rng, 37))
    start, loc = 2000, 4000
    g[loc + 60:loc + 60 + 37 * 40] = unit * 40
    locus = bytes(g[loc:loc + 300])
    calls = _both_strands([_window_call(g, start, 4000, _mutate(rng, locus, 0.01))])
    g = bytes(g)
    engine.set_genome(g)
    orc = Oracle()
    orc.set_genome(g)
    exp = _check_seeding(engine, orc, calls)
    assert sum(sorted(exp[0][1])[-64:]) > 1024
    _check_stage2(engine, orc, calls)


def test_gpu_seeding_order_plan_on_another_query(engine):
    """A stage-2 plan laid out from query arena A and run on arena B, where the middle call's read begins with
    150 nt of a tandem unit its window holds 900 nt of (hundreds of hits more than A's measured hit list and
    table): that call reports overflow as a status (-2), and its neighbours in the batch equal the oracle on
    B -- nothing was written outside the call's slices."""
    rng = np.random.default_rng(601)
    g = _genome(rng, 20000)
    calls, units = [], []
    for k in range(3):
        start = 1000 + 6000 * k
        unit = bytes(_genome(rng, 9))
        g[start + 300:start + 1200] = (unit * 100)[:900]
        loc = start + 1800
        calls.append(dict(_window_call(g, start, 3000, _mutate(rng, bytes(g[loc:loc + 250]))), splicingp=1,
                          maxintronlen=500000))
        units.append(unit)
    g = bytes(g)
    engine.set_genome(g)
    orc = Oracle()
    orc.set_genome(g)
    probs, qb, qub = gmapdp.Engine.build_stage2_batch(calls)
    qa = bytearray(qub)
    o = int(probs[1]["qoff"])
    qa[o:o + 150] = (units[1] * 17)[:150]
    qb2 = bytes(qa)
    exp = oracle_stage2_batch(orc, probs, qb2, qb2, nthreads=4)
    res, paths, pairs, _ = engine.stage2_plan_raw(probs, qub, qub, run_qbuf=qb2, run_qucbuf=qb2)
    assert int(res[1]["status"]) == -2, res["status"]
    bad = stage2_mismatches(res[[0, 2]], paths, pairs, exp, index=[0, 2])
    assert not bad, bad
