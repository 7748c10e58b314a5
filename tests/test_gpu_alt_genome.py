"""The alternate-allele genome (gmap --use-snps) on the GPU: Dynprog_single_gap / Dynprog_end5_gap /
Dynprog_end3_gap under gmapdp_set_genome_alt against what the reference's own objects gave for the same calls
(tests/golden/alt_*_golden.npz), through every entry point that shares the classification; identity with
alt == ref over the existing goldens; the launch classes before, under and after a binding; the compact pair
stream's escape for genomealt != genome; and the refusals of every other family.  Bar: bit-exact."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import altsnp
import gmapdp
import pcstream

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, ENOGENOME = -1, -5
K_DPX, K_ROWS, K_ALT = 2, 7, 8  # gmapdp_plan_launch_kind: the packed narrow class, the rows layout, dpa_kernel


@pytest.fixture(scope="module")
def gold():
    """(ref, alt, single calls, single outputs, end calls, end outputs), loaded once and left unchanged."""
    ref, alt, sc, so = altsnp.load(altsnp.GOLDEN_SINGLE)
    ref2, alt2, ec, eo = altsnp.load(altsnp.GOLDEN_END)
    assert (ref, alt) == (ref2, alt2)
    return ref, alt, sc, so, ec, eo


@pytest.fixture(scope="module")
def engines(gold):
    """mode -> a context with the SNP genome pair bound."""
    ref, alt = gold[0], gold[1]
    es = {}
    for mode in (0, 1):
        e = gmapdp.Engine(0, mode=mode)
        e.set_genome(ref)
        e.set_genome_alt(alt)
        es[mode] = e
    yield es
    for e in es.values():
        e.close()


def _first_diff(got, exp):
    assert len(got) == len(exp)
    for i, (a, b) in enumerate(zip(got, exp)):
        if a != b:
            return i, a, b
    return None


def _assert_same(got, exp, what):
    d = _first_diff(got, exp)
    assert d is None, "%s: call %d: gpu %s vs reference %s" % (what, d[0], d[1], d[2])


def _one_arena(eng, singles, ends):
    """The singles' and ends' descriptors over one query arena."""
    S, sq, squ = eng.build_single_batch(singles)
    E, eq, equ = eng.build_end_batch(ends)
    if not len(singles):
        sq = squ = b""
    E["qoff"] += len(sq)
    return S, E, sq + eq, squ + equ


def _dynprog_batch(eng, singles, ends):
    lib = eng.lib
    S, E, q, qu = _one_arena(eng, singles, ends)
    n = len(S) + len(E)
    cap = (lib.gmapdp_single_pair_capacity(S.ctypes.data, len(S)) + lib.gmapdp_end_pair_capacity(E.ctypes.data, len(E)))
    res = np.zeros(max(n, 1), dtype=gmapdp.RESULT_DTYPE)
    gres = np.zeros(1, dtype=gmapdp.GENOME_RESULT_DTYPE)
    pairs = np.zeros(max(cap, 1), dtype=gmapdp.PAIR_DTYPE)
    rc = lib.gmapdp_dynprog_batch(eng.h, S.ctypes.data, len(S), E.ctypes.data, len(E), None, 0, q, qu, len(q), None, 0,
                                  res.ctypes.data, gres.ctypes.data, pairs.ctypes.data, cap)
    eng._check(rc, "gmapdp_dynprog_batch")
    return gmapdp.decode_results(res[:n], pairs, [p["dynprogindex"] for p in singles + ends])


class Plan:
    """gmapdp_plan_create over singles + ends, and its device-resident run."""

    def __init__(self, eng, singles, ends):
        self.eng, self.calls = eng, singles + ends
        self.S, self.E, self.q, self.qu = _one_arena(eng, singles, ends)
        self.host = np.zeros(max(len(self.calls), 1), dtype=gmapdp.RESULT_DTYPE)
        self.plan = C.c_void_p()
        eng._check(eng.lib.gmapdp_plan_create(eng.h, self.S.ctypes.data, len(self.S), self.E.ctypes.data, len(self.E),
                                              self.host.ctypes.data, C.byref(self.plan)), "gmapdp_plan_create")

    def kinds(self):
        lib = self.eng.lib
        return sorted(lib.gmapdp_plan_launch_kind(self.plan, li) for li in range(lib.gmapdp_plan_nlaunches(self.plan)))

    def run_rc(self, dev):
        """(return code, device results, pair arena) of gmapdp_plan_run on buffers of `dev`."""
        lib = self.eng.lib
        self.ngpu, self.cap = lib.gmapdp_plan_gpu_problems(self.plan), lib.gmapdp_plan_pair_capacity(self.plan)
        d_q = dev.up(np.frombuffer(self.q, dtype=np.uint8))
        d_qu = dev.up(np.frombuffer(self.qu, dtype=np.uint8))
        self.d_res = dev.alloc(32 * max(self.ngpu, 1), fill=0)
        self.d_pairs = dev.alloc(16 * max(self.cap, 1), fill=0)
        rc = lib.gmapdp_plan_run(self.eng.h, self.plan, d_q, d_qu, self.d_res, self.d_pairs, None)
        dev.sync()
        return rc

    def run(self, dev):
        """Per call (scalars, pairs-or-None); also the raw results (problem order) and the pair arena."""
        lib = self.eng.lib
        self.eng._check(self.run_rc(dev), "gmapdp_plan_run")
        dres = dev.down(self.d_res, 32 * max(self.ngpu, 1), gmapdp.RESULT_DTYPE)
        pairs = dev.down(self.d_pairs, 16 * max(self.cap, 1), gmapdp.PAIR_DTYPE)
        res = self.host[:len(self.calls)].copy()
        di = np.array([lib.gmapdp_plan_dev_index(self.plan, i) for i in range(len(res))], dtype=np.int64)
        res[di >= 0] = dres[di[di >= 0]]
        self.dres, self.pairs = dres, pairs
        return gmapdp.decode_results(res, pairs, [p["dynprogindex"] for p in self.calls])

    def close(self):
        self.eng.lib.gmapdp_plan_destroy(self.plan)


# ---- 1. every golden call, every result and pair field, through every entry point ----

@pytest.mark.parametrize("mode,tag", [(0, "ref_alt"), (1, "ref_alt_mode1")])
def test_gpu_alt_batches_match_the_reference(gold, engines, mode, tag):
    _, _, sc, so, ec, eo = gold
    eng = engines[mode]
    assert eng.has_genome_alt()
    _assert_same(eng.single_gap_batch(sc), so[tag], "gmapdp_single_gap_batch")
    _assert_same(eng.end_gap_batch(ec), eo[tag], "gmapdp_end_gap_batch")
    # a batch below the latency threshold takes the latency-mode classes
    _assert_same(eng.single_gap_batch(sc[:100]), so[tag][:100], "gmapdp_single_gap_batch (small batch)")


@pytest.mark.parametrize("mode,tag", [(0, "ref_alt"), (1, "ref_alt_mode1")])
def test_gpu_alt_dynprog_batch_matches_the_reference(gold, engines, mode, tag):
    _, _, sc, so, ec, eo = gold
    _assert_same(_dynprog_batch(engines[mode], sc, ec), so[tag] + eo[tag], "gmapdp_dynprog_batch")


@pytest.mark.parametrize("mode,tag", [(0, "ref_alt"), (1, "ref_alt_mode1")])
def test_gpu_alt_plan_matches_the_reference(gold, engines, mode, tag):
    _, _, sc, so, ec, eo = gold
    # (replicated past the latency threshold so that the plan takes the throughput classes)
    plan = Plan(engines[mode], sc * 2, ec * 2)
    try:
        kinds = plan.kinds()
        assert kinds and set(kinds) == {K_ALT}
        lib = engines[mode].lib
        dl = set()
        for li in range(lib.gmapdp_plan_nlaunches(plan.plan)):
            v = C.c_int()
            lib.gmapdp_plan_launch_info(plan.plan, li, None, C.byref(v), None, None)
            dl.add(v.value)
        assert dl == {0, 1}, "both direction placements (LDS and the global scratch) must occur"
        with pcstream.Device() as dev:
            got = plan.run(dev)
    finally:
        plan.close()
    _assert_same(got, (so[tag] * 2) + (eo[tag] * 2), "gmapdp_plan_create + gmapdp_plan_run")


# ---- 2. identity: an alternate genome equal to the primary one changes nothing ----

def _existing(name):
    return altsnp._make_golden().load(os.path.join(HERE, "golden", name))


@pytest.mark.parametrize("mode", [0, 1])
def test_gpu_alt_equal_to_ref_is_the_identity(mode):
    g, sp, _ = _existing("single_gap_golden.npz")
    g2, ep, _ = _existing("end_gap_golden.npz")
    eng = gmapdp.Engine(0, mode=mode)
    try:
        for genome, run, probs in ((g, eng.single_gap_batch, sp), (g2, eng.end_gap_batch, ep)):
            eng.set_genome(genome)
            before = run(probs)
            eng.set_genome_alt(genome)
            assert eng.has_genome_alt()
            bound = run(probs)
            eng.clear_genome_alt()
            d = _first_diff(bound, before)
            assert d is None, "call %d: bound %s vs unbound %s" % d
            assert sum(1 for s, p in before if p is not None) > len(probs) // 2
    finally:
        eng.close()


# ---- 3. unbinding restores today's launches ----

def test_gpu_alt_unbinding_restores_the_launch_classes(gold):
    ref, alt, sc, so, ec, eo = gold
    eng = gmapdp.Engine(0)
    try:
        eng.set_genome(ref)

        def kinds():
            p = Plan(eng, sc * 2, ec * 2)
            try:
                lib = eng.lib
                return sorted((lib.gmapdp_plan_launch_kind(p.plan, li),) + _info(lib, p.plan, li)
                              for li in range(lib.gmapdp_plan_nlaunches(p.plan)))
            finally:
                p.close()
        before = kinds()
        assert {k[0] for k in before} >= {K_DPX, K_ROWS}, "the unbound plan should use the packed and rows classes"
        eng.set_genome_alt(alt)
        bound = kinds()
        assert {k[0] for k in bound} == {K_ALT}
        eng.clear_genome_alt()
        assert not eng.has_genome_alt()
        assert kinds() == before
        # a new primary genome drops the alternate one
        eng.set_genome_alt(alt)
        eng.set_genome(ref)
        assert not eng.has_genome_alt()
    finally:
        eng.close()


def _info(lib, plan, li):
    R, dl, cnt, lds = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    assert lib.gmapdp_plan_launch_info(plan, li, C.byref(R), C.byref(dl), C.byref(cnt), C.byref(lds)) == 0
    return R.value, dl.value, cnt.value, lds.value


# ---- 4. the compact pair stream carries genomealt ----

def test_gpu_alt_pairs_survive_the_compact_stream(gold, engines):
    _, _, sc, so, ec, eo = gold
    eng = engines[0]
    plan = Plan(eng, sc, ec)
    try:
        with pcstream.Device() as dev:
            plan.run(dev)
            dres, arena = plan.dres[:plan.ngpu], plan.pairs
    finally:
        plan.close()
    stream, offs, intact = pcstream.compact_pairs(eng, dres, np.zeros(0, dtype=gmapdp.GENOME_RESULT_DTYPE), arena)
    assert intact
    lists = [arena[int(r["pair_offset"]):int(r["pair_offset"]) + max(int(r["npairs"]), 0)] for r in dres]
    want, woffs = pcstream.encode(lists)
    assert stream == want and np.array_equal(offs, woffs)
    back = gmapdp.expand_pairs(np.frombuffer(stream, dtype=np.uint8), offs, dres["npairs"],
                               dres["pair_offset"].astype(np.int64), len(arena))
    for r, lst in zip(dres, lists):
        o, n = int(r["pair_offset"]), max(int(r["npairs"]), 0)
        assert back[o:o + n].tobytes() == lst.tobytes()
    # records escaped for no other reason than genomealt != genome
    alt_escapes = 0
    for lst in lists:
        raw = lst.tobytes()
        for i in range(len(lst)):
            ch = raw[16 * i + 12:16 * i + 16]
            if lst["querypos"][i] >= 0 and pcstream._code(ch) is None and pcstream._code(ch[:3] + ch[2:3]) is not None:
                alt_escapes += 1
    assert alt_escapes >= 1


# ---- 5. refusals ----

def _refused(eng, fn, family):
    with pytest.raises(gmapdp.GmapdpError) as e:
        fn()
    msg = str(e.value)
    assert "(%d)" % EINVAL in msg, "%s: %s" % (family, msg)
    assert "alternate" in msg and len(msg) > 40, "%s: %s" % (family, msg)


def test_gpu_alt_refusals(gold):
    import s2x
    from dpbind import (cdna_gap_problem, genome_gap_problem, microexon_problem, oligo_problem, random_genome,
                        splicejunction_problem, stage2_problem)
    ref, alt, sc, so, ec, eo = gold
    rng = random.Random(5)
    gg = bytearray(random_genome(rng, 400000))
    gps = [genome_gap_problem(rng, gg) for _ in range(4)]
    at = [100]
    mxs = [microexon_problem(rng, gg, at=at) for _ in range(4)]
    g = bytes(gg)
    alt_g = bytes(g[:1000] + bytes(b"ACGT"[(b"ACGT".find(bytes([c])) + 1) % 4] if c in b"ACGT" else c
                                   for c in g[1000:1200]) + g[1200:])
    sp = [([0.5] * max(0, p["glengthL"]), [0.5] * max(0, p["glengthR"])) for p in gps]
    cps = [cdna_gap_problem(rng, g) for _ in range(4)]
    sjs = [splicejunction_problem(rng, g) for _ in range(4)]
    ops = [oligo_problem(rng, g) for _ in range(4)]
    s2s = [stage2_problem(rng, g) for _ in range(2)]
    simd_single = [dict(sc[0], simd=True)]
    simd_end = [dict(next(p for p in ec if p["rlength"] > 0 and p["glength"] >= p["rlength"] and p["goffset"] > 100
                          and p["endalign"] != 2), simd=True)]
    eng = gmapdp.Engine(0)
    try:
        eng.set_genome(g)
        S, sq, squ = eng.build_single_batch(sc[:4])
        G, gq, gqu, nprob = gmapdp.build_genome_batch(gps)
        XS, xq, xqu = eng.build_microexon_batch(mxs)
        pos = np.array([5000, 6000], dtype=np.uint64)

        def mixed():
            rc, _ = eng.mixed_batch_raw(sq, squ, singles=S)
            eng._check(rc, "gmapdp_mixed_batch")

        def genome_plan():
            res = np.zeros(1, dtype=gmapdp.RESULT_DTYPE)
            gres = np.zeros(len(G), dtype=gmapdp.GENOME_RESULT_DTYPE)
            plan = C.c_void_p()
            rc = eng.lib.gmapdp_plan_create_all(eng.h, None, 0, None, 0, G.ctypes.data, len(G), res.ctypes.data,
                                                gres.ctypes.data, C.byref(plan))
            if rc == 0:
                eng.lib.gmapdp_plan_destroy(plan)
            eng._check(rc, "gmapdp_plan_create_all")

        def genome_dynprog():
            res = np.zeros(1, dtype=gmapdp.RESULT_DTYPE)
            gres = np.zeros(len(G), dtype=gmapdp.GENOME_RESULT_DTYPE)
            cap = eng.lib.gmapdp_genome_pair_capacity(G.ctypes.data, len(G))
            pairs = np.zeros(max(cap, 1), dtype=gmapdp.PAIR_DTYPE)
            arena = np.full(max(nprob, 1), 0.5)
            eng._check(eng.lib.gmapdp_dynprog_batch(eng.h, None, 0, None, 0, G.ctypes.data, len(G), gq, gqu, len(gq),
                                                    arena.ctypes.data, nprob, res.ctypes.data, gres.ctypes.data,
                                                    pairs.ctypes.data, cap), "gmapdp_dynprog_batch")

        def scan_plan():
            with eng.scan_plan(*eng.build_scan_batch(ops)) as sp_:
                sp_.run()

        families = [
            ("GMAPDP_SIMD single gap", lambda: eng.single_gap_batch(simd_single)),
            ("GMAPDP_SIMD end gap", lambda: eng.end_gap_batch(simd_end)),
            ("gmapdp_genome_gap_batch", lambda: eng.genome_gap_batch(gps, sp)),
            ("gmapdp_genome_gap_batch_known", lambda: eng.genome_gap_batch_known(gps, sp, [None] * len(gps))),
            ("gmapdp_dynprog_batch with genome gaps", genome_dynprog),
            ("plans with genome gaps", genome_plan),
            ("gmapdp_cdna_gap_batch", lambda: eng.cdna_gap_batch(cps)),
            ("gmapdp_end_splicejunction_batch", lambda: eng.end_splicejunction_batch(sjs)),
            ("gmapdp_microexon_search", lambda: eng.microexon_search_raw(XS, xq, xqu)),
            ("gmapdp_microexon_whole", lambda: eng.microexon_whole_batch(mxs)),
            ("gmapdp_mixed_batch", mixed),
            ("gmapdp_maxent_sites", lambda: eng.maxent_sites(pos, [1, 2], 0)),
            ("gmapdp_canonical_links", lambda: eng.canonical_links(pos, pos + 500, 1, 0, len(g))),
            ("gmapdp_oligo_mappings_batch", lambda: eng.oligo_mappings_batch(ops)),
            ("gmapdp_oligo_plan", lambda: eng.oligo_plan_batch(ops)),
            ("gmapdp_scan_plan", scan_plan),
            ("gmapdp_stage2_scan_batch", lambda: eng.stage2_scan_batch(ops)),
            ("gmapdp_stage2_batch", lambda: eng.stage2_batch(s2s)),
            ("gmapdp_stage2_plan", lambda: eng.stage2_plan_raw(*eng.build_stage2_batch(s2s))),
            ("gmapdp_stage2x_batch", lambda: eng.stage2x_batch(s2x.random_calls(gmapdp.S2X_ONE, 2, seed=3), gmapdp.S2X_ONE)),
        ]
        eng.set_genome_alt(alt_g)
        for family, fn in families:
            _refused(eng, fn, family)
        eng.clear_genome_alt()
        for family, fn in families:
            if family == "gmapdp_stage2x_batch":
                eng.set_genome(s2x.genome())  # (its calls address tests/s2x.py's own genome)
            fn()  # the same call succeeds once the alternate genome is unbound
    finally:
        eng.close()


def test_gpu_alt_binding_errors_and_plans_across_a_changed_binding(gold):
    ref, alt, sc, so, ec, eo = gold
    lib = gmapdp.load_library()
    eng = gmapdp.Engine(0)
    try:
        blocks = gmapdp.pack_genome(alt)
        # no primary genome
        rc = lib.gmapdp_set_genome_alt(eng.h, blocks.ctypes.data, blocks.size, len(alt))
        assert rc == ENOGENOME and b"primary" in lib.gmapdp_last_error(eng.h)
        eng.set_genome(ref)
        # a wrong length, a wrong word count
        short = gmapdp.pack_genome(alt[:-40])
        assert lib.gmapdp_set_genome_alt(eng.h, short.ctypes.data, short.size, len(alt) - 40) == EINVAL
        assert b"length" in lib.gmapdp_last_error(eng.h)
        assert lib.gmapdp_set_genome_alt(eng.h, blocks.ctypes.data, blocks.size - 3, len(alt)) == EINVAL
        assert not eng.has_genome_alt()
        # a plan runs only under the binding it was made under
        unbound_plan = Plan(eng, sc[:40], ec[:40])
        eng.set_genome_alt(blocks=blocks)
        bound_plan = Plan(eng, sc[:40], ec[:40])
        try:
            with pcstream.Device() as dev:
                assert unbound_plan.run_rc(dev) == EINVAL
                assert b"alternate" in lib.gmapdp_last_error(eng.h)
                got = bound_plan.run(dev)
                eng.clear_genome_alt()
                assert bound_plan.run_rc(dev) == EINVAL
                assert b"alternate" in lib.gmapdp_last_error(eng.h)
                assert unbound_plan.run_rc(dev) == 0
        finally:
            unbound_plan.close()
            bound_plan.close()
        _assert_same(got, so["ref_alt"][:40] + eo["ref_alt"][:40], "bound plan")
        # a sharing context takes the owner's alternate genome, an HBM-resident one binds without a copy
        eng.set_genome_alt(blocks=blocks)
        other = gmapdp.Engine(0)
        try:
            other.share_genome(eng)
            assert other.has_genome_alt()
            _assert_same(other.single_gap_batch(sc[:60]), so["ref_alt"][:60], "shared alternate genome")
            dg = C.c_void_p()
            assert lib.gmapdp_dgenome_create(0, blocks.ctypes.data, blocks.size, len(alt), C.byref(dg)) == 0
            try:
                other.set_genome(ref)
                assert not other.has_genome_alt()
                assert lib.gmapdp_use_dgenome_alt(other.h, dg) == 0 and other.has_genome_alt()
                _assert_same(other.end_gap_batch(ec[:60]), eo["ref_alt"][:60], "gmapdp_use_dgenome_alt")
                assert lib.gmapdp_use_dgenome_alt(other.h, None) == 0 and not other.has_genome_alt()
            finally:
                other.close()
                lib.gmapdp_dgenome_destroy(dg)
        finally:
            other.close()
    finally:
        eng.close()
