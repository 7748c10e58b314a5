"""Spot check of bench.py's own workload against the oracle (VERDICT r2 "the bench's outputs are never
checked"): the sub-problems of a bench read block -- generated exactly as bench.py generates them
(gmapdp.workload: packed genome, the stream's planted intron sites, block seeds) at the bench's real
universal coordinates -- run on the engine with the whole genome resident in HBM, and a 1 % sample of
every family (Dynprog_single_gap, _end5/3_gap, _genome_gap, _microexon_int, Stage2_compute) is compared
bit-exactly with the oracle run on the problem's chromosome alone (chroffset 0; outputs are
chromosome-relative, so only the addresses the kernels compute differ, as in test_gpu_large_coords.py).
The splice-site probabilities are GMAP's MaxEnt models as the bench computes them: on the device at the
universal coordinates (gmapdp.DEVICE), against the oracle's restatement on the chromosome alone -- so the
device MaxEnt is pinned past 2^31 (GRCh38) and past 2^32 (wheat) too.

configs[2]: block 0 of the default bench stream (GRCh38 layout, 3.09 Gnt, 10 000 reads, 8 blocks planted);
every one of its Stage2_compute calls through both engine paths (the batch API and the plan bench.py times).
configs[1]: block 0 of `bench.py --config 1` (chr22, single and end gaps only), a 5 % sample.
configs[4]: a 2 000-read block of the Iso-Seq stream on the 17-Gnt wheat layout (coordinates past 2^32),
sampled on its three smallest chromosomes."""
import random
import sys
import time

import numpy as np
import pytest

import gmapdp
from gmapdp import workload as W
import ctypes as C

from benchstep import oracle_dp_block as _oracle_dp_block
from benchstep import oracle_stage2_block as _oracle_stage2_block
from benchstep import stage2_problems as _stage2_problems
from dpbind import (Oracle, call_end, call_single, dp_batch_mismatches, microexon_probs, oracle_splice_probs,
                    stage2_mismatches)

pytestmark = pytest.mark.gpu
TAIL = 8192
T0 = time.perf_counter()


def _sample(n, frac, rng, allowed=None):
    idx = np.arange(n) if allowed is None else np.nonzero(allowed)[0]
    k = max(1, int(round(frac * n)))
    return np.sort(rng.choice(idx, size=min(k, len(idx)), replace=False)) if len(idx) else idx


def _progress(msg):
    sys.stderr.write("[bench-workload %.0fs] %s\n" % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def _block(layout, shape, reads, nblocks):
    genome = W.PackedGenome(layout.total, seed=38)
    _progress("genome %d nt" % layout.total)
    W.plant_stream(genome, layout, reads, range(nblocks), shape)
    _progress("planted")
    d = W.make_blocks(genome, layout, reads, [0], shape=shape, sprob=False)[0]
    _progress("block 0 generated")
    return genome, d


@pytest.fixture(scope="module")
def grch38_block0():
    """bench.py's configs[2] block 0 (the default stream: GRCh38 layout, 10 000 reads, 8 blocks planted)"""
    return _block(W.Layout(W.GRCH38), W.CDNA2K, 10000, 8)


def _run(layout, shape, reads, nblocks, chroms=None, frac=0.01, block=None):
    genome, d = block if block is not None else _block(layout, shape, reads, nblocks)
    eng = gmapdp.Engine(0)
    eng.set_genome(blocks=genome.blocks, length=genome.length)
    rng = np.random.default_rng(77)
    allow = None
    if chroms is not None:
        offs = set(int(layout.offsets[layout.names.index(c)]) for c in chroms)
        allow = lambda arr: np.isin(arr["chroffset"].astype(np.int64), list(offs))  # noqa: E731
    q = d["q"].tobytes()
    sp, ep, gp, mp, op = d["single"], d["end"], d["genome"], d["microexon"], d["oligo"]
    pick = {"single": _sample(len(sp), frac, rng, allow and allow(sp)),
            "end": _sample(len(ep), frac, rng, allow and allow(ep)),
            "genome": _sample(len(gp), frac, rng, allow and allow(gp)),
            "microexon": _sample(len(mp), frac, rng, allow and allow(mp)),
            "oligo": _sample(len(op), frac, rng, allow and allow(op))}

    def single_call(p):
        o, r = int(p["qoff"]), int(p["rlength"])
        f = int(p["flags"])
        return dict(q=q[o:o + r], quc=q[o:o + r], rlength=r, glength=int(p["glength"]), roffset=int(p["roffset"]),
                    goffset=int(p["goffset"]), chroffset=int(p["chroffset"]), chrhigh=int(p["chrhigh"]),
                    watsonp=f & 1, genestrand=int(p["genestrand"]), jump_late_p=(f >> 1) & 1,
                    extraband=int(p["extraband"]), widebandp=(f >> 2) & 1, defect_rate=float(p["defect_rate"]),
                    dynprogindex=int(p["dynprogindex"]))

    def end_call(p):
        c = single_call(p)
        del c["widebandp"]
        c.update(end3p=int(p["end3p"]), endalign=int(p["endalign"]), require_pos_score_p=int(p["require_pos_score_p"]))
        return c

    def genome_call(p):
        o, r = int(p["qoff"]), int(p["rlength"])
        c = {k: int(p[k]) for k in ("rlength", "glengthL", "glengthR", "roffset", "goffsetL", "rev_goffsetR",
                                    "chroffset", "chrhigh", "flags", "cdna_direction", "genestrand", "extraband",
                                    "maxpeelback", "dynprogindex")}
        c.update(q=q[o:o + r], quc=q[o:o + r], defect_rate=float(p["defect_rate"]))
        return c

    def mx_call(p):
        o, r = int(p["qoff"]), int(p["rlength"])
        c = {k: int(p[k]) for k in ("rlength", "roffset", "goffsetL", "rev_goffsetR", "cdna_direction", "chroffset",
                                    "chrhigh", "watsonp", "genestrand", "dynprogindex")}
        c.update(q=q[o:o + r], quc=q[o:o + r])
        return c

    def s2_call(p):
        o, n = int(p["qoff"]), int(p["querylength"])
        s = d["oq"][o:o + n].tobytes()
        return dict(q=s, quc=s, chrstart=int(p["chrstart"]), chrend=int(p["chrend"]), chroffset=int(p["chroffset"]),
                    chrhigh=int(p["chrhigh"]), plusp=int(p["plusp"]), splicingp=1, maxintronlen=500000)

    calls = {"single": [single_call(sp[i]) for i in pick["single"]], "end": [end_call(ep[i]) for i in pick["end"]],
             "genome": [genome_call(gp[i]) for i in pick["genome"]], "microexon": [mx_call(mp[i]) for i in pick["microexon"]],
             "oligo": [s2_call(op[i]) for i in pick["oligo"]]}
    # the engine, at universal coordinates (MaxEnt on the device)
    got = {"single": eng.single_gap_batch(calls["single"]), "end": eng.end_gap_batch(calls["end"]),
           "genome": eng.genome_gap_batch(calls["genome"], gmapdp.DEVICE),
           "microexon": eng.microexon_batch(calls["microexon"], gmapdp.DEVICE),
           "oligo": eng.stage2_batch(calls["oligo"])}
    eng.close()
    # the oracle, chromosome by chromosome
    orc = Oracle()
    bad = {k: [] for k in calls}
    byc = {}
    for fam, lst in calls.items():
        for k, c in enumerate(lst):
            byc.setdefault((c["chroffset"], c["chrhigh"]), []).append((fam, k))
    for (cho, chh), items in sorted(byc.items()):
        orc.set_genome(genome.ascii(cho, min(genome.length, chh + TAIL)))
        for fam, k in items:
            c = dict(calls[fam][k], chroffset=0, chrhigh=chh - cho)
            if fam == "single":
                exp = call_single(orc, c)
            elif fam == "end":
                exp = call_end(orc, c)
            elif fam == "genome":
                exp = orc.genome_gap(c, *oracle_splice_probs(orc, c))
            elif fam == "microexon":
                cands = orc.microexon_candidates(c) or []
                exp = orc.microexon_int(c, microexon_probs(orc, cands, 0))
            else:
                exp = orc.stage2_compute(c)
            if got[fam][k] != exp:
                bad[fam].append(int(pick[fam][k]))
    sizes = {k: len(v) for k, v in calls.items()}
    assert not any(bad.values()), "bench-workload problems differ from the oracle: %s of %s" % (
        {k: v[:8] for k, v in bad.items() if v}, sizes)
    return sizes, got


def test_gpu_bench_configs2_block_sample(grch38_block0):
    sizes, got = _run(W.Layout(W.GRCH38), W.CDNA2K, 10000, 8, block=grch38_block0)
    assert sizes["single"] > 2000 and sizes["genome"] > 4000 and sizes["oligo"] >= 150
    assert sum(1 for r in got["oligo"] if r[0] > 0) > 0.9 * sizes["oligo"]     # the reads chain


def test_gpu_bench_configs1_block_sample():
    """configs[1] ("100k synthetic 2-kb cDNA vs human chr22, Dynprog_single + Dynprog_end only"): block 0 of
    `bench.py --config 1` (chr22 layout, 10 000 reads, the 10 blocks of a 100 k-read cycle planted), its
    single and end gaps only, a 5 % sample against the oracle (dynprog_single.c:429, dynprog_end.c:1294/1924)."""
    genome, d = _block(W.Layout(W.CHR22), W.CDNA2K, 10000, 10)
    for k in ("genome", "microexon", "oligo"):  # as bench.py --config 1 strips them
        d[k] = d[k][:0]
    sizes, got = _run(W.Layout(W.CHR22), W.CDNA2K, 10000, 10, frac=0.05, block=(genome, d))
    assert sizes["single"] > 9000 and sizes["end"] > 5000 and sizes["genome"] == sizes["oligo"] == 0
    assert sum(1 for r in got["single"] if r[1]) > 0.5 * sizes["single"]   # the fills emit pairs


def test_gpu_bench_configs2_stage2_every_call(grch38_block0):
    """Every Stage2_compute call of bench block 0 (15 850 calls over ~214-kb windows at GRCh38 coordinates),
    bit-exact against the oracle through both engine paths:
      - gmapdp_stage2_batch, the drop-in's synchronous API (its seeding arenas laid out from upper bounds:
        13.6 GB of table for this block, past 2^31 entries -- the mappings are relative to each call's table);
      - the device-resident plan bench.py times (gmapdp_stage2_plan_create: the sizing run, the arenas
        re-laid out from it, the calls with fewer than 2^16 hits moved to the 16-bit seeding counters;
        gmapdp_stage2_plan_run; gmapdp_stage2_plan_fetch);
    and the plan's compact path-pair stream (gmapdp_stage2_plan_compact_pairs) expands on the host to exactly
    the records gmapdp_stage2_plan_fetch returns."""
    genome, d = grch38_block0
    s2p = _stage2_problems(d)
    q = d["oq"].tobytes()
    exp = _oracle_stage2_block(genome, s2p, q)
    assert np.all(exp[0][:, 0] >= 0), "oracle errors"
    eng = gmapdp.Engine(0)
    eng.set_genome(blocks=genome.blocks, length=genome.length)
    try:
        res, paths, pairs = eng.stage2_batch_raw(s2p, q, q)
        _progress("gmapdp_stage2_batch done")
        bad = stage2_mismatches(res, paths, pairs, exp)
        assert not bad, "gmapdp_stage2_batch differs from the oracle on %d of %d calls: %s" % (len(bad), len(s2p), bad[:8])
        cmp = {}
        pres, ppaths, ppairs, (n16, n32) = eng.stage2_plan_raw(s2p, q, q, compact_out=cmp)
        _progress("stage-2 plan done (%d calls 16-bit, %d 32-bit)" % (n16, n32))
        bad = stage2_mismatches(pres, ppaths, ppairs, exp)
        assert not bad, "the stage-2 plan differs from the oracle on %d of %d calls: %s" % (len(bad), len(s2p), bad[:8])
        cnt = np.maximum(ppaths["npairs"].astype(np.int64), 0)
        idx = np.repeat(ppaths["pair_offset"], cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        assert len(idx) > 0 and np.array_equal(cmp["pairs"][idx], ppairs[idx]), \
            "the compact path-pair stream does not expand to the records"
        assert cmp["bytes"] <= cmp["bound"]
        _progress("compact path-pair stream: %d records in %d bytes" % (len(idx), cmp["bytes"]))
    finally:
        eng.close()
    # the bench's configuration: 214-kb windows (>= 2^16 starts) seeded with 16-bit counters after the re-layout
    win = (s2p["chrend"] - s2p["chrstart"]).astype(np.int64)
    assert (win >= 65536).mean() > 0.99 and n16 + n32 == len(s2p) and n16 > 0.99 * len(s2p)
    assert (res["status"] == 2).sum() > 0.9 * len(s2p) and res["nresults"].sum() >= len(s2p)


def test_gpu_bench_configs4_block_sample():
    lay = W.Layout(W.WHEAT17)
    small = [lay.names[i] for i in np.argsort(lay.lens)[:3]]
    sizes, got = _run(lay, W.ISOSEQ5K, 2000, 1, chroms=small, frac=0.05)
    assert sizes["oligo"] >= 5 and sizes["genome"] > 100
    assert sum(1 for r in got["oligo"] if r[0] > 0) > 0.8 * sizes["oligo"]


def _dp_plan_block(eng, d, compact=False):
    """bench.py's DP path over block d: gmapdp_plan_create_all (single, end and genome gaps), the device
    MaxEnt bound (gmapdp_plan_bind_genome_maxent), gmapdp_plan_run; the microexon plan (search, device
    MaxEnt, finish).  Returns {family: (results in problem order, the pair arena)}."""
    lib = eng.lib
    hip = gmapdp._hip()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    bufs = []

    def dbuf(nbytes, src=None):
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), max(int(nbytes), 16)) == 0
        bufs.append(ptr)
        if src is not None:
            assert hip.hipMemcpy(ptr, src.ctypes.data, int(nbytes), 1) == 0
        return ptr

    def down(dst, ptr):
        assert hip.hipMemcpy(dst.ctypes.data, ptr, dst.nbytes, 2) == 0
        return dst

    sp, ep, gp, mp = d["single"], d["end"], d["genome"], d["microexon"]
    out = {}
    try:
        q = d["q"]
        d_q = dbuf(len(q), q)
        host_res = np.zeros(len(sp) + len(ep), dtype=gmapdp.RESULT_DTYPE)
        host_gres = np.zeros(max(len(gp), 1), dtype=gmapdp.GENOME_RESULT_DTYPE)
        plan = C.c_void_p()
        eng._check(lib.gmapdp_plan_create_all(eng.h, sp.ctypes.data, len(sp), ep.ctypes.data, len(ep), gp.ctypes.data,
                                              len(gp), host_res.ctypes.data, host_gres.ctypes.data, C.byref(plan)),
                   "gmapdp_plan_create_all")
        try:
            ngpu, nggpu = lib.gmapdp_plan_gpu_problems(plan), lib.gmapdp_plan_genome_gpu_problems(plan)
            cap = lib.gmapdp_plan_pair_capacity(plan)
            d_res = dbuf(32 * max(ngpu, 1))
            d_gres = dbuf(gmapdp.GENOME_RESULT_DTYPE.itemsize * max(nggpu, 1))
            d_pairs = dbuf(16 * max(cap, 1))
            m = int((gp["prob_offset"] + gp["glengthL"] + gp["glengthR"]).max()) if len(gp) else 1
            d_sprob = dbuf(8 * max(m, 1))
            eng._check(lib.gmapdp_plan_bind_genome_maxent(eng.h, plan, d_sprob, d_gres), "bind_genome_maxent")
            eng._check(lib.gmapdp_plan_run(eng.h, plan, d_q, d_q, d_res, d_pairs, None), "gmapdp_plan_run")
            assert hip.hipDeviceSynchronize() == 0
            dres = down(np.zeros(max(ngpu, 1), dtype=gmapdp.RESULT_DTYPE), d_res)
            dgres = down(np.zeros(max(nggpu, 1), dtype=gmapdp.GENOME_RESULT_DTYPE), d_gres)
            pairs = down(np.zeros(max(cap, 1), dtype=gmapdp.PAIR_DTYPE), d_pairs)
            res = host_res.copy()
            di = np.array([lib.gmapdp_plan_dev_index(plan, i) for i in range(len(res))], dtype=np.int64)
            res[di >= 0] = dres[di[di >= 0]]
            gres = host_gres[:len(gp)].copy()
            gi = np.array([lib.gmapdp_plan_genome_dev_index(plan, j) for j in range(len(gp))], dtype=np.int64)
            gres[gi >= 0] = dgres[gi[gi >= 0]]
            out["single"] = (res[:len(sp)], pairs)
            out["end"] = (res[len(sp):], pairs)
            out["genome"] = (gres, pairs)
            if compact:  # the compact pair stream, expanded on the host (gmapdp_plan_compact_pairs / _expand)
                nprob = ngpu + nggpu
                d_off = dbuf(8 * (nprob + 1))
                eng._check(lib.gmapdp_plan_compact_pairs(eng.h, plan, d_res, d_pairs, None, d_off, None), "compact")
                assert hip.hipDeviceSynchronize() == 0
                offs = down(np.zeros(nprob + 1, dtype=np.uint64), d_off)
                assert int(offs[-1]) <= lib.gmapdp_plan_compact_bound(plan)
                d_out = dbuf(int(offs[-1]))
                eng._check(lib.gmapdp_plan_compact_pairs(eng.h, plan, d_res, d_pairs, d_out, d_off, None), "compact")
                assert hip.hipDeviceSynchronize() == 0
                stream = down(np.zeros(max(int(offs[-1]), 1), dtype=np.uint8), d_out)
                npc = np.concatenate([dres["npairs"][:ngpu], dgres["npairs"][:nggpu]])
                poff = np.concatenate([dres["pair_offset"][:ngpu], dgres["pair_offset"][:nggpu]]).astype(np.int64)
                out["compact"] = (gmapdp.expand_pairs(stream, offs, npc, poff, cap), npc, poff, int(offs[-1]))
        finally:
            lib.gmapdp_plan_destroy(plan)
        if len(mp):
            mplan = C.c_void_p()
            eng._check(lib.gmapdp_microexon_plan_create(eng.h, mp.ctypes.data, len(mp), q.ctypes.data, q.ctypes.data,
                                                        len(q), C.byref(mplan)), "gmapdp_microexon_plan_create")
            try:
                mcap = lib.gmapdp_microexon_plan_pair_capacity(mplan)
                d_mres = dbuf(gmapdp.MICROEXON_RESULT_DTYPE.itemsize * len(mp))
                d_mpairs = dbuf(16 * max(mcap, 1))
                eng._check(lib.gmapdp_microexon_plan_run(eng.h, mplan, d_q, d_q, None, d_mres, d_mpairs, 3, None),
                           "gmapdp_microexon_plan_run")
                assert hip.hipDeviceSynchronize() == 0
                out["microexon"] = (down(np.zeros(len(mp), dtype=gmapdp.MICROEXON_RESULT_DTYPE), d_mres),
                                    down(np.zeros(max(mcap, 1), dtype=gmapdp.PAIR_DTYPE), d_mpairs))
            finally:
                lib.gmapdp_microexon_plan_destroy(mplan)
    finally:
        for b in bufs:
            hip.hipFree(b)
    return out


def _dp_every_call(genome, d, simd):
    fams = ("single", "end", "genome") + (() if simd else ("microexon",))
    if simd:
        d = dict(d)
        for fam in ("single", "end", "genome"):
            d[fam] = d[fam].copy()
            d[fam]["flags"] |= gmapdp.SIMD
    eng = gmapdp.Engine(0)
    eng.set_genome(blocks=genome.blocks, length=genome.length)
    try:
        got = _dp_plan_block(eng, d, compact=True)
    finally:
        eng.close()
    _progress("engine: the block's DP plan%s" % (" (SIMD semantics)" if simd else ""))
    # the compact pair stream expands to exactly the records the kernels wrote (every GPU problem's range)
    exp_pairs, npc, poff, nbytes = got["compact"]
    pairs = got["single"][1]
    cnt = np.maximum(npc.astype(np.int64), 0)
    idx = np.repeat(poff, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    assert np.array_equal(exp_pairs[idx], pairs[idx]), "the compact pair stream does not expand to the records"
    _progress("compact stream: %d records in %d bytes (%.2f B per record)" % (len(idx), nbytes, nbytes / max(len(idx), 1)))
    assert nbytes < 0.25 * 16 * len(idx)
    exp = _oracle_dp_block(genome, d, fams, simd=simd)
    bad = {}
    for fam in fams:
        res, pairs = got[fam]
        b = dp_batch_mismatches(fam, res, pairs, exp[fam])
        if b:
            bad[fam] = b[:8]
    sizes = {fam: len(d[fam]) for fam in fams}
    assert not bad, "bench block 0: calls differ from the oracle: %s of %s" % (bad, sizes)
    return sizes, got


def test_gpu_bench_configs2_dp_every_call(grch38_block0):
    """Every Dynprog_single_gap, _end5/3_gap, _genome_gap and _microexon_int call of bench block 0 (configs[2],
    GRCh38 coordinates; dynprog_single.c:429, dynprog_end.c:1294/1924, dynprog_genome.c:3288,
    dynprog_single.c:900) through the plan path bench.py times (device MaxEnt), bit-exact against the
    oracle's batch runner (orc_dp_batch, oracle MaxEnt) -- VERDICT r5 item 2: the whole block, not a sample."""
    genome, d = grch38_block0
    sizes, got = _dp_every_call(genome, d, simd=False)
    assert sizes["single"] > 150000 and sizes["genome"] > 400000 and sizes["microexon"] > 50000
    assert (got["genome"][0]["npairs"] > 0).mean() > 0.9


def test_gpu_bench_configs2_simd_every_call(grch38_block0):
    """`bench.py --simd` on bench block 0: every single, end and genome gap with the SIMD builds' semantics
    (gmap.avx2: sx_kernel, uxe_kernel, uxg_kernel; dynprog_simd.c) at GRCh38 coordinates against the oracle's
    S semantics (orc_set_simd 1)."""
    genome, d = grch38_block0
    sizes, got = _dp_every_call(genome, d, simd=True)
    assert sizes["genome"] > 400000
