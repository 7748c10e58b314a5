"""bench.py's block set-up and timed step, restated for tests (bench.py's `step` is a closure of main(), so
it cannot be imported).

Mirrors bench.py:
  * 525-603  per block: device arenas, the DP plan (gmapdp_plan_create_all), the stage-2 plan, the
             microexon plan, gmapdp_plan_bind_genome_maxent, each launch's stream from
             gmapdp_plan_launch_stream; the output arenas shared by the blocks;
  * 611-620  the four streams (main, two sides, stage 2) on a context made with CTX_TWO_SIDES;
  * 636-662  launch / orun / mrun;
  * 664-718  step (piped, GMAPDP_BENCH_PIPE in {0, 3}), without its timing events.

It differs from the bench in two ways:
  * every step may get its own output buffers (Bench.outputs(): d_res, d_gres, d_pairs, d_mres, d_mpairs,
    d_s2res), so a whole sequence of steps can be checked after one final synchronize.  The genome-gap
    results are bound to the plan (bench.py binds one buffer once, line 602), so step() binds the step's
    d_gres before it issues the launches: a host-side pointer the launches read when they are issued.
  * Bench.poison fills every output arena (and the splice-probability scratch) with 0xA5.

GMAPDP_BENCH_PIPE 1 and 2, the three-sides and stream-priority variants are not restated.

Also here: the bench-block oracle helpers shared with test_gpu_bench_workload.py (oracle_dp_block,
oracle_stage2_block, stage2_problems), oracle_block over both, the comparator step_mismatches, and the
blocks the step tests run (block200, blocks3), generated once per process."""
import ctypes as C
import functools
import sys
import time

import numpy as np

import gmapdp
from gmapdp import workload as W

from dpbind import (S2B_PATHS, Oracle, dp_batch_mismatches, oracle_dp_batch, oracle_stage2_batch,
                    stage2_mismatches)

TAIL = 8192
T0 = time.perf_counter()
POISON = 0xA5
DP_FAMS = ("single", "end", "genome", "microexon")


def _progress(msg):
    sys.stderr.write("[bench-block %.0fs] %s\n" % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


# ---------------------------------------------------------------------------------------------------
# the oracle over a bench block (shared with test_gpu_bench_workload.py)
# ---------------------------------------------------------------------------------------------------
def stage2_problems(d):
    op = d["oligo"]
    s2p = np.zeros(len(op), dtype=gmapdp.STAGE2_PROBLEM_DTYPE)
    for k in ("qoff", "querylength", "chrstart", "chrend", "chroffset", "chrhigh", "plusp"):
        s2p[k] = op[k]
    s2p["splicingp"] = 1       # GMAP's defaults, as bench.py passes them
    s2p["maxintronlen"] = 500000
    return s2p


def oracle_stage2_block(genome, s2p, q):
    """orc_stage2_batch over every call, chromosome by chromosome (the oracle holds one chromosome at
    chroffset 0; the outputs are chromosome-relative)."""
    orc = Oracle()
    n = len(s2p)
    scal = np.zeros((n, 8), dtype=np.int32)
    paths = np.zeros((n, S2B_PATHS, 2), dtype=np.int32)
    parts, off, base = [], np.zeros(n + 1, dtype=np.int64), 0
    for cho in sorted(set(int(x) for x in s2p["chroffset"])):
        idx = np.nonzero(s2p["chroffset"] == cho)[0]
        chh = int(s2p["chrhigh"][idx[0]])
        orc.set_genome(genome.ascii(cho, min(genome.length, chh + TAIL)))
        sub = s2p[idx].copy()
        sub["chroffset"] = 0
        sub["chrhigh"] = chh - cho
        sc, pa, pr, po = oracle_stage2_batch(orc, sub, q, q)
        _progress("oracle: %d calls at chroffset %d" % (len(idx), cho))
        scal[idx], paths[idx] = sc, pa
        off[idx] = base + po[:-1]
        parts.append(pr[:20 * int(po[-1])])
        base += int(po[-1])
    return scal, paths, np.concatenate(parts), off


def oracle_dp_block(genome, d, fams, simd=False):
    """orc_dp_batch over every call of the families, chromosome by chromosome (the oracle holds one
    chromosome at chroffset 0; outputs are chromosome-relative): {family: (scal, dscal, pairs, pair_off)}
    in problem order."""
    orc = Oracle(simd=simd)
    q = d["q"].tobytes()
    out = {}
    for fam in fams:
        p = d[fam]
        n = len(p)
        scal = np.zeros((n, 16), dtype=np.int32)
        dscal = np.zeros((n, 2), dtype=np.float64)
        parts, pair_off, base = [], np.zeros(n + 1, dtype=np.int64), 0
        order = np.zeros(n, dtype=np.int64)
        for cho in sorted(set(int(x) for x in p["chroffset"])):
            idx = np.nonzero(p["chroffset"] == cho)[0]
            chh = int(p["chrhigh"][idx[0]])
            orc.set_genome(genome.ascii(cho, min(genome.length, chh + TAIL)))
            sub = p[idx].copy()
            sub["chroffset"] = 0
            sub["chrhigh"] = chh - cho
            sc, ds, pr, po = oracle_dp_batch(orc, fam, sub, q, q)
            scal[idx], dscal[idx] = sc, ds
            pair_off[idx] = base + po[:-1]
            parts.append(pr[:int(po[-1])])
            base += int(po[-1])
            order[idx] = 1
        pair_off[n] = base
        out[fam] = (scal, dscal, np.concatenate(parts) if parts else np.zeros(1, dtype=gmapdp.PAIR_DTYPE), pair_off)
        _progress("oracle: every %s call (%d)" % (fam, n))
    return out


def with_simd(d):
    """The block as `bench.py --simd` runs it: GMAPDP_SIMD on every single, end and genome gap."""
    d = dict(d)
    for fam in ("single", "end", "genome"):
        d[fam] = d[fam].copy()
        d[fam]["flags"] |= gmapdp.SIMD
    return d


def oracle_block(genome, d, simd=False):
    """(what oracle_dp_block returns for the four DP families, what oracle_stage2_block returns) for block
    d.  simd: the SIMD builds' semantics for the single, end and genome gaps (d as with_simd made it); the
    microexon search and Stage2_compute have one semantics."""
    dp = oracle_dp_block(genome, d, ("single", "end", "genome"), simd=simd)
    dp.update(oracle_dp_block(genome, d, ("microexon",), simd=False))
    s2 = oracle_stage2_block(genome, stage2_problems(d), d["oq"].tobytes())
    return dp, s2


# ---------------------------------------------------------------------------------------------------
# the blocks of the step tests
# ---------------------------------------------------------------------------------------------------
def layout2():
    return W.Layout([("chrA", 2_500_000), ("chrB", 1_500_000)])


def make_stream(reads_per_block):
    """bench.py's make_stream on the two-chromosome layout: one genome with every block's intron sites
    planted (block k of the stream has reads_per_block[k] reads), then the blocks."""
    lay = layout2()
    genome = W.PackedGenome(lay.total, seed=38)
    for k, reads in enumerate(reads_per_block):
        W.plant_stream(genome, lay, reads, [k], W.CDNA2K)
    data = [W.make_blocks(genome, lay, reads, [k], shape=W.CDNA2K, sprob=False)[0]
            for k, reads in enumerate(reads_per_block)]
    return genome, data


@functools.lru_cache(maxsize=None)
def block200():
    """(genome, block): the 200-read CDNA2K block of the step tests"""
    genome, data = make_stream((200,))
    return genome, data[0]


@functools.lru_cache(maxsize=None)
def block200_oracle():
    return oracle_block(*block200())


@functools.lru_cache(maxsize=None)
def blocks3():
    """(genome, blocks): 120, 200 and 120 reads planted into one genome (the context's grow-only scratch is
    sized by a small block, grown by a larger one and reused by a smaller one)"""
    return make_stream((120, 200, 120))


@functools.lru_cache(maxsize=None)
def blocks3_oracle(simd=False):
    genome, data = blocks3()
    return [oracle_block(genome, with_simd(d) if simd else d, simd=simd) for d in data]


# ---------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------
def step_mismatches(got, oracle, stage2_paths=True):
    """got: one step's outputs as Bench.fetch returns them ({family: (results in problem order, pair arena)}
    for the DP families present, "stage2": (results, paths, pairs)); oracle: oracle_block's.  Returns
    [(family, call, what differs)].  stage2_paths False: the stage-2 result records only (an earlier run's
    paths are no longer in the plan's pools)."""
    dp, s2 = oracle
    bad = []
    for fam in DP_FAMS:
        if fam in got:
            res, pairs = got[fam]
            bad += [(fam, i, what) for i, what in dp_batch_mismatches(fam, res, pairs, dp[fam])]
    if "stage2" in got:
        res, paths, pairs = got["stage2"]
        bad += [("stage2", i, what) for i, what in stage2_mismatches(res, paths, pairs, s2,
                                                                     records_only=not stage2_paths)]
    return bad


def stage2_by_call(results, paths, pairs):
    """The stage-2 outputs independent of where the pools' atomic cursors put each call's records: per
    call (nresults, npaths, ncovered, status, query bounds, record count, [each path's pair bytes])."""
    pb = pairs.view(np.uint8).reshape(-1)
    out = []
    for r in results:
        lists = []
        for k in range(max(int(r["nresults"]), 0)):
            p = paths[int(r["path_offset"]) + k]
            lists.append(pb[20 * int(p["pair_offset"]):20 * (int(p["pair_offset"]) + int(p["npairs"]))].tobytes())
        out.append((int(r["nresults"]), int(r["npaths"]), int(r["ncovered"]), int(r["status"]),
                    int(r["diag_querystart"]), int(r["diag_queryend"]), int(r["npairs"]), lists))
    return out


# ---------------------------------------------------------------------------------------------------
# bench.py's set-up and step
# ---------------------------------------------------------------------------------------------------
class Bench:
    """bench.py:507-662 for the blocks `data` of one stream on `genome` (simd: `bench.py --simd`)."""

    def __init__(self, genome, data, simd=False, device=0):
        import torch
        self.torch = torch
        torch.cuda.set_device(device)
        self.dev = dev = torch.device("cuda", device)
        # the plans' launch classes over three streams (the caller's and two sides): stage 2 takes the fourth
        self.eng = eng = gmapdp.Engine(device, flags=gmapdp.CTX_TWO_SIDES)
        eng.set_genome(blocks=genome.blocks, length=genome.length)
        self.lib = lib = eng.lib
        self.B = []
        try:
            for bi, d in enumerate(data):
                self.B.append(self._block(bi, with_simd(d) if simd else d))
        except BaseException:
            self.close()
            raise
        mx = lambda k: max(b[k] for b in self.B)  # noqa: E731
        self.sizes = {
            "d_res": max(mx("ngpu"), 1) * 32, "d_gres": max(mx("nggpu"), 1) * 72, "d_pairs": max(mx("cap"), 1) * 16,
            # (one record per Stage2_compute call: a block has more calls than reads)
            "d_s2res": max(max(len(b["d"]["oligo"]) for b in self.B), 1) * gmapdp.STAGE2_RESULT_DTYPE.itemsize,
            "d_mres": max(max(len(b["d"]["microexon"]) for b in self.B), 1) * gmapdp.MICROEXON_RESULT_DTYPE.itemsize,
            "d_mpairs": max(mx("mcap"), 1) * 16}
        assert gmapdp.RESULT_DTYPE.itemsize == 32 and gmapdp.GENOME_RESULT_DTYPE.itemsize == 72
        assert gmapdp.PAIR_DTYPE.itemsize == 16
        self.stream = torch.cuda.Stream(dev)
        self.sides = [torch.cuda.Stream(dev) for _ in range(2)]
        self.ostream = torch.cuda.Stream(dev)
        self.sstream = self.ostream
        _ = lib

    def _block(self, bi, d):
        torch, eng, lib, dev = self.torch, self.eng, self.lib, self.dev
        sp, ep, gp, op, mp = d["single"], d["end"], d["genome"], d["oligo"], d["microexon"]
        blk = {"id": bi, "d": d, "ns": len(sp), "ne": len(ep), "ng": len(gp), "plan": None, "oplan": None,
               "mplan": None}
        blk["d_q"] = torch.from_numpy(d["q"]).to(dev)
        blk["d_oq"] = torch.from_numpy(d["oq"]).to(dev)
        # the genome gaps' splice-probability arena: scratch the device MaxEnt fills in the step
        blk["d_sprob"] = torch.zeros(max(d["sprob_len"], 1), dtype=torch.float64, device=dev)
        blk["host_res"] = np.zeros(len(sp) + len(ep), dtype=gmapdp.RESULT_DTYPE)
        blk["host_gres"] = np.zeros(max(len(gp), 1), dtype=gmapdp.GENOME_RESULT_DTYPE)
        plan = C.c_void_p()
        eng._check(lib.gmapdp_plan_create_all(eng.h, sp.ctypes.data, len(sp), ep.ctypes.data, len(ep),
                                              gp.ctypes.data, len(gp), blk["host_res"].ctypes.data,
                                              blk["host_gres"].ctypes.data, C.byref(plan)), "gmapdp_plan_create_all")
        blk["plan"] = plan
        s2p = stage2_problems(d)
        if len(s2p):
            oplan = C.c_void_p()
            eng._check(lib.gmapdp_stage2_plan_create(eng.h, s2p.ctypes.data, len(s2p), d["oq"].ctypes.data,
                                                     d["oq"].ctypes.data, len(d["oq"]), C.byref(oplan)),
                       "gmapdp_stage2_plan_create")
            blk["oplan"] = oplan
        if len(mp):
            mplan = C.c_void_p()
            eng._check(lib.gmapdp_microexon_plan_create(eng.h, mp.ctypes.data, len(mp), d["q"].ctypes.data,
                                                        d["q"].ctypes.data, len(d["q"]), C.byref(mplan)),
                       "gmapdp_microexon_plan_create")
            blk["mplan"] = mplan
        blk["ngpu"], blk["nggpu"] = lib.gmapdp_plan_gpu_problems(plan), lib.gmapdp_plan_genome_gpu_problems(plan)
        blk["cap"] = lib.gmapdp_plan_pair_capacity(plan)
        blk["mcap"] = lib.gmapdp_microexon_plan_pair_capacity(blk["mplan"]) if blk["mplan"] else 0
        nl = lib.gmapdp_plan_nlaunches(plan)
        blk["info"], blk["kinds"], blk["lstream"] = [], [], []
        for li in range(nl):
            R, dl, cnt, lds = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
            lib.gmapdp_plan_launch_info(plan, li, C.byref(R), C.byref(dl), C.byref(cnt), C.byref(lds))
            blk["info"].append((R.value, dl.value, cnt.value, lds.value))
            blk["kinds"].append(lib.gmapdp_plan_launch_kind(plan, li))
            blk["lstream"].append(lib.gmapdp_plan_launch_stream(plan, li))
        blk["dev_index"] = np.array([lib.gmapdp_plan_dev_index(plan, i) for i in range(len(sp) + len(ep))],
                                    dtype=np.int64)
        blk["gdev_index"] = np.array([lib.gmapdp_plan_genome_dev_index(plan, j) for j in range(len(gp))],
                                     dtype=np.int64)
        return blk

    def close(self):
        if self.eng is None:
            return
        self.torch.cuda.synchronize()
        for b in self.B:
            if b["plan"]:
                self.lib.gmapdp_plan_destroy(b["plan"])
            if b["oplan"]:
                self.lib.gmapdp_stage2_plan_destroy(b["oplan"])
            if b["mplan"]:
                self.lib.gmapdp_microexon_plan_destroy(b["mplan"])
        self.B = []
        self.eng.close()
        self.eng = None

    # -- output arenas -----------------------------------------------------------------------------
    def outputs(self, fill=0):
        """One set of output arenas (bench.py:592-600: sized for the largest block), every byte `fill`."""
        return {k: self.torch.full((n,), fill, dtype=self.torch.uint8, device=self.dev) for k, n in self.sizes.items()}

    def poison(self, out, b=None):
        """Every output arena of `out`, and block b's splice-probability scratch, filled with 0xA5; the
        device is synchronized after it, so that the fill precedes whatever the caller issues next."""
        for t in out.values():
            t.fill_(POISON)
        if b is not None:
            b["d_sprob"].view(self.torch.uint8).fill_(POISON)
        self.torch.cuda.synchronize()

    # -- bench.py:636-662 --------------------------------------------------------------------------
    def bind(self, b, out):
        self.eng._check(self.lib.gmapdp_plan_bind_genome_maxent(self.eng.h, b["plan"], C.c_void_p(b["d_sprob"].data_ptr()),
                                                                C.c_void_p(out["d_gres"].data_ptr())),
                        "gmapdp_plan_bind_genome_maxent")

    def launch(self, b, li, s, out, kernel_only=False):
        f = self.lib.gmapdp_plan_run_launch_kernel if kernel_only else self.lib.gmapdp_plan_run_launch
        self.eng._check(f(self.eng.h, b["plan"], li, C.c_void_p(b["d_q"].data_ptr()), C.c_void_p(b["d_q"].data_ptr()),
                          C.c_void_p(out["d_res"].data_ptr()), C.c_void_p(out["d_pairs"].data_ptr()),
                          C.c_void_p(s.cuda_stream)), "gmapdp_plan_run_launch")

    def plan_run(self, b, s, out):
        """gmapdp_plan_run: the engine's own schedule over the context's side streams"""
        self.eng._check(self.lib.gmapdp_plan_run(self.eng.h, b["plan"], C.c_void_p(b["d_q"].data_ptr()),
                                                 C.c_void_p(b["d_q"].data_ptr()), C.c_void_p(out["d_res"].data_ptr()),
                                                 C.c_void_p(out["d_pairs"].data_ptr()),
                                                 C.c_void_p(s.cuda_stream) if s is not None else None), "gmapdp_plan_run")

    def orun(self, b, s, what, out):
        self.eng._check(self.lib.gmapdp_stage2_plan_run(self.eng.h, b["oplan"], C.c_void_p(b["d_oq"].data_ptr()),
                                                        C.c_void_p(b["d_oq"].data_ptr()),
                                                        C.c_void_p(out["d_s2res"].data_ptr()), what,
                                                        C.c_void_p(s.cuda_stream)), "gmapdp_stage2_plan_run")

    def mrun(self, b, s, what, out):
        self.eng._check(self.lib.gmapdp_microexon_plan_run(self.eng.h, b["mplan"], C.c_void_p(b["d_q"].data_ptr()),
                                                           C.c_void_p(b["d_q"].data_ptr()), None,
                                                           C.c_void_p(out["d_mres"].data_ptr()),
                                                           C.c_void_p(out["d_mpairs"].data_ptr()), what,
                                                           C.c_void_p(s.cuda_stream)), "gmapdp_microexon_plan_run")

    def dp_launches(self, b, out, fork, used, kernel_only=False):
        """bench.py:694-704: every launch on the caller stream its plan names, the sides forked from `fork`"""
        for li in range(len(b["kinds"])):
            k = min(b["lstream"][li], len(self.sides))
            s = self.stream if k == 0 else self.sides[k - 1]
            if k and k not in used:
                s.wait_event(fork)
                used.add(k)
            self.launch(b, li, s, out, kernel_only=kernel_only)

    def join(self, used):
        for k in used:
            self.stream.wait_stream(self.sides[k - 1])

    # -- bench.py:664-718 --------------------------------------------------------------------------
    def step(self, b, out, do_oligo=True, do_dp=True, piped=False, pipe=3):
        torch, stream, sides = self.torch, self.stream, self.sides
        assert pipe in (0, 3)
        do_oligo = do_oligo and b["oplan"] is not None
        fork = torch.cuda.Event()
        fork.record(stream)
        used = set()
        os_, ss_ = self.ostream, self.sstream
        if do_oligo:
            if not (piped and pipe == 3):
                ss_.wait_event(fork)
            self.orun(b, ss_, 1, out)
            if ss_ is not os_:
                os_.wait_stream(ss_)
            # the chaining as its three kernels (what 4 / 8 / 16: s2a, the s2b sweep, s2c)
            self.orun(b, os_, 4, out)
            self.orun(b, os_, 8, out)
            self.orun(b, os_, 16, out)
        if do_dp:
            self.bind(b, out)
            self.dp_launches(b, out, fork, used)
            ms = sides[-1]
            if len(sides) not in used:
                ms.wait_event(fork)
                used.add(len(sides))
            if b["mplan"] is not None:
                self.mrun(b, ms, 3, out)
        self.join(used)
        if do_oligo and not (piped and pipe):
            stream.wait_stream(self.ostream)

    # -- what a step left --------------------------------------------------------------------------
    def _np(self, t, dtype, n):
        return np.frombuffer(t.cpu().numpy().tobytes(), dtype=dtype)[:n].copy()

    def fetch_dp(self, b, out):
        """{"single" / "end" / "genome": (results in problem order, the pair arena)}: the device records of the
        GPU problems over the host-resolved ones, as a caller of the plan assembles them"""
        dres = self._np(out["d_res"], gmapdp.RESULT_DTYPE, max(b["ngpu"], 1))
        dgres = self._np(out["d_gres"], gmapdp.GENOME_RESULT_DTYPE, max(b["nggpu"], 1))
        pairs = self._np(out["d_pairs"], gmapdp.PAIR_DTYPE, max(b["cap"], 1))
        res = b["host_res"].copy()
        di = b["dev_index"]
        res[di >= 0] = dres[di[di >= 0]]
        gres = b["host_gres"][:b["ng"]].copy()
        gi = b["gdev_index"]
        gres[gi >= 0] = dgres[gi[gi >= 0]]
        return {"single": (res[:b["ns"]], pairs), "end": (res[b["ns"]:], pairs), "genome": (gres, pairs)}

    def fetch_mx(self, b, out):
        n = len(b["d"]["microexon"])
        return {"microexon": (self._np(out["d_mres"], gmapdp.MICROEXON_RESULT_DTYPE, n),
                              self._np(out["d_mpairs"], gmapdp.PAIR_DTYPE, max(b["mcap"], 1)))}

    def fetch_s2(self, b, out, pools=True):
        """{"stage2": (results, paths, pairs)}: the result records `out` holds, and (pools) the path and pair
        pools of the plan's last run through gmapdp_stage2_plan_fetch"""
        n = len(b["d"]["oligo"])
        if not pools:
            return {"stage2": (self._np(out["d_s2res"], gmapdp.STAGE2_RESULT_DTYPE, n),
                               np.zeros(0, dtype=gmapdp.PATH_DTYPE), np.zeros(0, dtype=gmapdp.PATH_PAIR_DTYPE))}
        lib, eng = self.lib, self.eng
        results = np.zeros(n, dtype=gmapdp.STAGE2_RESULT_DTYPE)
        pn, qn = C.c_size_t(), C.c_size_t()
        d_res = C.c_void_p(out["d_s2res"].data_ptr())
        s = C.c_void_p(self.ostream.cuda_stream)
        rc = lib.gmapdp_stage2_plan_fetch(eng.h, b["oplan"], d_res, s, results.ctypes.data, None, 0, None, 0,
                                          C.byref(pn), C.byref(qn))
        if rc not in (0, -6):
            eng._check(rc, "gmapdp_stage2_plan_fetch")
        paths = np.zeros(max(pn.value, 1), dtype=gmapdp.PATH_DTYPE)
        pairs = np.zeros(max(qn.value, 1), dtype=gmapdp.PATH_PAIR_DTYPE)
        eng._check(lib.gmapdp_stage2_plan_fetch(eng.h, b["oplan"], d_res, s, results.ctypes.data, paths.ctypes.data,
                                                len(paths), pairs.ctypes.data, len(pairs), C.byref(pn), C.byref(qn)),
                   "gmapdp_stage2_plan_fetch")
        return {"stage2": (results, paths[:pn.value], pairs[:qn.value])}

    def s2_counters(self, b):
        """the stage-2 plan's four pool counters (gmapdp_stage2_plan_outputs), after a synchronize"""
        ctr = C.c_void_p()
        self.eng._check(self.lib.gmapdp_stage2_plan_outputs(b["oplan"], None, None, C.byref(ctr), None),
                        "gmapdp_stage2_plan_outputs")
        hip = gmapdp._hip()
        host = np.zeros(4, dtype=np.uint64)
        self.torch.cuda.synchronize()
        assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), ctr, host.nbytes, 2) == 0
        return [int(x) for x in host]

    def fetch(self, b, out, pools=True):
        self.torch.cuda.synchronize()
        got = self.fetch_dp(b, out)
        if b["mplan"] is not None:
            got.update(self.fetch_mx(b, out))
        if b["oplan"] is not None:
            got.update(self.fetch_s2(b, out, pools=pools))
        return got

    # -- the plan's schedule and its direction scratch ---------------------------------------------
    def launch_scratch(self, b):
        """Per launch: (stream, hull offset, hull bytes, members' offsets, members' bytes) from
        gmapdp_plan_launch_scratch / _member_scratch; and the plan's total."""
        lib, out = self.lib, []
        for li in range(len(b["kinds"])):
            n = b["info"][li][2]
            offs, nbytes = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
            o, t, o2, t2 = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            assert lib.gmapdp_plan_launch_scratch(b["plan"], li, C.byref(o), C.byref(t)) == 0
            assert lib.gmapdp_plan_launch_member_scratch(b["plan"], li, offs.ctypes.data, nbytes.ctypes.data,
                                                         C.byref(o2), C.byref(t2)) == 0
            assert (o.value, t.value) == (o2.value, t2.value)
            out.append((b["lstream"][li], o.value, t.value, offs.astype(np.int64), nbytes.astype(np.int64)))
        return out, int(lib.gmapdp_plan_scratch_bytes(b["plan"]))


def scratch_overlaps(launches, total):
    """What is wrong with a plan's direction-scratch layout (launch_scratch's output): member regions that
    overlap (of any two launches, so of any two streams), a member outside its launch's range, a range
    past the plan's total.  [] when the launches may all be in flight at once."""
    bad = []
    L, O, N = [], [], []
    for li, (_, off, nbytes, offs, mbytes) in enumerate(launches):
        if off + nbytes > total:
            bad.append("launch %d: range [%d, %d) ends past the plan's %d bytes" % (li, off, off + nbytes, total))
        live = mbytes > 0
        if live.any() and (offs[live].min() < off or (offs[live] + mbytes[live]).max() > off + nbytes):
            bad.append("launch %d: a member lies outside the launch's range" % li)
        if not live.any() and nbytes:
            bad.append("launch %d: a range without members" % li)
        L.append(np.full(int(live.sum()), li))
        O.append(offs[live])
        N.append(mbytes[live])
    if not L:
        return bad
    L, O, N = np.concatenate(L), np.concatenate(O), np.concatenate(N)
    k = np.argsort(O, kind="stable")
    L, O, N = L[k], O[k], N[k]
    # sorted by offset: every region must end before the next begins (running maximum of the ends)
    ends = np.maximum.accumulate(O + N)
    for i in np.nonzero(O[1:] < ends[:-1])[0][:8]:
        bad.append("launches %d and %d: member regions overlap at byte %d" % (L[i], L[i + 1], O[i + 1]))
    return bad
