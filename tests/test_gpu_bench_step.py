"""The outputs of the step bench.py times (its headline), against the oracle.  bench.py drives the engine in a
way nothing else does: Stage2_compute as four gmapdp_stage2_plan_run calls (what = 1 on one stream, then 4, 8,
16 on the stage-2 stream) on a plan that never makes a full run; the DP launches one at a time
(gmapdp_plan_run_launch) on caller streams, main plus two sides of a CTX_TWO_SIDES context; the microexon plan
on the last side beside them; with GMAPDP_BENCH_PIPE=3 the stage-2 chain of block k+1 overlapping block k's DP
classes; several blocks' plans on one context, replayed into output arenas that are never cleared.
tests/benchstep.py restates that set-up and step; here:

  a. the split runs equal the whole runs, and both the oracle (stage 2, DP, DP kernel-only replay, microexon);
  b. three replays of the serialised step, every output arena filled with 0xA5 before each, equal the oracle
     every time (a skipped record or pair range would keep the poison);
  c. the pipelined step over three blocks of 120, 200 and 120 reads, two rounds with per-step output buffers
     and one synchronize at the end, for GMAPDP_BENCH_PIPE 0 and 3, and 3 with `bench.py --simd`.  PIPE 1 and 2
     are variants DESIGN.md §7 records as slower; they are left out;
  d. beside the dynamic run a deterministic check: no two launches of a plan share a byte of the context's
     direction scratch (gmapdp_plan_launch_member_scratch), so they may be in flight together whatever the
     timing.  (A launch's range, gmapdp_plan_launch_scratch, is the hull of its members' regions; regions follow
     problem order, so the hulls of different launches interleave and only the members' regions are disjoint.)

Everything is compared bit for bit.  The stage-2 pools hand out their records through atomic cursors, so where a
call's paths land in them differs from run to run: pools and result records are compared call by call
(benchstep.stage2_by_call), the pool counters exactly.

Measured on an MI355X, wall time per test (block generation, plans and the oracle included; the first test of a
block pays for its generation and oracle): split on a fresh plan 1.8 s, split equals whole 0.02 s, DP whole /
per-launch / kernel-only 0.8 s, microexon 0.01 s, poisoned replays 0.7 s, pipelined step 1.7 s (pipe 0), 1.1 s
(pipe 3), 1.7 s (pipe 3, SIMD semantics); the module 8.5 s.

Why the poison matters (measured with these helpers): a step with one launch class left out, run into arenas a
complete step had filled, compares clean -- the stale bytes are the right ones; into poisoned arenas the same
step is reported for that launch's members and nothing else."""
import ctypes as C

import numpy as np
import pytest

import benchstep as BS

pytestmark = pytest.mark.gpu


def _premises(bench, b):
    """the block's plan is the bench's situation (test d of the issue), so nothing below passes vacuously"""
    assert set(b["lstream"]) == {0, 1, 2}, "the plan's launches use the main stream and both sides"
    genome_kinds = (1, 5)   # gg, uxg
    assert any(k in genome_kinds and not info[1] for k, info in zip(b["kinds"], b["info"])), \
        "a genome-gap launch keeps its directions in global scratch"
    assert any(info[1] for info in b["info"]), "a launch keeps its directions in LDS"
    n16, n32 = C.c_int(), C.c_int()
    assert bench.lib.gmapdp_stage2_plan_seeding_classes(b["oplan"], C.byref(n16), C.byref(n32)) == 0
    assert n16.value > 0 and n16.value + n32.value == len(b["d"]["oligo"])
    launches, total = bench.launch_scratch(b)
    assert total > 0 and any(nb for _, _, nb, _, _ in launches)
    assert BS.scratch_overlaps(launches, total) == []


def _work_premises(got, frac=0.9):
    assert np.all(got["stage2"][0]["status"] == 2), "every Stage2_compute call chains"
    assert (got["genome"][0]["npairs"] > 0).mean() >= frac, "the genome gaps emit pairs"


def _same_dp(a, b, fams=("single", "end", "genome")):
    """results and every problem's pair records identical between two runs"""
    for fam in fams:
        (ra, pa), (rb, pb) = a[fam], b[fam]
        assert ra.tobytes() == rb.tobytes(), fam
        cnt = np.maximum(ra["npairs"].astype(np.int64), 0)
        idx = np.repeat(ra["pair_offset"].astype(np.int64), cnt) + (np.arange(int(cnt.sum())) -
                                                                    np.repeat(np.cumsum(cnt) - cnt, cnt))
        assert len(idx) > 0 and pa[idx].tobytes() == pb[idx].tobytes(), fam


@pytest.fixture(scope="module")
def bench200():
    genome, d = BS.block200()
    bench = BS.Bench(genome, [d])
    yield bench
    bench.close()


@pytest.fixture(scope="module")
def oracle200():
    return BS.block200_oracle()


def _split_chain(bench, b, out):
    """what = 1 on stream A, then (event) 4, 8, 16 on stream B"""
    a, s = bench.sides[0], bench.ostream
    bench.orun(b, a, 1, out)
    s.wait_stream(a)
    for what in (4, 8, 16):
        bench.orun(b, s, what, out)


# ---- a. split runs equal whole runs -------------------------------------------------------------------
def test_gpu_stage2_split_on_fresh_plan(oracle200):
    """bench.py's actual situation: the 1 / 4 / 8 / 16 split on a plan that has never made a full run"""
    genome, d = BS.block200()
    bench = BS.Bench(genome, [d])
    try:
        b = bench.B[0]
        _premises(bench, b)
        out = bench.outputs(BS.POISON)
        bench.torch.cuda.synchronize()
        _split_chain(bench, b, out)
        bench.torch.cuda.synchronize()
        got = bench.fetch_s2(b, out)
        bad = BS.step_mismatches(got, oracle200)
        assert not bad, bad[:8]
        assert np.all(got["stage2"][0]["status"] == 2)
    finally:
        bench.close()


def test_gpu_stage2_split_equals_whole(bench200, oracle200):
    b = bench200.B[0]
    _premises(bench200, b)
    whole, split = bench200.outputs(BS.POISON), bench200.outputs(BS.POISON)
    bench200.torch.cuda.synchronize()
    bench200.orun(b, bench200.ostream, 3, whole)
    got_w = bench200.fetch_s2(b, whole)
    ctr_w = bench200.s2_counters(b)
    _split_chain(bench200, b, split)
    bench200.torch.cuda.synchronize()
    got_s = bench200.fetch_s2(b, split)
    ctr_s = bench200.s2_counters(b)
    for got in (got_w, got_s):
        bad = BS.step_mismatches(got, oracle200)
        assert not bad, bad[:8]
    assert ctr_w == ctr_s and ctr_w[1] == len(got_w["stage2"][1]) and ctr_w[2] == len(got_w["stage2"][2])
    assert ctr_w[1] >= len(b["d"]["oligo"])    # every call keeps a path
    assert BS.stage2_by_call(*got_w["stage2"]) == BS.stage2_by_call(*got_s["stage2"])


def test_gpu_dp_whole_equals_per_launch(bench200, oracle200):
    """gmapdp_plan_run (the engine's schedule over the context's own side streams) against the per-launch loop
    on caller streams (bench.py:694-704); then the loop replayed with gmapdp_plan_run_launch_kernel on a
    poisoned result arena, d_sprob as the prologues filled it."""
    bench, b = bench200, bench200.B[0]
    torch = bench.torch
    whole, loop, replay = bench.outputs(BS.POISON), bench.outputs(BS.POISON), bench.outputs(BS.POISON)
    bench.poison(whole, b)
    bench.bind(b, whole)
    bench.plan_run(b, bench.stream, whole)
    torch.cuda.synchronize()
    got_w = bench.fetch_dp(b, whole)
    bench.poison(loop, b)
    for out, kernel_only in ((loop, False), (replay, True)):
        bench.bind(b, out)
        fork, used = torch.cuda.Event(), set()
        fork.record(bench.stream)
        bench.dp_launches(b, out, fork, used, kernel_only=kernel_only)
        bench.join(used)
        torch.cuda.synchronize()
        assert used == {1, 2}
    got_l, got_r = bench.fetch_dp(b, loop), bench.fetch_dp(b, replay)
    for got in (got_w, got_l, got_r):
        bad = BS.step_mismatches(got, oracle200)
        assert not bad, bad[:8]
    _same_dp(got_w, got_l)
    _same_dp(got_l, got_r)
    assert (got_w["genome"][0]["npairs"] > 0).mean() >= 0.9


def test_gpu_microexon_split_equals_whole(bench200, oracle200):
    bench, b = bench200, bench200.B[0]
    whole, split = bench.outputs(BS.POISON), bench.outputs(BS.POISON)
    bench.torch.cuda.synchronize()
    ms = bench.sides[-1]
    bench.mrun(b, ms, 3, whole)
    bench.torch.cuda.synchronize()
    bench.mrun(b, ms, 1, split)
    bench.mrun(b, ms, 2, split)
    bench.torch.cuda.synchronize()
    got_w, got_s = bench.fetch_mx(b, whole), bench.fetch_mx(b, split)
    for got in (got_w, got_s):
        bad = BS.step_mismatches(got, oracle200)
        assert not bad, bad[:8]
    assert got_w["microexon"][0].tobytes() == got_s["microexon"][0].tobytes()
    assert (got_w["microexon"][0]["npairs"] > 0).sum() > 0
    _same_dp(got_w, got_s, fams=("microexon",))


# ---- b. replays into poisoned arenas ------------------------------------------------------------------
def test_gpu_replays_into_poisoned_arenas(bench200, oracle200):
    """The serialised step (all three plans) three times into one set of arenas, every arena -- DP results,
    genome results, pairs, microexon results and pairs, the stage-2 result records, d_sprob -- filled with
    0xA5 before each run: every record and every pair record of every problem equals the oracle each time."""
    bench, b = bench200, bench200.B[0]
    out = bench.outputs()
    runs = []
    for run in range(3):
        bench.poison(out, b)
        bench.step(b, out, piped=False, pipe=0)
        got = bench.fetch(b, out)
        bad = BS.step_mismatches(got, oracle200)
        assert not bad, (run, bad[:8])
        _work_premises(got)
        runs.append((BS.stage2_by_call(*got["stage2"]), bench.s2_counters(b)))
    assert runs[2][1] == runs[0][1], "the stage-2 pool counters after run 3 and after run 1"
    assert runs[2][0] == runs[0][0], "the stage-2 pools after run 3 and after run 1"


# ---- c. the pipelined step ----------------------------------------------------------------------------
@pytest.mark.parametrize("pipe,simd", [(0, False), (3, False), (3, True)], ids=["pipe0", "pipe3", "pipe3-simd"])
def test_gpu_pipelined_step(pipe, simd):
    genome, data = BS.blocks3()
    oracle = BS.blocks3_oracle(simd)
    bench = BS.Bench(genome, data, simd=simd)
    try:
        for b in bench.B:
            _premises(bench, b)
        nb = len(bench.B)
        outs = [bench.outputs(BS.POISON) for _ in range(2 * nb)]
        bench.torch.cuda.synchronize()
        for k, out in enumerate(outs):       # two rounds over the blocks, nothing synchronized in between
            bench.step(bench.B[k % nb], out, piped=True, pipe=pipe)
        bench.stream.wait_stream(bench.ostream)
        bench.torch.cuda.synchronize()
        emit = []
        for k, out in enumerate(outs):
            b = bench.B[k % nb]
            last = k >= nb                   # the plan's pools hold the block's last run
            got = bench.fetch(b, out, pools=last)
            bad = BS.step_mismatches(got, oracle[k % nb], stage2_paths=last)
            assert not bad, ("step %d (block %d)" % (k, k % nb), bad[:8])
            _work_premises(got, frac=0.85 if simd else 0.9)
            emit.append(got["genome"][0]["npairs"] > 0)
        assert np.concatenate(emit).mean() >= 0.9
    finally:
        bench.close()
