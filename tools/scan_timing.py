"""Stage2_scan on the bench's configs[2] reads: the scan plan against the other two ways to get ncovered.

Every read's true stage-2 window goes in, plus K decoy windows of the same length elsewhere on the same
chromosome (default 3), both strands mixed, all of a read's regions on one query slice -- what
stage3_from_gregions hands Stage2_scan.  Timed:
  (a) the device-resident scan plan (gmapdp_scan_plan_run), at the default scratch budget and at the
      budgets of --arena-mb (GMAPDP_SCAN_ARENA_MB, read at plan creation);
  (b) the only way the engine offered before: gmapdp_oligo_mappings_batch plus a count on the host, one
      problem per distinct query slice per call (it refuses shared slices), on the first --sub-reads reads;
  (c) the C oracle (orc_oligo_mappings + the same count) on 16 host threads, same reads as (b).
(b) and (c) are scaled to 10 000 reads from their subset: (b) copies the whole positions table to the
host, 0.86 MB per 214-kb region, and its host arrays for 40 000 regions would not fit a call's 2^31-entry table.
Warm-up runs first, then --reps timed runs each; medians with min / max.  Results of (a), (b) and (c)
are compared on the subset.  Writes profiles/<round>_scan/scan_timing.json (--out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gmap-2024_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gmapdp  # noqa: E402
from gmapdp import workload as W  # noqa: E402


def regions_of(genome, layout, reads, decoys, seed=3000):
    """(problems in read-major order, query arena): the reads' true windows (workload.make_stage2, first calls
    only) and `decoys` windows of the same length elsewhere on the read's chromosome."""
    sh = W.CDNA2K
    op, oq = W.make_stage2(genome, layout, reads, np.random.default_rng(seed), exons=sh.exons, exlen=sh.exlen,
                           pad=sh.pad, subs=sh.subs, indel=sh.indel, extra=0.0)
    rng = np.random.default_rng(seed + 1)
    probs = np.repeat(op, 1 + decoys)
    wlen = (op["chrend"].astype(np.int64) - op["chrstart"].astype(np.int64))
    clen = op["chrhigh"].astype(np.int64) - op["chroffset"].astype(np.int64)
    for k in range(1, 1 + decoys):
        s = (rng.random(reads) * (clen - wlen - 2)).astype(np.int64)
        probs["chrstart"][k::1 + decoys] = s
        probs["chrend"][k::1 + decoys] = s + wlen
    return probs, oq


def ncovered_of(diags, off, nd, qlen):
    sc = np.zeros(qlen + 1, dtype=np.int64)
    d = diags[4 * off:4 * (off + nd)].reshape(-1, 4)
    np.add.at(sc, d[:, 1], 1)
    np.add.at(sc, d[:, 2], -1)
    return int(np.count_nonzero(np.cumsum(sc[:qlen]) > 0))


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "runs": len(ms)}


def time_plan(eng, probs, qbuf, warmup, reps):
    hip = gmapdp._hip()
    with eng.scan_plan(probs, qbuf) as plan:
        for _ in range(warmup):
            plan.run()
        hip.hipDeviceSynchronize()
        run_ms, fetch_ms = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            plan.run()
            hip.hipDeviceSynchronize()
            t1 = time.perf_counter()
            out = plan.results()
            t2 = time.perf_counter()
            run_ms.append((t1 - t0) * 1e3)
            fetch_ms.append((t2 - t0) * 1e3)
        return out, plan.nlaunches, plan.scratch_bytes, run_ms, fetch_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--decoys", type=int, default=3)
    ap.add_argument("--sub-reads", type=int, default=1000, help="reads of (b) and (c)")
    ap.add_argument("--genome", default="chr22", choices=["grch38", "chr22"], help="configs[2] genome layout")
    ap.add_argument("--arena-mb", default="2048,32768", help="further scratch budgets for (a), MB, comma-separated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_scan", "scan_timing.json"))
    args = ap.parse_args()

    layout = W.Layout(W.GRCH38 if args.genome == "grch38" else W.CHR22)
    genome = W.PackedGenome(layout.total, seed=38)
    probs, oq = regions_of(genome, layout, args.reads, args.decoys)
    qbuf = oq.tobytes()
    n, per = len(probs), 1 + args.decoys
    scale = 10000.0 / args.reads
    eng = gmapdp.Engine(0)
    eng.set_genome(blocks=genome.blocks, length=genome.length)
    rec = {"workload": "configs[2] reads (workload.CDNA2K: 5 x 400-nt exons, 2 %% substitutions), %s layout; per read "
                       "its stage-2 window and %d decoy windows of the same length on the same chromosome"
                       % (args.genome, args.decoys),
           "reads": args.reads, "regions": n, "mean_querylength": float(probs["querylength"].mean()),
           "mean_window": float((probs["chrend"].astype(np.int64) - probs["chrstart"]).mean()),
           "plus_fraction": float(probs["plusp"].mean()), "warmup": args.warmup, "reps": args.reps}

    # ---- (a) the scan plan, at the default budget and the others ----
    rec["a_scan_plan"] = []
    os.environ.pop("GMAPDP_SCAN_ARENA_MB", None)
    ref_out = None
    for mb in [None] + [int(x) for x in args.arena_mb.split(",") if x]:
        if mb is not None:
            os.environ["GMAPDP_SCAN_ARENA_MB"] = str(mb)
        out, nl, sbytes, run_ms, fetch_ms = time_plan(eng, probs, qbuf, args.warmup, args.reps)
        if ref_out is None:
            ref_out = out
        assert np.array_equal(out, ref_out), "the scan results depend on the budget"
        r = stats(run_ms)
        rec["a_scan_plan"].append({
            "budget": "default" if mb is None else "%d MB" % mb, "sub_batches": nl, "scratch_bytes": int(sbytes),
            "run": r, "run_and_fetch": stats(fetch_ms),
            "ms_per_10k_reads": round(r["median_ms"] * scale, 3),
            "regions_per_s": round(n / (r["median_ms"] * 1e-3)), "host_bytes_per_region": 16})
    os.environ.pop("GMAPDP_SCAN_ARENA_MB", None)
    rec["covered_regions"] = int((ref_out[:, 0] > 0).sum())
    rec["true_window_mean_ncovered"] = float(ref_out[0::per, 0].mean())
    rec["decoy_mean_ncovered"] = float(ref_out[1::per, 0].mean()) if args.decoys else None

    # ---- (b) gmapdp_oligo_mappings_batch + host count: one call per region index (distinct slices) ----
    m = min(args.sub_reads, args.reads)
    sub = probs[:m * per]
    qsub = qbuf[:int(sub["qoff"].max()) + int(sub["querylength"][np.argmax(sub["qoff"])])]
    b_ms, b_count_ms, b_bytes = [], [], 0
    b_out = np.zeros((m * per, 4), dtype=np.int32)
    for it in range(args.warmup + max(3, args.reps // 3)):
        t0 = time.perf_counter()
        tc = 0.0
        nbytes = 0
        for k in range(per):
            pk = np.ascontiguousarray(sub[k::per])
            res, npos, maps, positions, diags = eng.oligo_mappings_batch_raw(pk, qsub)
            nbytes += res.nbytes + npos.nbytes + maps.nbytes
            nbytes += 4 * eng.lib.gmapdp_oligo_positions_capacity(pk.ctypes.data, len(pk))
            nbytes += 16 * eng.lib.gmapdp_oligo_diagonal_capacity(pk.ctypes.data, len(pk))
            c0 = time.perf_counter()
            for i in range(len(pk)):
                b_out[i * per + k] = (ncovered_of(diags, int(res[i]["diag_offset"]), int(res[i]["ndiagonals"]),
                                                  int(pk[i]["querylength"])), 1, res[i]["totalpositions"],
                                      res[i]["maxnconsecutive"])
            tc += time.perf_counter() - c0
        if it >= args.warmup:
            b_ms.append((time.perf_counter() - t0) * 1e3)
            b_count_ms.append(tc * 1e3)
        b_bytes = nbytes
    assert np.array_equal(b_out, ref_out[:m * per]), "(a) and (b) disagree"
    r = stats(b_ms)
    rec["b_oligo_batch_plus_host_count"] = {
        "reads": m, "regions": m * per, "calls": per, "whole": r, "host_count_part": stats(b_count_ms),
        "ms_per_10k_reads": round(r["median_ms"] * 10000.0 / m, 3),
        "regions_per_s": round(m * per / (r["median_ms"] * 1e-3)),
        "host_bytes_per_region": round(b_bytes / (m * per))}

    # ---- (c) the C oracle on 16 host threads ----
    try:
        if layout.total >= 1 << 32:
            raise OSError("the oracle's coordinates are 32-bit; run with --genome chr22")
        from dpbind import Oracle
        orc = Oracle()
        orc.set_genome(genome.ascii(0, genome.length))
        f = orc.lib.orc_oligo_mappings
        f.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_int),
                      C.POINTER(C.c_uint), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
        f.restype = C.c_int
        T = 16
        c_out = np.zeros((m * per, 4), dtype=np.int32)

        def work(t):
            cap = 1 << 22
            pos, dg, sc = (C.c_uint * cap)(), (C.c_int * (4 * 65536))(), (C.c_int * 4)()
            for i in range(t, m * per, T):
                p = sub[i]
                ql = int(p["querylength"])
                npos = (C.c_int * ql)()
                q = qsub[int(p["qoff"]):int(p["qoff"]) + ql]
                rc = f(q, ql, int(p["chrstart"]), int(p["chrend"]), int(p["chroffset"]), int(p["chrhigh"]),
                       int(p["plusp"]), 0, npos, pos, cap, sc, dg, 65536)
                assert rc >= 0
                d = np.frombuffer(dg, dtype=np.int32, count=4 * sc[3])
                c_out[i] = (ncovered_of(d, 0, sc[3], ql), 1, sc[0], sc[1])
        c_ms = []
        for it in range(1 + max(3, args.reps // 3)):
            t0 = time.perf_counter()
            with ThreadPoolExecutor(T) as ex:
                list(ex.map(work, range(T)))
            if it >= 1:
                c_ms.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(c_out, ref_out[:m * per]), "(a) and the oracle disagree"
        r = stats(c_ms)
        rec["c_oracle_16_threads"] = {"reads": m, "regions": m * per, "whole": r,
                                      "ms_per_10k_reads": round(r["median_ms"] * 10000.0 / m, 3),
                                      "regions_per_s": round(m * per / (r["median_ms"] * 1e-3))}
    except OSError as e:  # the oracle library is not built
        rec["c_oracle_16_threads"] = {"not_measured": str(e)}
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
