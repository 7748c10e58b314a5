"""Stage2_compute_one / Stage2_compute_ends / Stage2_compute_starts on the engine against the CPU oracles on 16
threads.

ONE and ENDS: the calls are the goldens' (tests/golden/stage2x_golden.npz: the shapes stage 3 makes, the edge
shapes included), repeated to --calls per kind (default 10 000) in one batch.  STARTS (--kinds starts): --calls
calls from s2starts.random_calls, and beside them the same number of ENDS calls from s2x.random_calls
("ends_random") and the STARTS calls' mirror images as ENDS calls ("ends_mirrored": the same chains without the
mirrored layout and the un-mirroring) on the same build.  Timed per kind:
  (a) gmapdp_stage2x_batch, the whole synchronous call: upload, seeding, chaining, copy-out into host arenas
      large enough (a first untimed call sizes them);
  (b) the oracle (tests/s2xoracle's orc_stage2x_batch, tests/s2soracle's orc_stage2s_batch) on 16 host threads.
One warm-up run, then --reps timed runs each; medians with min / max.  The two results are compared.
Prints one JSON line and writes it to --out when given."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gmap-2024_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gmapdp  # noqa: E402
import s2starts  # noqa: E402
import s2x  # noqa: E402
from dpbind import stage2_mismatches  # noqa: E402


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10000, help="calls per kind")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kinds", default="one,ends", help="comma-separated: one, ends (the goldens' calls), starts "
                    "(random STARTS calls, as many random ENDS calls, and the STARTS calls mirrored into ENDS calls)")
    args = ap.parse_args()
    g, calls, _, _ = s2x.golden()
    eng = gmapdp.Engine(0)
    eng.set_genome(g)
    orc = s2x.S2XOracle()
    orc.set_genome(g)
    sorc = s2starts.S2SOracle(orc.orc)
    rec = {"workload": "the goldens' calls of each kind repeated to %d calls in one batch; starts / ends_random: "
                       "%d random calls" % (args.calls, args.calls),
           "reps": args.reps, "oracle_threads": args.threads}
    todo = []
    for name in args.kinds.split(","):
        if name == "starts":
            starts = s2starts.random_calls(args.calls, seed=77)
            todo += [("starts", gmapdp.S2X_STARTS, starts),
                     ("ends_random", s2x.ENDS, s2x.random_calls(s2x.ENDS, args.calls, seed=77)),
                     # the same chains as ENDS calls: the reverse-complemented queries on the opposite strand
                     ("ends_mirrored", s2x.ENDS, [s2starts.mirrored_ends_call(p) for p in starts])]
        else:
            kind = {"one": s2x.ONE, "ends": s2x.ENDS}[name]
            base = [calls[i] for i in s2x.by_kind(calls)[kind] if len(calls[i]["quc"]) > 8]
            todo.append((name, kind, [base[i % len(base)] for i in range(args.calls)]))
    for name, kind, batch in todo:
        run_oracle = ((lambda *a, **k: sorc.batch(*a, **k)) if kind == gmapdp.S2X_STARTS
                      else (lambda *a, _kind=kind, **k: orc.batch(_kind, *a, **k)))
        probs, qbuf, qucbuf = eng.build_stage2x_batch(batch, kind)
        results, paths, pairs = eng.stage2x_batch_raw(probs, qbuf, qucbuf)   # warm-up; sizes the arenas
        pcap, qcap = len(paths) + 1, len(pairs) + 1
        gpu = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = eng.stage2x_batch_raw(probs, qbuf, qucbuf, path_cap=pcap, pair_cap=qcap)
            gpu.append((time.perf_counter() - t0) * 1e3)
            assert len(out) == 3 and not isinstance(out[0], int)
        exp = run_oracle(probs, qbuf, qucbuf, nthreads=args.threads)   # warm-up
        cpu = []
        for _ in range(max(3, args.reps // 2)):
            t0 = time.perf_counter()
            exp = run_oracle(probs, qbuf, qucbuf, nthreads=args.threads)
            cpu.append((time.perf_counter() - t0) * 1e3)
        bad = stage2_mismatches(results, paths, pairs, exp)
        rec[name] = {
            "calls": len(batch), "mean_querylength": float(probs["querylength"].mean()),
            "mean_window": float((probs["chrend"].astype(np.int64) - probs["chrstart"].astype(np.int64)).mean()),
            "lists": int(results["nresults"].sum()), "pair_records": int(len(pairs)),
            "gpu_batch": stats(gpu), "oracle": stats(cpu), "mismatches": len(bad)}
    eng.close()
    line = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
