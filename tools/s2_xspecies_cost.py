"""What cross-species canonical scoring (GMAPDP_S2_CANONICAL_MIDDLE, gmap --cross-species) costs the stage-2
sweep: the s2b kernel alone (gmapdp_stage2_plan_run what = 8) and stage 2 alone (what = 3) on bench.py's
Stage2_compute calls (tools/s2_run.py's: chr22 layout, the configs[2] read shape, `gmap -d` windows), with
the flag off and on.  Per setting one plan, one warm-up chain, then `reps` timed runs of each (wall clock
around a device synchronisation; medians).  Prints one JSON line: ms per 10 000 reads for both settings, and
the flagged sweep's own counters for one run (range-2 candidates by form, MaxEnt-evaluated shifts).

    python tools/s2_xspecies_cost.py [reads] [reps]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gmap-2024_amd"))
import gmapdp  # noqa: E402
from gmapdp import workload as W  # noqa: E402


def main(reads=10000, reps=7):
    layout = W.Layout(W.CHR22)
    genome = W.make_genome(layout, seed=22)
    eng = gmapdp.Engine(0)
    eng.set_genome(genome.tobytes())
    sh = W.CDNA2K
    op, oq = W.make_stage2(genome, layout, reads, np.random.default_rng(3000), pad=sh.pad, extra=sh.stage2 - 1.0)
    calls = [dict(quc=oq[int(p["qoff"]):int(p["qoff"]) + int(p["querylength"])].tobytes(),
                  **{k: int(p[k]) for k in ("chrstart", "chrend", "chroffset", "chrhigh", "plusp")}) for p in op]
    hip, lib = gmapdp._hip(), eng.lib
    out = {"reads": reads, "reps": reps}
    for name, flag in (("default", False), ("cross_species", True)):
        probs, qb, qub = eng.build_stage2_batch(calls, cross_species=flag)
        plan = C.c_void_p()
        eng._check(lib.gmapdp_stage2_plan_create(eng.h, probs.ctypes.data, len(probs), qb, qub, len(qub), C.byref(plan)),
                   "gmapdp_stage2_plan_create")
        bufs = []

        def dbuf(nbytes, src=None):
            ptr = C.c_void_p()
            assert hip.hipMalloc(C.byref(ptr), max(nbytes, 16)) == 0
            bufs.append(ptr)
            if src is not None:
                assert hip.hipMemcpy(ptr, src, nbytes, 1) == 0
            return ptr
        d_q, d_quc = dbuf(len(qb), qb), dbuf(len(qub), qub)
        d_res = dbuf(len(probs) * gmapdp.STAGE2_RESULT_DTYPE.itemsize)

        def run(what):
            t0 = time.perf_counter()
            eng._check(lib.gmapdp_stage2_plan_run(eng.h, plan, d_q, d_quc, d_res, what, None), "gmapdp_stage2_plan_run")
            assert hip.hipDeviceSynchronize() == 0
            return (time.perf_counter() - t0) * 1e3
        run(3)
        eng.canon_counters()
        run(8)
        counters = eng.canon_counters()
        s2b = [run(8) for _ in range(reps)]
        whole = [run(3) for _ in range(reps)]
        scale = 10000.0 / reads
        out[name] = {"s2b_ms_per_10k": round(statistics.median(s2b) * scale, 3),
                     "s2b_ms_all": [round(x * scale, 3) for x in s2b],
                     "stage2_ms_per_10k": round(statistics.median(whole) * scale, 3),
                     "stage2_ms_all": [round(x * scale, 3) for x in whole]}
        if flag:
            out[name]["range2_candidates_by_form"] = counters[:7]
            out[name]["range2_candidates"] = sum(counters[:7])
            out[name]["maxent_evaluated_shifts"] = counters[7]
        for b in bufs:
            hip.hipFree(b)
        lib.gmapdp_stage2_plan_destroy(plan)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10000, int(sys.argv[2]) if len(sys.argv) > 2 else 7)
