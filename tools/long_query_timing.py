"""Diagnostic (GPU box): the time of one stage-2 seeding call of the long class (queries with more than 16 384
distinct 8-mers, GMAPDP_CTX_LONG_QUERIES) beside the largest LDS class and the reference on the CPU.

Each call is a one-problem device-resident seeding plan (gmapdp_oligo_plan_run: oi_long_kernel or oi_kernel, then
oi_map_kernel), timed with HIP events on the context's stream: 3 warm-up runs, then the median, minimum and
maximum of 20.  The calls are tests/longq.py's: a spliced 24-kb read in its ~40-kb window (case B), the whole
de Bruijn sequence (65 536 distinct 8-mers) against a 70 000-nt window, and its 16 384-id prefix, which still
takes the LDS class, against the same window.  With the reference harness built (oracle/_ref) the same calls
are timed there too (refh_oligo_mappings, one thread, best of 5).  Prints one JSON line per call.

    python tools/long_query_timing.py"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gmap-2024_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gmapdp  # noqa: E402
import longq  # noqa: E402
from dpbind import Ref, ref_available  # noqa: E402

WARM, RUNS = 3, 20


def gpu_times(eng, hip, call):
    lib = eng.lib
    lib.gmapdp_stream.restype = C.c_void_p
    stream = C.c_void_p(lib.gmapdp_stream(eng.h))
    probs, qucbuf = gmapdp.Engine.build_oligo_batch([call])
    plan = C.c_void_p()
    eng._check(lib.gmapdp_oligo_plan_create(eng.h, probs.ctypes.data, 1, qucbuf, len(qucbuf), C.byref(plan)),
               "gmapdp_oligo_plan_create")
    pc = max(lib.gmapdp_oligo_plan_positions_capacity(plan), 1)
    dc = max(lib.gmapdp_oligo_plan_diagonal_capacity(plan), 1)
    sizes = [len(qucbuf), gmapdp.OLIGO_RESULT_DTYPE.itemsize, 4 * len(qucbuf), 4 * len(qucbuf), 4 * pc, 16 * dc]
    dev = []
    for nbytes in sizes:
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(nbytes, 16)) == 0
        dev.append(p)
    assert hip.hipMemcpy(dev[0], qucbuf, len(qucbuf), 1) == 0
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    ms = []
    for r in range(WARM + RUNS):
        assert hip.hipEventRecord(e0, stream) == 0
        eng._check(lib.gmapdp_oligo_plan_run(eng.h, plan, *dev, None), "gmapdp_oligo_plan_run")
        assert hip.hipEventRecord(e1, stream) == 0
        assert hip.hipEventSynchronize(e1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        if r >= WARM:
            ms.append(t.value)
    res = np.zeros(1, dtype=gmapdp.OLIGO_RESULT_DTYPE)
    assert hip.hipMemcpy(res.ctypes.data, dev[1], res.nbytes, 2) == 0
    for p in dev:
        hip.hipFree(p)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    lib.gmapdp_oligo_plan_destroy(plan)
    return ms, res[0]


def ref_time(ref, call):
    out = ref.oligo_mappings(call)  # (sets the binding up; the timed calls below are the C function alone)
    f, n = ref.lib.refh_oligo_mappings, len(call["quc"])
    npos = (C.c_int * n)()
    best = None
    for _ in range(5):
        ref._before_call()
        t0 = time.perf_counter()
        r = f(call["quc"], n, C.c_uint(call["chrstart"]), C.c_uint(call["chrend"]), C.c_uint(call["chroffset"]),
              C.c_uint(call["chrhigh"]), int(call["plusp"]), int(call["minor"]), npos, ref._om_pos, ref._om_cap,
              ref._om_sc, ref._om_dg, 65536)
        t = time.perf_counter() - t0
        assert r >= 0
        best = t if best is None else min(best, t)
    return 1e3 * best, out[0]


def main():
    g = longq.genome()
    cases = [("case_B_24kb_read", longq.spliced_calls(g)[0][0]),
             ("n65536_window70000", longq.call(longq.prefix(65536), 20000, 90000, 1)),
             ("n16384_window70000_lds_class", longq.call(longq.prefix(16384), 20000, 90000, 1))]
    eng = gmapdp.Engine(0, flags=gmapdp.CTX_LONG_QUERIES)
    eng.set_genome(g)
    hip = gmapdp._hip()
    ref = None
    if ref_available():
        ref = Ref()
        ref.set_genome(g)
    for name, call in cases:
        before = eng.long_query_calls()
        ms, res = gpu_times(eng, hip, call)
        rec = {"case": name, "querylength": len(call["quc"]), "window": call["chrend"] - call["chrstart"],
               "distinct_8mers": longq.distinct_8mers(call["quc"]), "long_class": eng.long_query_calls() > before,
               "totalpositions": int(res["totalpositions"]), "ndiagonals": int(res["ndiagonals"]),
               "gpu_ms_median": round(statistics.median(ms), 4), "gpu_ms_min": round(min(ms), 4),
               "gpu_ms_max": round(max(ms), 4)}
        if ref is not None:
            t, sc = ref_time(ref, call)
            rec["ref_cpu_ms"] = round(t, 3)
            rec["ref_totalpositions"] = int(sc[0])
        print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
