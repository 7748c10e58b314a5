"""Debug aid (GPU box): run one Stage2_compute problem through the engine and the oracle and compare
the chaining state (minactive / maxactive and the per-hit link arrays) -- s2_scratch's layout."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gmap-2024_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gmapdp  # noqa: E402
from dpbind import Oracle  # noqa: E402


def a16(x):
    return (x + 15) & ~15


def layout(ql, T, nd):
    Q, D, H = ql + 1, max(nd, 1), max(T, 1)
    s = {"diff": 0}
    s["run"] = a16(4 * Q)
    s["off"] = a16(s["run"] + 8 * Q)
    s["minact"] = a16(s["off"] + 4 * Q)
    s["maxact"] = a16(s["minact"] + 4 * Q)
    s["first"] = a16(s["maxact"] + 4 * Q)
    s["proc"] = a16(s["first"] + 4 * Q)
    s["diags"] = a16(s["proc"] + 4 * Q)
    s["ord"] = a16(s["diags"] + 32 * D)
    s["tmp"] = a16(s["ord"] + 4 * D)
    s["hits"] = a16(s["tmp"] + 4 * D)
    s["maps"] = a16(s["hits"] + 16 * H)  # S2Hit {consec, root, tracei, pred}
    s["sc"] = a16(s["maps"] + 4 * H)
    s["end"] = a16(s["sc"] + 4 * H)
    return s


def main(k=0):
    import importlib.util
    spec = importlib.util.spec_from_file_location("mg", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    g, probs, exp = m.load_stage2(os.path.join(ROOT, "tests", "golden", "stage2_golden.npz"))
    p = probs[k]
    orc = Oracle()
    orc.set_genome(g)
    sc_all = orc.oligo_mappings(dict(p, minor=0))
    sc = sc_all[0]
    T, nd, ql = sc[0], sc[3], len(p["quc"])
    buf = (C.c_int * (2 * ql + 8 * T + 16))()
    orc.lib.orc_stage2_debug(buf)
    o = orc.stage2_compute(p)
    ob = np.frombuffer(buf, dtype=np.int32)
    eng = gmapdp.Engine(0)
    eng.set_genome(g)
    got = eng.stage2_batch([p])[0]
    L = layout(ql, T, nd)
    raw = np.zeros(L["end"], dtype=np.uint8)
    eng.lib.gmapdp_debug_stage2_scratch(eng.h, raw.ctypes.data, C.c_size_t(L["end"]))
    minact = raw[L["minact"]:L["minact"] + 4 * ql].view(np.uint32).astype(np.int64)
    maxact = raw[L["maxact"]:L["maxact"] + 4 * ql].view(np.uint32).astype(np.int64)
    off = raw[L["off"]:L["off"] + 4 * (ql + 1)].view(np.int32)
    # The layout is compact: of each query position only the hits inside [minactive, maxactive], of the
    # first position with hits at or after querystart (q0) all of them.  TL = off[ql] hits are laid out;
    # laid[i] is the oracle's index (position-major over all T hits) of laid-out hit i.
    TL = int(off[ql])
    rec = raw[L["hits"]:L["hits"] + 16 * TL].view(np.int32).reshape(TL, 4)
    maps = raw[L["maps"]:L["maps"] + 4 * TL].view(np.int32)
    scs = raw[L["sc"]:L["sc"] + 4 * TL].view(np.int32)
    npos, pos = np.array(sc_all[1]), np.array(sc_all[2], dtype=np.uint32)
    ooff = np.concatenate([[0], np.cumsum(npos)])
    qstart, qend = int(orc._s2_sc[4]), int(orc._s2_sc[5])
    has = np.nonzero(npos[qstart:qend + 1] > 0)[0]
    q0 = qstart + int(has[0]) if len(has) else -1
    laid, lq = [], []
    for q in range(ql):
        if q > qend or npos[q] == 0:
            continue
        sl = pos[ooff[q]:ooff[q + 1]]
        lo = int(np.searchsorted(sl, minact[q], side="left"))
        hi = max(lo, int(np.searchsorted(sl, maxact[q], side="right")))
        if q == q0:
            lo, hi = 0, int(npos[q])
        assert off[q + 1] - off[q] == hi - lo, (q, off[q], off[q + 1], lo, hi)
        laid.extend(range(ooff[q] + lo, ooff[q] + hi))
        lq.extend([q] * (hi - lo))
    laid, lq = np.array(laid, dtype=np.int64), np.array(lq, dtype=np.int64)
    assert len(laid) == TL, (len(laid), TL)
    # the oracle's field order {map, consec, root, fpos, fhit, tracei, score, active} (+ q): records are
    # written only for the hits the sweep scores, so compare those (score > 0).  The record's link is the
    # predecessor's laid-out index; its (fpos, fhit) come back from off[] and q0's range.
    def pos_of(h):
        return np.searchsorted(off, h, side="right") - 1
    pred = rec[:, 3]
    fpos = np.where(pred >= 0, pos_of(np.maximum(pred, 0)), -1)
    fhit = np.where(pred >= 0, laid[np.maximum(pred, 0)] - ooff[np.maximum(fpos, 0)], -1)
    hits = np.zeros((TL, 9), dtype=np.int32)
    hits[:, 0] = maps
    hits[:, 1:3] = rec[:, 0:2]
    hits[:, 3] = fpos
    hits[:, 4] = fhit
    hits[:, 5] = rec[:, 2]
    hits[:, 6] = scs
    hits[:, 8] = lq
    print("problem", k, "T", T, "laid out", TL, "nd", nd, "ql", ql, "equal results:", got == o, "exp==orc:", exp[k] == o)
    omin = ob[:ql].view(np.uint32).astype(np.int64)
    omax = ob[ql:2 * ql].view(np.uint32).astype(np.int64)
    bad = np.nonzero(omin != minact)[0]
    print("minactive differs at", bad[:10], [(int(omin[i]), int(minact[i])) for i in bad[:5]])
    bad = np.nonzero(omax != maxact)[0]
    print("maxactive differs at", bad[:10], [(int(omax[i]), int(maxact[i])) for i in bad[:5]])
    oall = ob[2 * ql:2 * ql + 8 * T].reshape(T, 8)
    out = np.ones(T, dtype=bool)
    out[laid] = False
    print("hits not laid out with a score in the oracle:", int((oall[out, 6] > 0).sum()))
    oh = oall[laid]
    names = ["map", "consec", "root", "fpos", "fhit", "tracei", "score", "active"]
    scored = oh[:, 6] > 0
    for f in range(7):
        bad = np.nonzero((oh[:, f] != hits[:, f]) & (scored | (f in (0, 6))))[0]
        if len(bad):
            i = bad[0]
            print("hit field %s differs at %d hits, first hit %d (q %d): oracle %s gpu %s" % (
                names[f], len(bad), i, hits[i, 8], oh[i].tolist(), hits[i, :8].tolist()))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
