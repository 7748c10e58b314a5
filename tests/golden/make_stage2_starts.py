#!/usr/bin/env python3
"""Writes tests/golden/stage2_starts_golden.npz: Stage2_compute_starts calls with the lists the *reference's own*
function returns for them.

Needs the reference tree and the objects `make -C oracle ref` leaves in oracle/_ref/nosimd/ (build()); runs on
the CPU.  stage2_starts_refharness.c (beside this file) is compiled against those objects into a temporary
directory; nothing built here is kept.

The inputs are tests/s2starts.py's edge shapes and 70 random calls.  Each call's rule counters (restart,
zero-score early branch, position with >= 100 hits scored, tied best cells, lists eliminated, "nothing
eliminated, first kept", terminal pruning) come from the oracle tests/s2soracle, after the oracle's lists have
been checked against the reference's here; the script refuses to write a set in which a counter other than
`pruned` stays zero, or in which a strand or splicingp value does not occur.

Usage: python tests/golden/make_stage2_starts.py [--ref /path/to/reference]"""
import argparse
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import s2starts  # noqa: E402
from dpbind import Pair  # noqa: E402

NOT_LINKED = {"refharness.o", "gmap.o", "inbuffer.o", "outbuffer.o", "access.o", "own_check.o", "fiber_check.o"}
NRANDOM = 70
PAIR_CAP, PATH_CAP = 1 << 16, 256


def build_harness(ref, tmp):
    objs = sorted(o for o in glob.glob(os.path.join(ROOT, "oracle", "_ref", "nosimd", "*.o"))
                  if os.path.basename(o) not in NOT_LINKED)
    if not objs:
        raise SystemExit("no reference objects in oracle/_ref/nosimd: run build() where the reference tree is")
    vs = os.path.join(tmp, "harness.map")
    with open(vs, "w") as f:
        f.write("{ global: s2sh_*; local: *; };\n")
    ho = os.path.join(tmp, "stage2_starts_refharness.o")
    flags = ["-O2", "-fPIC", "-pthread", "-w", "-ffunction-sections", "-fdata-sections", "-DHAVE_CONFIG_H",
             '-DTARGET="x86_64-pc-linux-gnu"', '-DGMAPDB="/nonexistent/gmapdb"', "-I" + os.path.join(ref, "src")]
    subprocess.run(["gcc"] + flags + ["-c", os.path.join(HERE, "stage2_starts_refharness.c"), "-o", ho], check=True)
    so = os.path.join(tmp, "libs2sref.so")
    subprocess.run(["gcc", "-shared", "-pthread", "-Wl,--gc-sections", "-Wl,--version-script=" + vs, "-o", so, ho]
                   + objs + ["-lz", "-lm"], check=True)
    lib = C.CDLL(so)
    lib.s2sh_compute.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                 C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(Pair), C.c_int]
    lib.s2sh_compute.restype = C.c_int
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=s2starts.GOLDEN)
    a = ap.parse_args()
    g = s2starts.genome()
    calls = list(s2starts.edge_calls()[0]) + s2starts.random_calls(NRANDOM, seed=1)
    orc = s2starts.S2SOracle()
    orc.set_genome(g)
    paths = (C.c_int * (2 * PATH_CAP))()
    pairs = (Pair * PAIR_CAP)()
    recs, lists, allpairs, counters = [], [], [], []
    qs, qu, qoff, differ = [], [], 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        ref = build_harness(a.ref, tmp)
        ref.s2sh_set_genome(g, len(g))
        for i, p in enumerate(calls):
            n = len(p["quc"])
            # as stage 3 passes the 5' end: the query's first characters, the rest of the query behind them
            r = ref.s2sh_compute(p["q"] + b"ACGTACGTAC", p["quc"] + b"ACGTACGTAC", n, p["query_offset"],
                                 C.c_uint(p["chrstart"]), C.c_uint(p["chrend"]), C.c_uint(p["chroffset"]),
                                 C.c_uint(p["chrhigh"]), p["plusp"], p["splicingp"], p["maxintronlen"], paths,
                                 PATH_CAP, pairs, PAIR_CAP)
            if r < 0:
                raise SystemExit("call %d: capacity" % i)
            exp = [[pairs[paths[2 * k] + j].key() for j in range(paths[2 * k + 1])] for k in range(r)]
            cnt = (C.c_long * len(s2starts.COUNTERS))()
            got = orc.compute(p, counters=cnt)
            if got[0] == "err" or (got[0], got[1]) != (r, exp):
                differ += 1
                print("call %d: oracle differs from the reference: %s vs %d lists" % (i, got[0], r))
            recs.append((qoff, n, p["query_offset"], p["chrstart"], p["chrend"], p["chroffset"], p["chrhigh"],
                         p["plusp"], p["splicingp"], p["maxintronlen"], r, len(lists)))
            for lst in exp:
                lists.append((len(allpairs), len(lst)))
                allpairs += lst
            counters.append(list(cnt))
            qs.append(p["q"])
            qu.append(p["quc"])
            qoff += n
    if differ:
        raise SystemExit("%d of %d calls differ: fix the oracle first (the counters come from it)"
                         % (differ, len(calls)))
    cdt = np.dtype([(k, "<i8") for k in ("qoff", "querylength", "query_offset", "chrstart", "chrend", "chroffset",
                                         "chrhigh", "plusp", "splicingp", "maxintronlen", "nlists", "list_off")])
    pdt = np.dtype([("querypos", "<i4"), ("genomepos", "<i4"), ("queryjump", "<i4"), ("genomejump", "<i4"),
                    ("dynprogindex", "<i4"), ("cdna", "S1"), ("comp", "S1"), ("genome", "S1"), ("genomealt", "S1"),
                    ("gapp", "<i4")])
    c = np.array(recs, dtype=cdt)
    cn = np.array(counters, dtype=np.int64)
    # power: the set must reach every rule by itself
    for j, name in enumerate(s2starts.COUNTERS):
        tot = int(cn[:, j].sum())
        print("%-13s %d" % (name, tot))
        if tot == 0 and name != "pruned":
            raise SystemExit("counter %s never fired" % name)
    if set(c["plusp"]) != {0, 1} or set(c["splicingp"]) != {0, 1}:
        raise SystemExit("a strand or splicingp value is missing")
    np.savez_compressed(a.out, genome=np.frombuffer(g, dtype=np.uint8), calls=c,
                        qseq=np.frombuffer(b"".join(qs), dtype=np.uint8), quc=np.frombuffer(b"".join(qu), dtype=np.uint8),
                        lists=np.array(lists, dtype=np.dtype([("pair_off", "<i8"), ("npairs", "<i4")])),
                        pairs=np.array(allpairs, dtype=pdt), counters=cn)
    print("wrote %s: %d calls, %d lists, %d pairs, %d bytes" % (a.out, len(c), len(lists), len(allpairs),
                                                               os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
