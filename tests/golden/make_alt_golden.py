#!/usr/bin/env python3
"""Writes tests/golden/alt_single_gap_golden.npz and alt_end_gap_golden.npz: Dynprog_single_gap and
Dynprog_end5_gap / Dynprog_end3_gap calls under an alternate-allele genome (gmap --use-snps), with what the
*reference's own* functions return for them.

Needs the reference tree and the objects `make -C oracle ref` leaves in oracle/_ref/nosimd/ (build()); runs on
the CPU.  alt_refharness.c (beside this file) is compiled against those objects into a temporary directory;
nothing built here is kept.  The genome pair and the calls are tests/altsnp.py's.  Per call three outputs are
kept: both alleles in mode 0 (ref_alt), genomealt == genome (ref_same: what the alternate allele changed) and
both alleles in the stranded cmet mode 1 (ref_alt_mode1).  The cases the set must contain are counted from
the inputs and the reference's outputs (altsnp.count_cases) and printed; the script refuses to write a file
that misses one.

Usage: python tests/golden/make_alt_golden.py [--ref /path/to/reference] [--outdir DIR]"""
import argparse
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import altsnp  # noqa: E402
from dpbind import Pair  # noqa: E402

NOT_LINKED = {"refharness.o", "gmap.o", "inbuffer.o", "outbuffer.o", "access.o", "own_check.o", "fiber_check.o"}
MAXPAIRS = 8192


class Harness:
    """One loaded copy of the harness: Dynprog_init's tables are process-wide per library, so each mode loads its
    own copy of the file."""

    def __init__(self, so, mode, ref, alt):
        self.lib = lib = C.CDLL(so)
        lib.alth_single_gap.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint,
                                        C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(Pair), C.c_int]
        lib.alth_end_gap.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                     C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(Pair), C.c_int]
        lib.alth_init(mode)
        self._keep = (C.create_string_buffer(ref, len(ref)), C.create_string_buffer(alt, len(alt)))
        lib.alth_set_genomes(self._keep[0], self._keep[1], len(ref))
        self.pairs = (Pair * MAXPAIRS)()
        self.scal = (C.c_int * 6)()

    def _out(self, n):
        assert n <= MAXPAIRS
        return tuple(self.scal), (None if n < 0 else [self.pairs[i].key() for i in range(n)])

    def single(self, use_alt, p):
        return self._out(self.lib.alth_single_gap(
            use_alt, p["q"], p["quc"], p["rlength"], p["glength"], p["roffset"], p["goffset"], p["chroffset"],
            p["chrhigh"], p["watsonp"], p["genestrand"], p["jump_late_p"], p["extraband"], p["widebandp"],
            p["defect_rate"], p["dynprogindex"], self.scal, self.pairs, MAXPAIRS))

    def end(self, use_alt, p):
        qpos = 0 if p["end3p"] else max(len(p["q"]) - 1, 0)
        return self._out(self.lib.alth_end_gap(
            use_alt, p["end3p"], p["q"] or b"A", p["quc"] or b"A", qpos, p["rlength"], p["glength"], p["roffset"],
            p["goffset"], p["chroffset"], p["chrhigh"], p["watsonp"], p["genestrand"], p["jump_late_p"],
            p["extraband"], p["defect_rate"], p["endalign"], p["require_pos_score_p"], p["dynprogindex"], self.scal,
            self.pairs, MAXPAIRS))


def build_harness(ref_tree, tmp):
    objs = sorted(o for o in glob.glob(os.path.join(ROOT, "oracle", "_ref", "nosimd", "*.o"))
                  if os.path.basename(o) not in NOT_LINKED)
    if not objs:
        raise SystemExit("no reference objects in oracle/_ref/nosimd: run build() where the reference tree is")
    vs = os.path.join(tmp, "harness.map")
    with open(vs, "w") as f:
        f.write("{ global: alth_*; local: *; };\n")
    ho = os.path.join(tmp, "alt_refharness.o")
    flags = ["-O2", "-fPIC", "-pthread", "-w", "-ffunction-sections", "-fdata-sections", "-DHAVE_CONFIG_H",
             '-DTARGET="x86_64-pc-linux-gnu"', '-DGMAPDB="/nonexistent/gmapdb"', "-I" + os.path.join(ref_tree, "src")]
    subprocess.run(["gcc"] + flags + ["-c", os.path.join(HERE, "alt_refharness.c"), "-o", ho], check=True)
    so = os.path.join(tmp, "libaltref0.so")
    subprocess.run(["gcc", "-shared", "-pthread", "-Wl,--gc-sections", "-Wl,--version-script=" + vs, "-o", so, ho]
                   + objs + ["-lz", "-lm"], check=True)
    so1 = os.path.join(tmp, "libaltref1.so")
    shutil.copy(so, so1)
    return so, so1


def generate(ref_tree, outdir):
    mg = altsnp._make_golden()
    ref, alt = altsnp.snp_genomes()
    sets = (("single", altsnp.single_calls(ref, alt), mg.SINGLE_PARAMS, os.path.basename(altsnp.GOLDEN_SINGLE)),
            ("end", altsnp.end_calls(ref, alt), mg.END_PARAMS, os.path.basename(altsnp.GOLDEN_END)))
    with tempfile.TemporaryDirectory() as tmp:
        so0, so1 = build_harness(ref_tree, tmp)
        h0, h1 = Harness(so0, 0, ref, alt), Harness(so1, 1, ref, alt)
        for kind, calls, names, fname in sets:
            run = (lambda h, ua, p: h.single(ua, p)) if kind == "single" else (lambda h, ua, p: h.end(ua, p))
            outs = {"ref_alt": [run(h0, 1, p) for p in calls], "ref_same": [run(h0, 0, p) for p in calls],
                    "ref_alt_mode1": [run(h1, 1, p) for p in calls]}
            counts = altsnp.count_cases(ref, alt, kind, calls, outs)
            for c in sorted(counts):
                print("%-7s %-22s %d" % (kind, c, counts[c]))
            miss = altsnp.missing_cases(kind, counts)
            if miss:
                raise SystemExit("%s set misses: %s" % (kind, ", ".join(miss)))
            d = mg.pack(ref, calls, outs, names)
            d["genome_alt"] = np.frombuffer(alt, dtype=np.uint8)
            out = os.path.join(outdir, fname)
            np.savez_compressed(out, **d)
            print("wrote %s: %d calls, %d bytes" % (out, len(calls), os.path.getsize(out)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--outdir", default=HERE)
    a = ap.parse_args()
    generate(a.ref, a.outdir)
