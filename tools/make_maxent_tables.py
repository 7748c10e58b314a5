#!/usr/bin/env python3
"""Regenerate the MaxEnt splice-site model tables the engine's device Maxent_hr_*_prob reads.

GMAP's splice-site models (maxent_hr.c:25-24660) are constant tables: per model a 7-mer/9-mer score table of
16 384 doubles and a 16-entry dinucleotide table (the acceptor models have five score tables).  This script
reads them from the reference's source where it lies (default /root/reference/src/maxent_hr.c), converts
every decimal literal the way a C compiler does (correctly rounded to the nearest double; Python's float() is
correctly rounded too) and writes them as one little-endian binary that libgmapdp.so loads
(gmap-2024_amd/lib/maxent_hr_tables.bin, next to the library; git-ignored, built by __graft_entry__.build()
and `make -C gmap-2024_amd`).

A checkout without the reference tree builds the same binary from the stored model weights
tests/golden/maxent_hr_{plus,minus}.npz: the same doubles, one named array per table, recorded from the
reference's source by `--write-golden` (run it where the reference tree is present; tests/test_maxent.py checks
that the fixtures and the source agree).

Layout (include/gmapdp.h "Device MaxEnt"): 8-byte magic "GMDPMXT1", uint32 table count (16), uint32 0,
then per table in TABLES order: 32-byte NUL-padded name, uint32 entries, uint32 0, entries x float64.

  python3 tools/make_maxent_tables.py [--src maxent_hr.c] [--out gmap-2024_amd/lib/maxent_hr_tables.bin]
  python3 tools/make_maxent_tables.py [--src maxent_hr.c] --write-golden
"""
import argparse
import os
import re
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the order the engine uploads them in (gmapdp_engine.cpp kMaxentTables)
TABLES = [("donor_score_plus", 16384), ("donor_discore_plus", 16),
          ("acc_score1_plus", 16384), ("acc_score2_plus", 16384), ("acc_score3_plus", 16384),
          ("acc_discore_plus", 16), ("acc_score467_plus", 16384), ("acc_score589_plus", 16384),
          ("donor_score_minus", 16384), ("donor_discore_minus", 16),
          ("acc_score1_minus", 16384), ("acc_score2_minus", 16384), ("acc_score3_minus", 16384),
          ("acc_discore_minus", 16), ("acc_score467_minus", 16384), ("acc_score589_minus", 16384)]
MAGIC = b"GMDPMXT1"
GOLDEN = os.path.join(ROOT, "tests", "golden")
STRANDS = ("plus", "minus")   # one fixture file per strand's eight tables


def golden_path(strand, golden=GOLDEN):
    return os.path.join(golden, "maxent_hr_%s.npz" % strand)


def read_golden(golden=GOLDEN):
    """The tables from the stored fixtures, or None where a file is missing."""
    import numpy as np
    out = {}
    for strand in STRANDS:
        if not os.path.exists(golden_path(strand, golden)):
            return None
        with np.load(golden_path(strand, golden)) as z:
            for name, n in TABLES:
                if name.endswith("_" + strand):
                    v = z[name]
                    if v.dtype != np.float64 or v.shape != (n,):
                        raise SystemExit("make_maxent_tables: %s in %s is not %d doubles"
                                         % (name, golden_path(strand, golden), n))
                    out[name] = v.tolist()
    return out


def write_golden(tables, golden=GOLDEN):
    import numpy as np
    for strand in STRANDS:
        np.savez(golden_path(strand, golden), **{name: np.array(tables[name], dtype=np.float64)
                                                 for name, _ in TABLES if name.endswith("_" + strand)})
        print("wrote %s (%d bytes)" % (golden_path(strand, golden), os.path.getsize(golden_path(strand, golden))))


def parse(src):
    text = open(src).read()
    out = {}
    for name, n in TABLES:
        m = re.search(r"static const double %s\[(\d+)\]\s*=\s*\{(.*?)\};" % name, text, re.S)
        if not m:
            raise SystemExit("make_maxent_tables: table %s not found in %s" % (name, src))
        if int(m.group(1)) != n:
            raise SystemExit("make_maxent_tables: %s has %s entries, expected %d" % (name, m.group(1), n))
        vals = [float(x) for x in m.group(2).replace("\n", " ").split(",") if x.strip()]
        if len(vals) != n:
            raise SystemExit("make_maxent_tables: %s: %d initialisers, expected %d" % (name, len(vals), n))
        out[name] = vals
    return out


def write(tables, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(MAGIC + struct.pack("<II", len(TABLES), 0))
        for name, n in TABLES:
            f.write(name.encode().ljust(32, b"\0") + struct.pack("<II", n, 0))
            f.write(struct.pack("<%dd" % n, *tables[name]))
    os.replace(tmp, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default="/root/reference/src/maxent_hr.c")
    ap.add_argument("--out", default=os.path.join(ROOT, "gmap-2024_amd", "lib", "maxent_hr_tables.bin"))
    ap.add_argument("--golden", default=GOLDEN, help="directory of the stored fixtures maxent_hr_{plus,minus}.npz")
    ap.add_argument("--write-golden", action="store_true", help="record the fixtures from --src instead of --out")
    a = ap.parse_args()
    if a.write_golden:
        write_golden(parse(a.src), a.golden)
        return 0
    if os.path.exists(a.src):
        tables = parse(a.src)
    else:
        tables = read_golden(a.golden)
        if tables is None:
            raise SystemExit("make_maxent_tables: neither %s nor the fixtures in %s found" % (a.src, a.golden))
        print("make_maxent_tables: %s absent, taking the tables from %s" % (a.src, a.golden))
    write(tables, a.out)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
