#!/usr/bin/env python3
"""Writes tests/golden/long_query_golden.npz: the reference's (oracle/_ref) seeding and Stage2_compute outputs
for two long-query calls of tests/longq.py -- the first spliced read (case B, plus strand) and the count-wrap
read on the minus strand (case D).  Windows are below 60 kb, so the file stays well under 1 MB.

    python tests/golden/make_long_query.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import longq  # noqa: E402
from dpbind import Ref  # noqa: E402


def golden_calls(g):
    return [longq.spliced_calls(g)[0][0], longq.wrap_calls(g)[1]]


def pack(impl, calls):
    """The arrays of one implementation's outputs on `calls` (the fixture's format)."""
    out = {}
    for i, c in enumerate(calls):
        sc, npos, pos, dg = impl.oligo_mappings(c)
        out["om%d_scalars" % i] = np.array(sc, dtype=np.int32)
        out["om%d_npositions" % i] = np.array(npos, dtype=np.uint8 if max(npos) < 256 else np.int32)
        out["om%d_positions" % i] = np.array(pos, dtype=np.uint32)
        out["om%d_diagonals" % i] = np.array(dg, dtype=np.int32).reshape(-1, 4)
        n, lists = impl.stage2_compute(c)
        out["s2%d_nresults" % i] = np.array([n], dtype=np.int32)
        out["s2%d_lengths" % i] = np.array([len(x) for x in lists], dtype=np.int32)
        # (querypos, genomepos, queryjump, genomejump, dynprogindex, gapp) and the four characters of every pair
        flat = [p for lst in lists for p in lst]
        out["s2%d_ints" % i] = np.array([p[:5] + (p[9],) for p in flat], dtype=np.int32).reshape(-1, 6)
        out["s2%d_chars" % i] = np.frombuffer(b"".join(p[5][:1] + p[6][:1] + p[7][:1] + p[8][:1] for p in flat),
                                              dtype=np.uint8).reshape(-1, 4)
    return out


def main():
    g = longq.genome()
    ref = Ref()
    ref.set_genome(g)
    out = pack(ref, golden_calls(g))
    path = os.path.join(HERE, "long_query_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
