"""Shared pieces of the Stage2_compute_one / Stage2_compute_ends tests (gmapdp_stage2x_batch):

* ``S2XOracle`` -- tests/s2xoracle/libgmapdp_s2xoracle.so, the chain oracle of the two calls with its per-call
  rule counters;
* the goldens tests/golden/stage2x_golden.npz (tests/golden/make_stage2x.py: the reference's own functions);
* the call generators: the shapes stage 3 makes (a segment across a dual break, an unaligned 3' end) over a
  repeat-rich two-chromosome genome, and the edge shapes;
* the comparison of an engine batch with the oracle's batch.

Everything is seeded; what the lru_cache'd functions return must not be modified."""
import ctypes as C
import functools
import os
import random

import numpy as np

from dpbind import Oracle, Pair, S2B_PATHS, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S2XORACLE_SO = os.path.join(ROOT, "tests", "s2xoracle", "libgmapdp_s2xoracle.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage2x_golden.npz")
ONE, ENDS = 1, 2                      # GMAPDP_S2X_ONE, GMAPDP_S2X_ENDS
KIND_NAMES = {ONE: "one", ENDS: "ends"}
COUNTERS = ("restart", "zero_early", "big_position", "tied_cells", "eliminated", "first_kept", "gapholder")
# the kinds each counter applies to (ENDS has no gap holders; ONE neither restarts nor filters)
COUNTER_KINDS = {"restart": (ENDS,), "zero_early": (ENDS,), "big_position": (ONE, ENDS), "tied_cells": (ONE, ENDS),
                 "eliminated": (ENDS,), "first_kept": (ENDS,), "gapholder": (ONE,)}
PAIR_CAP, PATH_CAP = 1 << 16, 256

_ONE_ARGS = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
             C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(Pair), C.c_int, C.POINTER(C.c_long)]


class S2XOracle:
    """The oracle of the two calls.  It reads the genome of the process's libgmapdp_oracle.so, i.e. of `orc` (a
    dpbind.Oracle): set the genome there (set_genome)."""

    def __init__(self, orc=None):
        self.orc = orc or Oracle()
        self.lib = C.CDLL(S2XORACLE_SO)
        self._f = {ONE: self.lib.orc_stage2_one, ENDS: self.lib.orc_stage2_ends}
        for f in self._f.values():
            f.argtypes = _ONE_ARGS
            f.restype = C.c_int
        self.lib.orc_stage2x_batch.restype = C.c_int
        self._sc = (C.c_int * 8)()
        self._paths = (C.c_int * (2 * PATH_CAP))()
        self._pairs = (Pair * PAIR_CAP)()

    def set_genome(self, g):
        self.orc.set_genome(g)

    def compute(self, p, kind=None, counters=None):
        """(number of lists, [pair-key list per list], scalars) or ("err", code).  counters: a ctypes long array
        of len(COUNTERS) that the call's rule counts are added to."""
        kind = kind or p["kind"]
        cnt = counters if counters is not None else (C.c_long * len(COUNTERS))()
        r = self._f[kind](p["q"], p["quc"], len(p["quc"]), int(p.get("query_offset", 0)), C.c_uint(p["chrstart"]),
                          C.c_uint(p["chrend"]), C.c_uint(p["chroffset"]), C.c_uint(p["chrhigh"]), int(p["plusp"]),
                          int(p.get("splicingp", 1)), int(p.get("maxintronlen", 500000)), self._sc, self._paths,
                          PATH_CAP, self._pairs, PAIR_CAP, cnt)
        if r < 0:
            return ("err", r)
        pr, pa = self._pairs, self._paths
        return r, [[pr[pa[2 * i] + j].key() for j in range(pa[2 * i + 1])] for i in range(r)], tuple(self._sc[:6])

    def counters(self, p, kind=None):
        cnt = (C.c_long * len(COUNTERS))()
        self.compute(p, kind, cnt)
        return dict(zip(COUNTERS, cnt))

    def batch(self, kind, probs, qbuf, qucbuf, nthreads=None):
        """orc_stage2x_batch over gmapdp.STAGE2X_PROBLEM_DTYPE problems on the oracle's current genome, in
        dpbind.oracle_stage2_batch's format: (scalars (n, 8), paths (n, S2B_PATHS, 2), pairs (20-B records),
        pair_off (n + 1))."""
        n = len(probs)
        ql = probs["querylength"].astype(np.int64)
        pair_off = np.zeros(n + 1, dtype=np.int64)
        pair_off[1:] = np.cumsum(8 * ql + 256)
        col = lambda k, dt: np.ascontiguousarray(probs[k], dtype=dt)  # noqa: E731
        args = [col("qoff", np.int32), col("querylength", np.int32), col("query_offset", np.int32),
                col("chrstart", np.uint32), col("chrend", np.uint32), col("chroffset", np.uint32),
                col("chrhigh", np.uint32), col("plusp", np.int32), col("splicingp", np.int32),
                col("maxintronlen", np.int32)]
        scal = np.zeros((n, 8), dtype=np.int32)
        paths = np.zeros((n, S2B_PATHS, 2), dtype=np.int32)
        pairs = np.zeros(int(pair_off[-1]) * 20 + 20, dtype=np.uint8)
        nt = nthreads or min(16, os.cpu_count() or 4)
        self.lib.orc_stage2x_batch(C.c_int(kind), C.c_int(n), C.c_char_p(qbuf), C.c_char_p(qucbuf),
                                   *[C.c_void_p(a.ctypes.data) for a in args], C.c_void_p(scal.ctypes.data),
                                   C.c_void_p(paths.ctypes.data), C.c_int(S2B_PATHS), C.c_void_p(pairs.ctypes.data),
                                   C.c_void_p(pair_off.ctypes.data), C.c_int(nt))
        return scal, paths, pairs, pair_off


# ---------------------------------------------------------------------------------------------------------
# The genome and the calls
# ---------------------------------------------------------------------------------------------------------
CHROMS = ((0, 30000), (30011, 60000))   # [chroffset, end): the second offset is odd
# tandem repeats: (start in the genome, unit length, copies) -- 100 to 250 copies, so that a window holding one
# gives its 8-mers 100 or more hits (Count_T is an unsigned char)
REPEATS = ((4000, 5, 180), (12000, 9, 120), (21000, 3, 240), (34000, 7, 150), (47000, 11, 110))
# short tandem repeats: (start, unit length, copies, start of three more copies further on) -- a query of three
# units ties at both shifts of the four copies, which overlap by two thirds (the second list is eliminated), and
# at the three copies further on (kept: several lists returned)
SMALL_REPEATS = ((27000, 12, 4, 27300), (58000, 10, 4, 58200))
# duplicated segments: (source, destination, length) -- a query from one matches both alike (tied cells)
DUPS = ((7000, 9000, 400), (16000, 24500, 300), (38000, 41000, 500), (52000, 56000, 250))


@functools.lru_cache(maxsize=None)
def genome():
    rng = random.Random(20240621)
    g = bytearray(rng.choice(b"ACGT") for _ in range(CHROMS[-1][1]))
    for at, u, c, *more in REPEATS + SMALL_REPEATS:
        unit = bytes(rng.choice(b"ACGT") for _ in range(u))
        while len(set(unit)) < 2:
            unit = bytes(rng.choice(b"ACGT") for _ in range(u))
        g[at:at + u * c] = unit * c
        for m in more:
            g[m:m + 3 * u] = unit * 3
    for a, b, n in DUPS:
        g[b:b + n] = g[a:a + n]
    for at in (2500, 33000):   # a few N
        g[at:at + 3] = b"NNN"
    return bytes(g)


def _chrom_of(pos):
    for co, end in CHROMS:
        if co <= pos < end:
            return co, end - 1
    raise ValueError(pos)


def _mutate(rng, s, rate):
    s = bytearray(s)
    for i in range(len(s)):
        if rng.random() < rate:
            s[i] = rng.choice(b"ACGT")
    return s


def _lower_some(rng, q):
    ql = bytearray(q)
    for j in range(len(ql)):
        if rng.random() < 0.05:
            ql[j] = ord(chr(ql[j]).lower())
    return bytes(ql)


def _call(kind, q, co, chrhigh, ws, we, plusp, rng, query_offset=None):
    """One call: query q in genome orientation (reverse-complemented here for the minus strand), the window
    [ws, we] in genome coordinates of the chromosome at offset co."""
    q = bytes(q)
    if not plusp:
        q = revcomp(q)
    return dict(kind=kind, q=_lower_some(rng, q), quc=q, chrstart=ws - co, chrend=we - co, chroffset=co,
                chrhigh=chrhigh, plusp=int(plusp), splicingp=0 if rng.random() < 0.25 else 1,
                maxintronlen=rng.choice([500000, 500000, 2000, 200]),
                query_offset=rng.choice([0, 0, 1, 37, 512, 2999]) if query_offset is None else query_offset)


def random_call(rng, kind, g=None):
    """A call of the shapes stage 3 makes.  ONE: a 20-300-nt segment across a break (two pieces of the window,
    sometimes with a few query nucleotides between them that the genome lacks); ENDS: a 11-250-nt 3' end whose
    head often does not match the window (a diverged tail: positions without a predecessor) and whose rest
    does.  Either may lie over a tandem repeat or a duplicated segment."""
    g = g or genome()
    u = rng.random()
    plusp = rng.random() < 0.5
    if u < 0.06:       # three or four units of a short tandem repeat: tied, partly overlapping chains
        at, unit, c, more = rng.choice(SMALL_REPEATS)
        co, chrhigh = _chrom_of(at)
        ws, we = at - rng.randint(20, 800), more + 3 * unit + rng.randint(20, 800)
        q = bytearray(g[at:at + 3 * unit])
    elif u < 0.25:     # over a tandem repeat: 100 or more hits per position, tied and overlapping chains
        at, unit, c = rng.choice(REPEATS)
        co, chrhigh = _chrom_of(at)
        ws = max(co, at - rng.randint(50, 1500))
        we = min(chrhigh, at + unit * c + rng.randint(50, 1500))
        a = at - rng.randint(0, 60)
        b = at + rng.randint(2, 6) * unit + rng.randint(0, 7)
        q = bytearray(g[a:b])
        if rng.random() < 0.5:
            tail = at + unit * c
            q += g[tail:tail + rng.randint(10, 80)]
    elif u < 0.45:     # from a duplicated segment, the window over both copies
        a0, b0, n = rng.choice(DUPS)
        co, chrhigh = _chrom_of(a0)
        ws = max(co, a0 - rng.randint(100, 2000))
        we = min(chrhigh, b0 + n + rng.randint(100, 2000))
        s = a0 + rng.randint(0, n - 60)
        q = bytearray(g[s:s + rng.randint(20, min(200, a0 + n - s))])
    else:
        co, end = rng.choice(CHROMS)
        chrhigh = end - 1
        wl = rng.choice([rng.randint(30, 300), rng.randint(300, 5000), rng.randint(5000, 25000)])
        ws = rng.randint(co, end - 1 - wl)
        we = ws + wl
        if rng.random() < 0.1:
            ws, we = (co, co + wl) if rng.random() < 0.5 else (chrhigh - wl, chrhigh)   # at a chromosome's end
        n1 = rng.randint(12, 150)
        s1 = rng.randint(ws, max(ws, we - n1))
        q = bytearray(g[s1:min(s1 + n1, we + 1)])
        if rng.random() < 0.6 and we - (s1 + n1) > 40:   # a second piece further on (an indel or an intron)
            gap = rng.choice([rng.randint(1, 30), rng.randint(30, max(31, min(4000, we - s1 - n1 - 20)))])
            s2 = s1 + n1 + gap
            if rng.random() < 0.3:
                q += bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 12)))
            q += g[s2:min(s2 + rng.randint(12, 150), we + 1)]
    q = _mutate(rng, q, rng.choice([0.0, 0.01, 0.04]))
    if kind == ENDS and rng.random() < 0.5:   # a diverged head
        q = bytearray(rng.choice(b"ACGT") for _ in range(rng.randint(3, 40))) + q
    if len(q) < 9:
        q += bytes(rng.choice(b"ACGT") for _ in range(9 - len(q)))
    q = q[:300]
    return _call(kind, q, co, chrhigh, ws, we, plusp, rng)


def random_calls(kind, n, seed):
    rng = random.Random(seed * 7 + kind)
    return [random_call(rng, kind) for _ in range(n)]


def edge_calls(kind):
    """The edge shapes: querylength 9, 10 and 64; windows of 8 nt, chrend == chrstart and chrend == chrstart - 1;
    a window without hits; exactly one hit; a position with exactly 99 and exactly 100 hits; a tail whose first
    scored position restarts (every ENDS call with hits); tied best cells; query_offset 0 and non-zero; the
    minus strand at a chromosome's far end."""
    g = genome()
    rng = random.Random(99 + kind)
    out = []
    co, end = CHROMS[1]
    chrhigh = end - 1
    for ql in (9, 10, 64):
        s = co + 5000
        for plusp in (1, 0):
            out.append(_call(kind, g[s:s + ql], co, chrhigh, s - 40, s + ql + 40, plusp, rng, query_offset=ql % 2 * 17))
    s = co + 6000
    out.append(_call(kind, g[s:s + 30], co, chrhigh, s + 4, s + 12, 1, rng, 0))        # an 8-nt window: one 8-mer
    out.append(_call(kind, g[s:s + 30], co, chrhigh, s + 4, s + 11, 0, rng, 5))        # minus: chrend + 1 - chrstart = 8
    out.append(_call(kind, g[s:s + 30], co, chrhigh, s + 4, s + 4, 1, rng, 0))         # chrend == chrstart
    out.append(_call(kind, g[s:s + 30], co, chrhigh, s + 4, s + 4, 0, rng, 0))
    out.append(_call(kind, g[s:s + 30], co, chrhigh, s + 5, s + 4, 1, rng, 3))         # chrend == chrstart - 1
    out.append(_call(kind, g[s:s + 30], co, chrhigh, s + 5, s + 4, 0, rng, 3))
    out.append(_call(kind, b"ACGTTGCA" * 4, co, chrhigh, co + 8000, co + 8000 + 200, 1, rng, 0))  # (very likely) no hits
    # exactly one hit: a 9-nt query whose first 8-mer occurs once in a small window (its second 8-mer does not)
    out.append(_call(kind, g[s:s + 8] + bytes([ord("A") if g[s + 8] != ord("A") else ord("C")]), co, chrhigh, s - 20,
                     s + 28, 1, rng, 11))
    # a tandem repeat window cut to hold exactly 99 and exactly 100 copies of the unit's 8-mers
    at, unit, c = REPEATS[3]                  # on the second chromosome, unit 7
    for copies in (99, 100):
        for plusp in (1, 0):
            # 8-mers starting in [ws, we - 8] (plus; minus likewise over chrend + 1): `copies` starts of each phase
            ws = at
            we = at + unit * (copies - 1) + 8 + (unit - 1)
            q = g[at:at + 2 * unit + 8]
            out.append(_call(kind, q, co, chrhigh, ws, we if plusp else we - 1, plusp, rng, 0))
    # tied best cells: a query from a duplicated segment, the window over both copies
    a0, b0, n = DUPS[2]
    for plusp in (1, 0):
        out.append(_call(kind, g[a0 + 50:a0 + 120], co, chrhigh, a0 - 200, b0 + n + 200, plusp, rng, 250))
    # several lists kept: three units of a short tandem repeat
    at, unit, c, more = SMALL_REPEATS[1]
    for plusp in (1, 0):
        out.append(_call(kind, g[at:at + 3 * unit], co, chrhigh, at - 300, more + 3 * unit + 300, plusp, rng, 40))
    # the minus strand at the chromosome's far end (chrinit = (chrhigh - chroffset) - chrend = 0)
    out.append(_call(kind, g[chrhigh - 100:chrhigh - 20], co, chrhigh, chrhigh - 400, chrhigh, 0, rng, 1000))
    out.append(_call(kind, g[chrhigh - 60:chrhigh + 1], co, chrhigh, chrhigh - 90, chrhigh, 0, rng, 0))
    for p in out:
        p["splicingp"] = 1
        p["maxintronlen"] = 500000
    return out


# ---------------------------------------------------------------------------------------------------------
# Goldens
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    """(genome, calls, expected, counters): expected[i] = (number of lists, [pair-key list per list]) from the
    reference's own function, counters[i] = the oracle's rule counts of call i (COUNTERS order)."""
    z = np.load(GOLDEN)
    g = z["genome"].tobytes()
    c, qs, qu = z["calls"], z["qseq"].tobytes(), z["quc"].tobytes()
    lists, pairs = z["lists"], z["pairs"]
    calls, expected = [], []
    for i in range(len(c)):
        r = c[i]
        a, n = int(r["qoff"]), int(r["querylength"])
        calls.append(dict(kind=int(r["kind"]), q=qs[a:a + n], quc=qu[a:a + n], chrstart=int(r["chrstart"]),
                          chrend=int(r["chrend"]), chroffset=int(r["chroffset"]), chrhigh=int(r["chrhigh"]),
                          plusp=int(r["plusp"]), splicingp=int(r["splicingp"]), maxintronlen=int(r["maxintronlen"]),
                          query_offset=int(r["query_offset"])))
        ls = []
        for k in range(int(r["list_off"]), int(r["list_off"]) + int(r["nlists"])):
            o, m = int(lists[k]["pair_off"]), int(lists[k]["npairs"])
            ls.append([(int(x["querypos"]), int(x["genomepos"]), int(x["queryjump"]), int(x["genomejump"]),
                        int(x["dynprogindex"]), bytes(x["cdna"]) or b"\0", bytes(x["comp"]) or b"\0",
                        bytes(x["genome"]) or b"\0", bytes(x["genomealt"]) or b"\0", int(x["gapp"]))
                       for x in pairs[o:o + m]])
        expected.append((int(r["nlists"]), ls))
    return g, tuple(calls), tuple(expected), z["counters"]


# ---------------------------------------------------------------------------------------------------------
# Engine against oracle
# ---------------------------------------------------------------------------------------------------------
def engine_lists(results, paths, pairs):
    """An engine batch in the oracle's single-call format: [(number of lists, [pair-key list per list])]."""
    out = []
    for r in results:
        ls = []
        for k in range(int(r["nresults"])):
            pr = paths[int(r["path_offset"]) + k]
            o, m = int(pr["pair_offset"]), int(pr["npairs"])
            ls.append([(int(x["querypos"]), int(x["genomepos"]), int(x["queryjump"]), int(x["genomejump"]), 0,
                        bytes(x["cdna"]) or b"\0", bytes(x["comp"]) or b"\0", bytes(x["genome"]) or b"\0",
                        bytes(x["genomealt"]) or b"\0", 1 if x["querypos"] == -1 and x["genomepos"] == -1 else 0)
                       for x in pairs[o:o + m]])
        out.append((int(r["nresults"]), ls))
    return out


def by_kind(calls):
    """{kind: [index into calls]}"""
    d = {}
    for i, p in enumerate(calls):
        d.setdefault(int(p["kind"]), []).append(i)
    return d
