"""Shared pieces of the Stage2_compute_starts tests (gmapdp_stage2x_batch, kind GMAPDP_S2X_STARTS):

* ``S2SOracle`` -- tests/s2soracle/libgmapdp_s2soracle.so, the lookforward chain oracle with its per-call rule
  counters;
* the goldens tests/golden/stage2_starts_golden.npz (tests/golden/make_stage2_starts.py: the reference's own
  function);
* the call generators over s2x.genome(): the shape stage 3 makes (an unaligned 5' end, whose 3' part adjoins
  the aligned region and whose 5' part may not match the window at all) and the edge shapes;
* the mirror of a call: the ENDS call on the reverse-complemented query and the opposite strand.

Everything is seeded; what the lru_cache'd functions return must not be modified."""
import ctypes as C
import functools
import os
import random

import numpy as np

import s2x
from dpbind import Oracle, Pair, S2B_PATHS, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S2SORACLE_SO = os.path.join(ROOT, "tests", "s2soracle", "libgmapdp_s2soracle.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage2_starts_golden.npz")
STARTS = 3                            # GMAPDP_S2X_STARTS
COUNTERS = ("restart", "zero_early", "big_position", "tied_cells", "eliminated", "first_kept", "pruned")
PAIR_CAP, PATH_CAP = 1 << 16, 256

_ARGS = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
         C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(Pair), C.c_int, C.POINTER(C.c_long)]


class S2SOracle:
    """The oracle of Stage2_compute_starts.  It reads the genome of the process's libgmapdp_oracle.so, i.e. of
    `orc` (a dpbind.Oracle): set the genome there (set_genome)."""

    def __init__(self, orc=None):
        self.orc = orc or Oracle()
        self.lib = C.CDLL(S2SORACLE_SO)
        self.lib.orc_stage2_starts.argtypes = _ARGS
        self.lib.orc_stage2_starts.restype = C.c_int
        self.lib.orc_stage2s_batch.restype = C.c_int
        self._sc = (C.c_int * 8)()
        self._paths = (C.c_int * (2 * PATH_CAP))()
        self._pairs = (Pair * PAIR_CAP)()

    def set_genome(self, g):
        self.orc.set_genome(g)

    def compute(self, p, counters=None):
        """(number of lists, [pair-key list per list], scalars) or ("err", code).  counters: a ctypes long array
        of len(COUNTERS) that the call's rule counts are added to."""
        cnt = counters if counters is not None else (C.c_long * len(COUNTERS))()
        r = self.lib.orc_stage2_starts(p["q"], p["quc"], len(p["quc"]), int(p.get("query_offset", 0)),
                                       C.c_uint(p["chrstart"]), C.c_uint(p["chrend"]), C.c_uint(p["chroffset"]),
                                       C.c_uint(p["chrhigh"]), int(p["plusp"]), int(p.get("splicingp", 1)),
                                       int(p.get("maxintronlen", 500000)), self._sc, self._paths, PATH_CAP,
                                       self._pairs, PAIR_CAP, cnt)
        if r < 0:
            return ("err", r)
        pr, pa = self._pairs, self._paths
        return r, [[pr[pa[2 * i] + j].key() for j in range(pa[2 * i + 1])] for i in range(r)], tuple(self._sc[:6])

    def counters(self, p):
        cnt = (C.c_long * len(COUNTERS))()
        self.compute(p, cnt)
        return dict(zip(COUNTERS, cnt))

    def batch(self, probs, qbuf, qucbuf, nthreads=None):
        """orc_stage2s_batch over gmapdp.STAGE2X_PROBLEM_DTYPE problems on the oracle's current genome, in
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
        self.lib.orc_stage2s_batch(C.c_int(n), C.c_char_p(qbuf), C.c_char_p(qucbuf),
                                   *[C.c_void_p(a.ctypes.data) for a in args], C.c_void_p(scal.ctypes.data),
                                   C.c_void_p(paths.ctypes.data), C.c_int(S2B_PATHS), C.c_void_p(pairs.ctypes.data),
                                   C.c_void_p(pair_off.ctypes.data), C.c_int(nt))
        return scal, paths, pairs, pair_off


# ---------------------------------------------------------------------------------------------------------
# The calls
# ---------------------------------------------------------------------------------------------------------
genome = s2x.genome


def _append(p, tail):
    """p with `tail` (upper case, query orientation) appended to its query."""
    p = dict(p)
    p["q"], p["quc"] = p["q"] + tail, p["quc"] + tail
    return p


def _prepend(p, head):
    p = dict(p)
    p["q"], p["quc"] = head + p["q"], head + p["quc"]
    return p


def random_call(rng):
    """An unaligned 5' end as stage 3 hands it over: s2x's segment shapes (one or two pieces of the window, a
    tandem repeat, a duplicated segment), half of them with a diverged 5' part (positions whose hits find
    nothing further 3' to link to lie at the other end: a diverged 3' part, a quarter of them)."""
    p = s2x.random_call(rng, s2x.ONE)
    p["kind"] = STARTS
    u = rng.random()
    if u < 0.5:
        p = _prepend(p, bytes(rng.choice(b"ACGT") for _ in range(rng.randint(3, 40))))
    if rng.random() < 0.25:
        p = _append(p, bytes(rng.choice(b"ACGT") for _ in range(rng.randint(3, 40))))
    p["q"], p["quc"] = p["q"][:300], p["quc"][:300]
    return p


def random_calls(n, seed):
    rng = random.Random(seed * 7 + STARTS)
    return [random_call(rng) for _ in range(n)]


def _edge(g, q, co, chrhigh, ws, we, plusp, rng, query_offset=0, splicingp=1, maxintronlen=500000):
    p = s2x._call(STARTS, q, co, chrhigh, ws, we, plusp, rng, query_offset)
    p["splicingp"], p["maxintronlen"] = splicingp, maxintronlen
    return p


@functools.lru_cache(maxsize=None)
def edge_calls():
    """(calls, tags): s2x.edge_calls' shapes as STARTS calls (querylength 9, 10 and 64; windows of 8 nt, chrend ==
    chrstart and chrend == chrstart - 1; no hits; exactly one hit; positions with 99 and 100 hits; tied best cells;
    overlapping and separate lists; query_offset 0 and non-zero), then: positions with exactly 64 and with 70 hits;
    a query whose last three 8-mers have no hit, and one whose first eight have none; both strands at a window
    starting at chromosome position 0 and at one ending at the chromosome's last position; two pieces 3 000 nt
    apart with maxintronlen above and below that, with and without splicing; a short 5' piece before an indel.
    tags[i] names what call i is there
    for ("" for s2x's shapes)."""
    g = genome()
    rng = random.Random(99 + STARTS)
    calls = []
    for p in s2x.edge_calls(s2x.ENDS):
        p = dict(p)
        p["kind"] = STARTS
        calls.append(p)
    tags = [""] * len(calls)
    co, end = s2x.CHROMS[1]
    chrhigh = end - 1
    at, unit, c = s2x.REPEATS[3]                  # on the second chromosome, unit 7
    for copies in (64, 70):
        for plusp in (1, 0):
            we = at + unit * (copies - 1) + 8 + (unit - 1)
            calls.append(_edge(g, g[at:at + 2 * unit + 8], co, chrhigh, at, we if plusp else we - 1, plusp, rng))
            tags.append("hits%d" % copies)
    s = co + 11000
    for plusp in (1, 0):
        # in genome orientation; the minus call's query is the reverse complement, so its ends swap
        q = bytearray(g[s:s + 48])
        q[48 - 3 if plusp else 2] = ord("A") if q[48 - 3 if plusp else 2] != ord("A") else ord("C")
        calls.append(_edge(g, q, co, chrhigh, s - 60, s + 110, plusp, rng, query_offset=7))
        tags.append("tail_nohit")
        q = bytearray(g[s:s + 48])
        q[7 if plusp else 48 - 8] = ord("A") if q[7 if plusp else 48 - 8] != ord("A") else ord("C")
        calls.append(_edge(g, q, co, chrhigh, s - 60, s + 110, plusp, rng))
        tags.append("head_nohit")
    for plusp in (1, 0):
        calls.append(_edge(g, g[co:co + 60], co, chrhigh, co, co + 300, plusp, rng))
        tags.append("chrstart0")
        calls.append(_edge(g, g[chrhigh - 59:chrhigh + 1], co, chrhigh, chrhigh - 300, chrhigh, plusp, rng, query_offset=3))
        tags.append("chrlast")
    s = co + 13000
    for plusp in (1, 0):
        for splicingp in (1, 0):
            for mil in (2000, 500000):
                calls.append(_edge(g, g[s:s + 40] + g[s + 3040:s + 3100], co, chrhigh, s - 200, s + 3300, plusp, rng,
                                   splicingp=splicingp, maxintronlen=mil))
                tags.append("intron_%s_%d" % ("long" if mil == 2000 else "short", splicingp))
    s = co + 15000
    # an 11-nt piece, 5 nt of the genome skipped, a 50-nt piece: were the short piece's hits to link across the
    # indel, their chain would count fewer than MIN_TERMINAL_NCONSECUTIVE matches and the traceback would prune it.
    # They do not (with localp and middlep false only adjacent hits link), so `pruned` stays 0.
    for plusp in (1, 0):
        calls.append(_edge(g, g[s:s + 11] + g[s + 16:s + 66], co, chrhigh, s - 100, s + 200, plusp, rng))
        tags.append("short5p_indel")
    return tuple(calls), tuple(tags)


# ---------------------------------------------------------------------------------------------------------
# The mirror: a STARTS call as an ENDS call
# ---------------------------------------------------------------------------------------------------------
_COMP = bytes.maketrans(b"ACGTacgtNn", b"TGCAtgcaNn")


def mirrored_ends_call(p):
    """The ENDS call whose chain is p's seen from the other strand: the reverse-complemented query on the opposite
    strand of the same window, query_offset 0."""
    m = dict(p)
    m["kind"] = s2x.ENDS
    m["q"], m["quc"] = p["q"].translate(_COMP)[::-1], revcomp(p["quc"])
    m["plusp"] = 0 if p["plusp"] else 1
    m["query_offset"] = 0
    return m


def unmirror_lists(p, lists):
    """The ENDS lists of mirrored_ends_call(p) taken back to p's strand: positions mapped back and characters
    complemented, pair by pair.  An ENDS list runs 5' end first on the mirrored strand, which on p's strand is
    3' end first, the order of a STARTS list: mapping the positions is the reversal."""
    ql, chrlength = len(p["quc"]), p["chrhigh"] - p["chroffset"] + 1
    qo = int(p.get("query_offset", 0))
    out = []
    for lst in lists:
        out.append([(ql - 1 - k[0] + qo, chrlength - 1 - k[1]) + k[2:5] + tuple(x.translate(_COMP) for x in k[5:9]) +
                    k[9:] for k in lst])
    return out


# ---------------------------------------------------------------------------------------------------------
# Goldens
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    """(genome, calls, expected, counters): expected[i] = (number of lists, [pair-key list per list]) from the
    reference's own Stage2_compute_starts, counters[i] = the oracle's rule counts of call i (COUNTERS order)."""
    z = np.load(GOLDEN)
    g = z["genome"].tobytes()
    c, qs, qu = z["calls"], z["qseq"].tobytes(), z["quc"].tobytes()
    lists, pairs = z["lists"], z["pairs"]
    calls, expected = [], []
    for i in range(len(c)):
        r = c[i]
        a, n = int(r["qoff"]), int(r["querylength"])
        calls.append(dict(kind=STARTS, q=qs[a:a + n], quc=qu[a:a + n], chrstart=int(r["chrstart"]),
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


engine_lists = s2x.engine_lists


def strip_dynprogindex(ev):
    """An oracle or golden result with the pairs' dynprogindex zeroed (the engine's records carry none)."""
    return ev[0], [[k[:4] + (0,) + k[5:] for k in lst] for lst in ev[1]]
