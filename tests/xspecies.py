"""Shared pieces of the cross-species (gmap --cross-species, GMAPDP_S2_CANONICAL_MIDDLE) tests:

* ``XOracle`` -- tests/xoracle/libgmapdp_xoracle.so, the chain oracle with the flag and the canonical-link
  predicate written as the reference writes it (two descending walks merged by shift);
* the predicate grid: a ~3-kb two-chromosome genome with planted sites, the (prevpos, currpos) pairs and a
  brute-force form of the predicate (string compares per shift);
* the chain generator: spliced reads whose stage-2 chains depend on the flag.

Everything is seeded and computed once per process (lru_cache); callers must not modify what they get."""
import ctypes as C
import functools
import os
import random

import numpy as np

from dpbind import Oracle, Pair, Ref, S2_PAIR_CAP, S2_PATH_CAP, ref_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XORACLE_SO = os.path.join(ROOT, "tests", "xoracle", "libgmapdp_xoracle.so")
CANONICAL_MIDDLE = 1  # GMAPDP_S2_CANONICAL_MIDDLE
GREEDY_ADVANCE, MISS_BEHIND = 6, 16

# strong consensus sites (the genome-gap generator's, dpbind.genome_gap_problem): MaxEnt probabilities near 1
DONOR = b"CAG" + b"GTAAGT"                       # GT at +3: donor position = start + 3
ACCEPTOR = b"TTCTTTTCTTTCTTTTCCAG" + b"GTA"      # AG at +18: acceptor position = start + 20
BOTH = b"TTCTTTTCTTTCTTTTCCAG" + b"GTAAGT"       # an acceptor and a donor at the same position, start + 20
_RC = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s):
    return bytes(s).translate(_RC)[::-1]


ANTIACCEPTOR = revcomp(ACCEPTOR)                 # CT at +3: antiacceptor position = start + 3
ANTIDONOR = revcomp(DONOR)                       # AC at +4: antidonor position = start + 6
ANTIBOTH = revcomp(BOTH)                         # AC at +4, CT at +6: both positions = start + 6


class XOracle:
    """The cross-species chain oracle.  It reads the genome and MaxEnt tables of the process's
    libgmapdp_oracle.so, i.e. of `orc` (a dpbind.Oracle): set the genome there."""

    def __init__(self, orc=None):
        self.orc = orc or Oracle()
        self.orc.maxent(0, 0)  # loads the MaxEnt tables into libgmapdp_oracle.so
        self.lib = C.CDLL(XORACLE_SO)
        f = self.lib.xorc_stage2_compute
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
                      C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(Pair), C.c_int]
        f.restype = C.c_int
        self.lib.xorc_canonical_links.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_ulonglong, C.c_void_p]
        self.lib.xorc_canonical_links.restype = None
        self.lib.xorc_stage2_stats.argtypes = [C.POINTER(C.c_long)]
        self._sc = (C.c_int * 8)()
        self._paths = (C.c_int * (2 * S2_PATH_CAP))()
        self._pairs = (Pair * S2_PAIR_CAP)()

    def set_genome(self, g):
        self.orc.set_genome(g)

    def stage2_compute(self, p, flags=0):
        """dpbind's Oracle.stage2_compute format: (number of results, [pair-key list per result])."""
        r = self.lib.xorc_stage2_compute(p["q"], p["quc"], len(p["quc"]), C.c_uint(p["chrstart"]),
                                         C.c_uint(p["chrend"]), C.c_uint(p["chroffset"]), C.c_uint(p["chrhigh"]),
                                         int(p["plusp"]), int(p.get("splicingp", 1)),
                                         int(p.get("maxintronlen", 500000)), int(flags), self._sc, self._paths,
                                         S2_PATH_CAP, self._pairs, S2_PAIR_CAP)
        if r < 0:
            return ("err", r)
        pr, pa = self._pairs, self._paths
        return r, [[pr[pa[2 * i] + j].key() for j in range(pa[2 * i + 1])] for i in range(r)]

    def canonical_links(self, prevpos, currpos, plusp, chroffset):
        pp = np.ascontiguousarray(prevpos, dtype=np.uint64)
        cp = np.ascontiguousarray(currpos, dtype=np.uint64)
        out = np.zeros(len(pp), dtype=np.uint8)
        self.lib.xorc_canonical_links(pp.ctypes.data, cp.ctypes.data, len(pp), int(plusp), int(chroffset),
                                      out.ctypes.data)
        return out

    def reset_stats(self):
        self.lib.xorc_stage2_reset_stats()

    def stats(self):
        """Range 2 since reset_stats: (candidates tested, winning links penalised, winning links canonical)."""
        out = (C.c_long * 3)()
        self.lib.xorc_stage2_stats(out)
        return tuple(out)


# ---------------------------------------------------------------------------------------------------------
# The predicate grid
# ---------------------------------------------------------------------------------------------------------
GRID_CHR2 = 1493            # the second chromosome's offset: not a multiple of 32
GRID_LEN = 3001
# seed ends around a site position s: the shifts 0 and 22 and one past each on both strands (plus: the site's
# shift is 16 - (s - pos), minus: 6 - (s - pos)), and some between
GRID_OFFS = (-17, -16, -7, -6, 0, 6, 7, 16, 17)
GRID_OFFS_FEW = (-16, -6, 0, 6, 16)     # the other sites: the window edges and the middle only
GRID_FULL_SITES = (100, 671, 833, 1100, GRID_CHR2 + 150, GRID_CHR2 + 300, GRID_CHR2 + 750, GRID_CHR2 + 1390)


def _put(g, at, motif):
    n = min(len(motif), len(g) - at)  # (a motif at the genome's end is cut there)
    g[at:at + n] = motif[:n]


@functools.lru_cache(maxsize=None)
def grid_genome():
    """(genome, site positions by kind).  Two chromosomes, [0, GRID_CHR2) and [GRID_CHR2, GRID_LEN)."""
    rng = random.Random(20241)
    # (no G or C by chance next to the planted sites would matter; a random background has its own weak sites)
    g = bytearray(rng.choice(b"ACGT") for _ in range(GRID_LEN))
    sites = {"both": [], "antiboth": [], "donor": [], "acceptor": [], "antidonor": [], "antiacceptor": [],
             "straddle": [], "n": []}

    def plant(kind, pos):  # pos: the site position (GT / CT start, or one past AG / AC)
        motif, off = {"both": (BOTH, 20), "antiboth": (ANTIBOTH, 6), "donor": (DONOR, 3), "acceptor": (ACCEPTOR, 20),
                      "antidonor": (ANTIDONOR, 6), "antiacceptor": (ANTIACCEPTOR, 3)}[kind]
        _put(g, pos - off, motif)
        sites[kind].append(pos)

    # combined sites (acceptor and donor at one position): any two of them are canonical at equal shifts
    for pos in (100, 163, 227, 290, 352, 416, 480, 545, 610, 735, 860, 925, 990):
        plant("both", pos)
    for pos in (1100, 1230, 1360):
        plant("antiboth", pos)
    # a dinucleotide straddling two 32-nt blocks: GT at (31, 32) mod 32, AG / AC likewise (site - 2 = 31 mod 32)
    plant("both", 671)                              # GT starts at 671 = 31 mod 32
    sites["straddle"].append(671)
    plant("both", 833)                              # AG starts at 831 = 31 mod 32
    sites["straddle"].append(833)
    # second chromosome: single sites (unequal shifts against each other), combined ones, an N inside a site
    c2 = GRID_CHR2
    plant("donor", c2 + 150)
    plant("acceptor", c2 + 300)
    plant("antiacceptor", c2 + 450)
    plant("antidonor", c2 + 600)
    for pos in (c2 + 750, c2 + 815, c2 + 880, c2 + 945, c2 + 1010, c2 + 1075, c2 + 1140, c2 + 1205):
        plant("both", pos)
    plant("antiboth", c2 + 1270)
    plant("both", c2 + 1390)
    g[c2 + 1390 + 1] = ord("N")                     # GN: the donor dinucleotide holds an N
    sites["n"].append(c2 + 1390)
    plant("both", c2 + 30)                          # within MISS_BEHIND + a window of the chromosome start
    plant("both", GRID_LEN - 3)                     # GT at the last three positions of the genome
    sites["end"] = [GRID_LEN - 3]
    return bytes(g), {k: tuple(v) for k, v in sites.items()}


@functools.lru_cache(maxsize=None)
def grid_pairs(chrom):
    """The seed-end grid of one chromosome (0 or 1): (chroffset, chrhigh, positions ascending).  Every ordered
    pair of them is a case: (prevpos, currpos) = (low, high) on the plus strand, (high, low) on the minus."""
    g, sites = grid_genome()
    lo, hi = (0, GRID_CHR2) if chrom == 0 else (GRID_CHR2, GRID_LEN)
    pos = set()
    for kind, lst in sites.items():
        for s in lst:
            if lo <= s < hi:
                for o in (GRID_OFFS if s in GRID_FULL_SITES else GRID_OFFS_FEW):
                    if lo <= s - o < hi:
                        pos.add(s - o)
    # within 6 and 16 of the chromosome start, and within 3 of its end
    pos.update(lo + d for d in (0, 3, 5, 6, 10, 15, 16, 17, 18, 24))
    pos.update(hi - d for d in (1, 2, 3, 4))
    return lo, hi - 1, tuple(sorted(pos))


def grid_cases(chrom, plusp):
    """(prevpos, currpos) uint64 arrays of every pair of the chromosome's grid, and its chroffset / chrhigh."""
    chroffset, chrhigh, pos = grid_pairs(chrom)
    a = np.array(pos, dtype=np.uint64)
    i, j = np.triu_indices(len(a), k=1)
    low, high = a[i], a[j]
    return (low, high, chroffset, chrhigh) if plusp else (high, low, chroffset, chrhigh)


def brute_canonical(g, maxent, prevpos, currpos, plusp, chroffset):
    """The predicate by brute force for one pair: for each shift the two dinucleotides by string compare, the
    probabilities from maxent(model, pos, chroffset).  Returns (answer, set of case classes met)."""
    floor = GREEDY_ADVANCE if plusp else MISS_BEHIND
    if prevpos < floor or currpos < floor:
        return False, {"early"}
    up = MISS_BEHIND if plusp else GREEDY_ADVANCE
    L, H = (prevpos, currpos) if plusp else (currpos, prevpos)
    rl, rh = L + up, H + up
    cls, ans = set(), False

    def di(at):
        return g[at:at + 2] if at >= 0 else b""

    left_gt = left_ct = right_ag = right_ac = False
    for k in range(GREEDY_ADVANCE + MISS_BEHIND + 1):
        dl, dh = di(rl - k), di(rh - k - 2)
        if b"N" in dl or b"N" in dh:
            cls.add("n")
        if rl - k + 1 >= len(g) or rh - k - 1 >= len(g):
            cls.add("past_end")
        left_gt |= dl == b"GT"
        left_ct |= dl == b"CT"
        right_ag |= dh == b"AG"
        right_ac |= dh == b"AC"
        for sense in (True, False):
            if (dl, dh) != ((b"GT", b"AG") if sense else (b"CT", b"AC")):
                continue
            cls.add("pair_at_equal_shift")
            if (rl - k) % 32 == 31 or (rh - k - 2) % 32 == 31:
                cls.add("straddle")
            pl = maxent(0 if sense else 3, rl - k, chroffset)
            ph = maxent(1 if sense else 2, rh - k, chroffset)
            if pl > 0.9 and ph > 0.9:
                ans = True
                cls.add("sense" if sense else "antisense")
                cls.add("shift_%d" % k if k in (0, 22) else "shift_mid")
            else:
                cls.add("weak_pair")
    if not ans and ((left_gt and right_ag) or (left_ct and right_ac)) and "pair_at_equal_shift" not in cls:
        cls.add("unequal_shifts")
    return ans, cls


def grid_maxent():
    """maxent(model, pos, chroffset) over the grid genome: the reference's own where its objects are built,
    else the oracle's restatement.  Returns (function, keep-alive object)."""
    g, _ = grid_genome()
    if ref_available():
        ref = Ref("nosimd")
        ref.set_genome(g)
        return (lambda m, p, c: ref.maxent(m, p, c) if p >= 0 else 0.0), ref
    orc = Oracle()
    orc.set_genome(g)
    return (lambda m, p, c: orc.maxent(m, p, c) if p >= 0 else 0.0), orc


# ---------------------------------------------------------------------------------------------------------
# The chain generator
# ---------------------------------------------------------------------------------------------------------
CHAIN_CHROMS = ((0, 700000), (700013, 1400000))   # [chroffset, end): the second offset is odd


def _np_genome(seed, n):
    r = np.random.RandomState(seed)
    return bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[r.randint(0, 4, n)].tobytes())


def _plant_intron(g, rng, t, s, minus_gene, shift=0):
    """Strong canonical sites for the intron [t, s) (genome coordinates), moved `shift` into the intron at the
    donor side and out of it at the acceptor side (the same shift on both sides)."""
    if not minus_gene:
        _put(g, t + shift - 3, DONOR)
        _put(g, s + shift - 20, ACCEPTOR)
    else:
        _put(g, t + shift - 3, ANTIACCEPTOR)
        _put(g, s + shift - 6, ANTIDONOR)


@functools.lru_cache(maxsize=None)
def chain_calls(kind="spliced", n=200, seed=77):
    """(genome, calls).  kind:
    spliced  300-600-nt reads of 3-4 exons on 20-kb windows: half the introns carry planted canonical sites, a
             quarter of those displaced against the seed ends (up to and one past the window edges); 45 % of
             the reads have a 10-13-nt second exon that the default chain includes and the flagged chain
             skips (one canonical link against two penalised ones); splicingp 0 on 15 %
    short    three exons of 40-70 nt each: few positions, one hit each (the one-hit forms)
    repeat   the first exon ends in a tandem repeat that the first intron holds 66-88 more copies of: many
             active hits per position (_mult, the 64-lane chunks, the multi-hit windows)"""
    rng = random.Random(seed + {"spliced": 0, "short": 1, "repeat": 2}[kind])
    g = _np_genome(seed, CHAIN_CHROMS[-1][1])
    plans = []
    for ci in range(n):
        chroffset, chrend_u = CHAIN_CHROMS[rng.randrange(2)]
        chrlen = chrend_u - chroffset
        nex = rng.randint(3, 4)
        if kind == "short":
            nex = 3
            exlen = [rng.randint(40, 70) for _ in range(nex)]
        else:
            total = rng.randint(300, 600)
            cuts = sorted(rng.sample(range(40, total - 40, 20), nex - 1))
            exlen = [b - a for a, b in zip([0] + cuts, cuts + [total])]
        micro = kind != "repeat" and rng.random() < 0.45
        if micro:
            m = rng.randint(10, 13)
            exlen[0] += exlen[1] - m
            exlen[1] = m
        introns = [rng.randint(200, 4500) for _ in range(nex - 1)]
        if kind == "repeat":
            introns[0] = rng.randint(1800, 4500)
        ws = rng.randint(1000, chrlen - 21000)                      # the 20-kb window (chromosome coordinates)
        s0 = ws + rng.randint(2500, 4000)
        exons, pos = [], s0
        for e in range(nex):
            exons.append((pos, pos + exlen[e]))
            if e < nex - 1:
                pos += exlen[e] + introns[e]
        plans.append(dict(chroffset=chroffset, chrhigh=chrend_u, ws=ws, exons=exons, plusp=rng.random() < 0.5,
                          minus_gene=rng.random() < 0.5, micro=micro,
                          splicingp=0 if ci % 20 in (3, 9, 15) else 1))   # 15 % of the calls
    # pass 1: write the windows (duplicated exons, repeats, planted sites)
    for P in plans:
        co, ex = P["chroffset"], P["exons"]
        P["mut"] = []
        for i in range(len(ex) - 1):
            t, s = co + ex[i][1], co + ex[i + 1][0]
            if P["micro"] and i < 2:
                continue
            if rng.random() < 0.5:
                u = rng.random()
                if u < 0.75:
                    _plant_intron(g, rng, t, s, P["minus_gene"])
                elif u < 0.9:   # seeds end m short of the junction: the query's last m exon bases will differ
                    _plant_intron(g, rng, t, s, P["minus_gene"])
                    P["mut"].append((i, rng.choice((4, 9, 15, 16, 17))))
                else:           # the sites sit `d` inside the exons' matching stretch (greedy side)
                    d = rng.choice((3, 6, 7))
                    g[s:s + d] = g[t:t + d]
                    _plant_intron(g, rng, t, s, P["minus_gene"], shift=d)
        if P["micro"]:
            # a 10-13-nt second exon between two introns without sites, strong sites at the first exon's end and
            # the third's start: by default the chain goes through the small exon (its few consecutive points
            # outweigh the second link), with the flag the two penalised links lose to the one canonical link
            # that skips it
            _put(g, co + ex[0][1] - 3, DONOR if not P["minus_gene"] else ANTIACCEPTOR)
            if not P["minus_gene"]:
                _put(g, co + ex[2][0] - 20, ACCEPTOR)
            else:
                _put(g, co + ex[2][0] - 6, ANTIDONOR)
            for at in (co + ex[1][0] - 24, co + ex[1][1]):     # no site by chance around the small exon
                g[at:at + 24] = bytes(rng.choice(b"AT") for _ in range(24))
        if kind == "repeat":
            # the first exon ends in a few copies of a 9-12-nt unit, and the first intron holds 66-88 more: 70-95
            # hits at each of those query positions (below MAX_NACTIVE), inside the active range
            a, b = ex[0]
            u = rng.randint(9, 12)
            unit = bytes(rng.choice(b"ACGT") for _ in range(u))
            L = min(b - a - 20, rng.randint(40, 60))
            g[co + b - L:co + b] = (unit * (L // u + 1))[:L]
            c = rng.randint(66, 88)
            g[co + b + 300:co + b + 300 + c * u] = unit * c
    # pass 2: the reads
    calls = []
    for P in plans:
        co, ex = P["chroffset"], P["exons"]
        parts = [bytearray(g[co + a:co + b]) for a, b in ex]
        for i, m in P["mut"]:
            for k in range(1, min(m, len(parts[i]) - 9) + 1):
                parts[i][-k] = ord(bytes([parts[i][-k]]).translate(bytes.maketrans(b"ACGT", b"CATG")))
        q = bytes(b"".join(parts))
        if not P["plusp"]:
            q = revcomp(q)
        ql = bytearray(q)
        for j in range(0, len(ql), 17):
            ql[j] = ord(chr(ql[j]).lower())
        chrlen = P["chrhigh"] - co
        calls.append(dict(q=bytes(ql), quc=q, chrstart=P["ws"], chrend=min(chrlen - 1, P["ws"] + 20000),
                          chroffset=co, chrhigh=P["chrhigh"], plusp=int(P["plusp"]), splicingp=P["splicingp"],
                          maxintronlen=500000, micro=P["micro"], exons=tuple(ex)))
    return bytes(g), tuple(calls)


@functools.lru_cache(maxsize=None)
def chain_expected(kind="spliced", n=200):
    """(oracle without the flag, oracle with it, range-2 statistics of the flagged runs) for chain_calls."""
    g, calls = chain_calls(kind, n)
    xo = XOracle()
    xo.set_genome(g)
    off = [xo.stage2_compute(p, 0) for p in calls]
    xo.reset_stats()
    on = [xo.stage2_compute(p, CANONICAL_MIDDLE) for p in calls]
    return off, on, xo.stats()
