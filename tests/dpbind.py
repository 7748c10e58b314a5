"""ctypes bindings used by the tests (test infrastructure).

Three implementations share one calling convention for each Dynprog_* entry
point:

* ``Ref``    -- the reference's own objects (oracle/_ref/librefdp_<v>.so,
                built from /root/reference by oracle/ref.mk);
* ``Oracle`` -- the repo's CPU restatement (oracle/libgmapdp_oracle.so);
* the HIP engine is bound separately through gmapdp (the product package).

Problem generation helpers (seeded, GMAP-shaped sub-problems) live here too.
"""
import ctypes as C
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SO = os.path.join(ROOT, "oracle", "libgmapdp_oracle.so")
REF_SO = {v: os.path.join(ROOT, "oracle", "_ref", "librefdp_%s.so" % v) for v in ("nosimd", "avx2", "nosimda", "avx2a", "gpushim", "gpushim_avx2")}


class Pair(C.Structure):
    _fields_ = [("querypos", C.c_int), ("genomepos", C.c_int), ("queryjump", C.c_int),
                ("genomejump", C.c_int), ("dynprogindex", C.c_int),
                ("cdna", C.c_char), ("comp", C.c_char), ("genome", C.c_char), ("genomealt", C.c_char),
                ("gapp", C.c_int)]

    def key(self):
        return (self.querypos, self.genomepos, self.queryjump, self.genomejump, self.dynprogindex,
                self.cdna, self.comp, self.genome, self.genomealt, self.gapp)


MAXPAIRS = 8192


class _Impl:
    prefix = None

    def __init__(self, path):
        self.lib = C.CDLL(path)
        p = self.prefix
        f = getattr(self.lib, p + "single_gap")
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint,
                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                      C.POINTER(C.c_int), C.POINTER(Pair), C.c_int]
        f.restype = C.c_int
        self._single = f
        f = getattr(self.lib, p + "end_gap")
        f.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint,
                      C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                      C.POINTER(C.c_int), C.POINTER(Pair), C.c_int]
        f.restype = C.c_int
        self._end = f
        self._pairs = (Pair * MAXPAIRS)()
        self._scal = (C.c_int * 6)()
        self._genome_keep = None

    def _before_call(self):
        pass

    def single_gap(self, q, quc, rlength, glength, roffset, goffset, chroffset, chrhigh, watsonp,
                   genestrand, jump_late_p, extraband, widebandp, defect_rate, dynprogindex):
        self._before_call()
        n = self._single(q, quc, rlength, glength, roffset, goffset, chroffset, chrhigh, watsonp,
                         genestrand, jump_late_p, extraband, widebandp, defect_rate, dynprogindex,
                         self._scal, self._pairs, MAXPAIRS)
        assert n <= MAXPAIRS
        pairs = None if n < 0 else [self._pairs[i].key() for i in range(n)]
        return tuple(self._scal), pairs

    def end_gap(self, end3p, q, quc, qpos, rlength, glength, roffset, goffset, chroffset, chrhigh, watsonp,
                genestrand, jump_late_p, extraband, defect_rate, endalign, require_pos_score_p, dynprogindex):
        self._before_call()
        n = self._end(end3p, q, quc, qpos, rlength, glength, roffset, goffset, chroffset, chrhigh, watsonp,
                      genestrand, jump_late_p, extraband, defect_rate, endalign, require_pos_score_p,
                      dynprogindex, self._scal, self._pairs, MAXPAIRS)
        assert n <= MAXPAIRS
        pairs = None if n < 0 else [self._pairs[i].key() for i in range(n)]
        return tuple(self._scal), pairs


class Ref(_Impl):
    prefix = "refh_"

    def __init__(self, variant="nosimd"):
        super().__init__(REF_SO[variant])
        self.variant = variant
        self.lib.refh_init(0, 0, 0)
        self.lib.refh_poison_arenas.argtypes = [C.c_int, C.c_int]

    def _before_call(self):
        # SIMD builds read Dynprog_T arena cells the call never writes (dynprog_simd.c, see
        # oracle/gmapdp_oracle.c "SIMD-build fills"): zero the arenas so that every call sees a
        # fresh arena, the semantics the engine and the oracle define.  No-op for nosimd.
        self.lib.refh_poison_arenas(0, 3)

    def set_genome(self, g: bytes):
        self._genome_keep = C.create_string_buffer(g, len(g))
        self.lib.refh_set_genome(self._genome_keep, len(g))


class Oracle(_Impl):
    prefix = "orc_"

    def __init__(self, simd=False):
        super().__init__(ORACLE_SO)
        self.lib.orc_init(0, 0, 0, 0)
        self.simd = 1 if simd else 0

    def _before_call(self):
        self.lib.orc_set_simd(self.simd)  # the oracle library's semantics switch is process-global

    def set_genome(self, g: bytes):
        self._genome_keep = C.create_string_buffer(g, len(g))
        self.lib.orc_set_genome(self._genome_keep, C.c_uint(len(g)))


def ref_available(variant="nosimd"):
    return os.path.exists(REF_SO[variant])


# ---------------------------------------------------------------------------
# Seeded GMAP-shaped problem generators
# ---------------------------------------------------------------------------
COMP = {ord("A"): "T", ord("C"): "G", ord("G"): "C", ord("T"): "A", ord("N"): "N"}


def random_genome(rng: random.Random, n: int, nfrac=0.002) -> bytes:
    s = bytearray(rng.choice(b"ACGT") for _ in range(n))
    for i in range(n):
        if rng.random() < nfrac:
            s[i] = ord("N")
    return bytes(s)


def mutate(rng, seg: bytes, sub=0.03, indel=0.01, maxindel=4, lower=0.05, iupac=0.002):
    out = bytearray()
    i = 0
    while i < len(seg):
        x = rng.random()
        if x < indel / 2:
            i += rng.randint(1, maxindel)  # deletion in query
            continue
        if x < indel:
            out.extend(rng.choice(b"ACGT") for _ in range(rng.randint(1, maxindel)))
        b = seg[i]
        y = rng.random()
        if y < sub:
            b = rng.choice(b"ACGT")
        elif y < sub + iupac:
            b = rng.choice(b"RYWSMKHBVDNX")
        out.append(b)
        i += 1
    q = bytes(out)
    uc = q
    if lower:
        q = bytes((c + 32) if (65 <= c <= 90 and rng.random() < lower) else c for c in q)
    return q, uc


def revcomp(s: bytes) -> bytes:
    return bytes(ord(COMP.get(c, "N")) for c in reversed(s))


def single_gap_problem(rng, genome: bytes, maxlen=400, chrhigh=None):
    """One Dynprog_single_gap-shaped call: query slice ~ genome slice."""
    glen = len(genome)
    chrhigh = glen if chrhigh is None else chrhigh
    watsonp = rng.random() < 0.6
    glength = max(1, int(rng.expovariate(1 / 110.0))) if rng.random() < 0.9 else rng.randint(1, maxlen)
    glength = min(glength, maxlen)
    goffset = rng.randint(-3 if rng.random() < 0.02 else 0, max(0, chrhigh - glength - 1))
    if rng.random() < 0.03:
        goffset = max(0, chrhigh - glength + rng.randint(0, 5))  # run past chromosome end
    if not watsonp:
        # minus strand reads genome[chrhigh-goffset-glength+1 .. chrhigh-goffset]; GMAP never passes
        # goffset outside [1, chrhigh+1] there (the reference would read outside the genome).
        goffset = min(max(goffset, 1), chrhigh + 1)
    # genome characters as the engine will see them
    if watsonp:
        seg = bytes(genome[goffset + i] if 0 <= goffset + i < chrhigh else ord("*") for i in range(glength))
    else:
        seg = bytes(ord(COMP.get(genome[chrhigh - goffset - i], "?")) if 0 <= chrhigh - goffset - i < chrhigh
                    else ord("*") for i in range(glength))
    seg = seg.replace(b"*", b"A")
    mode = rng.random()
    if mode < 0.15:
        q, uc = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, maxlen // 2))), None
        uc = q
    elif mode < 0.25:
        q, uc = mutate(rng, seg, sub=0.0, indel=0.0)  # equal length, maybe simple path
    else:
        q, uc = mutate(rng, seg, sub=rng.choice([0.01, 0.03, 0.08]), indel=rng.choice([0.0, 0.01, 0.03]))
    if len(q) == 0:
        q = uc = b"A"
    rlength = len(q)
    roffset = rng.randint(0, 3000)
    return dict(q=q, quc=uc, rlength=rlength, glength=glength, roffset=roffset, goffset=goffset,
                chroffset=0, chrhigh=chrhigh, watsonp=int(watsonp), genestrand=0,
                jump_late_p=rng.randint(0, 1), extraband=rng.choice([0, 3, 6, 6, 6, 14]),
                widebandp=int(rng.random() < 0.85),
                defect_rate=rng.choice([0.001, 0.005, 0.02, 0.05]),
                dynprogindex=rng.choice([1, 5, -1, -7]))


def edge_single_gap_problem(rng, genome: bytes):
    """Stress shapes: wide bands (several band words per lane), long segments
    (directions spilled out of LDS), genome skips >= 9 (gap holders), banded
    problems whose band misses the corner, and chromosome-boundary segments."""
    kind = rng.randrange(6)
    p = single_gap_problem(rng, genome, maxlen=2000)
    g = genome
    if kind == 0:    # wide band: R = 2..8
        p["extraband"] = rng.choice([40, 70, 130, 250])
    elif kind == 1:  # long segments (max_rlength 660 / max_glength 2000)
        glength = rng.randint(700, 2000)
        goffset = rng.randint(1, len(g) - glength - 1)
        seg = g[goffset:goffset + glength] if p["watsonp"] else revcomp(g[len(g) - goffset - glength + 1:len(g) - goffset + 1])
        cut = rng.randint(0, max(0, glength - 660))
        q, uc = mutate(rng, seg[cut:cut + rng.randint(200, 660)], sub=0.03, indel=0.01)
        q, uc = q[:660], uc[:660]
        p.update(q=q, quc=uc, rlength=len(q), glength=glength, goffset=goffset, widebandp=1,
                 extraband=rng.choice([6, 14]))
    elif kind == 2:  # big deletion inside -> genome skip >= 9 (gap holder) or long E chain
        seg_len = rng.randint(60, 400)
        goffset = rng.randint(1, len(g) - seg_len - 1)
        seg = g[goffset:goffset + seg_len] if p["watsonp"] else revcomp(g[len(g) - goffset - seg_len + 1:len(g) - goffset + 1])
        a = rng.randint(5, seg_len // 2)
        d = rng.randint(3, min(60, seg_len - a - 2))
        q = seg[:a] + seg[a + d:]
        p.update(q=q, quc=q, rlength=len(q), glength=seg_len, goffset=goffset, widebandp=1,
                 extraband=rng.choice([3, 6, 14]))
    elif kind == 3:  # big insertion -> long F chain
        seg_len = rng.randint(40, 300)
        goffset = rng.randint(1, len(g) - seg_len - 1)
        seg = g[goffset:goffset + seg_len] if p["watsonp"] else revcomp(g[len(g) - goffset - seg_len + 1:len(g) - goffset + 1])
        a = rng.randint(1, seg_len - 1)
        ins = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 80)))
        q = seg[:a] + ins + seg[a:]
        q = q[:660]
        p.update(q=q, quc=q, rlength=len(q), glength=seg_len, goffset=goffset, widebandp=1,
                 extraband=rng.choice([3, 6, 14]))
    elif kind == 4:  # narrow band that may not reach the corner
        p["widebandp"] = 0
        p["extraband"] = rng.choice([0, 1, 2, 3])
    else:            # chromosome boundary
        glength = rng.randint(5, 200)
        goffset = len(g) - glength + rng.randint(-3, 10)
        if not p["watsonp"]:
            goffset = min(goffset, len(g) + 1)
        p.update(glength=glength, goffset=goffset)
    return p


def genomic_char(genome: bytes, p: int, chrhigh: int, watsonp: bool) -> int:
    """get_genomic_nt with chroffset 0 (dynprog_single.c:116)."""
    if watsonp:
        return genome[p] if 0 <= p < chrhigh else ord("*")
    pos = chrhigh - p
    return ord(COMP.get(genome[pos], "N")) if 0 <= pos < chrhigh else ord("*")


ENDALIGNS = (0, 1, 2, 3)  # QUERYEND_GAP, QUERYEND_INDELS, QUERYEND_NOGAPS, BEST_LOCAL


def end_gap_problem(rng, genome: bytes, edge=False):
    """One Dynprog_end5_gap / Dynprog_end3_gap-shaped call (stage3.c:10244-10600):
    query = the read end beyond the last anchor, genome = queryjump + extramaterial_end."""
    chrhigh = len(genome)
    end3p = rng.random() < 0.5
    watsonp = rng.random() < 0.6
    L = max(1, int(rng.gammavariate(1.6, 110))) if not edge else rng.choice([1, 2, 5, rng.randint(300, 800)])
    glength = L + rng.choice([10, 10, 10, 0, 30, -3]) if rng.random() < 0.9 else rng.randint(1, 2100)
    glength = max(1, glength)
    if end3p:
        goffset = rng.randint(0, chrhigh - 1)
        if not edge:
            goffset = rng.randint(0, max(0, chrhigh - glength - 2))
        if not watsonp:
            goffset = min(max(goffset, 1), chrhigh)
        seg = bytes(genomic_char(genome, goffset + i, chrhigh, watsonp) for i in range(min(L, glength)))
    else:
        goffset = rng.randint(-2 if edge else 0, chrhigh - 1)
        if not edge:
            goffset = rng.randint(min(glength, chrhigh - 1), chrhigh - 1)
        if not watsonp:
            goffset = min(goffset, chrhigh - 1)
        n = min(L, glength)
        seg = bytes(genomic_char(genome, goffset - n + 1 + i, chrhigh, watsonp) for i in range(n))
    seg = seg.replace(b"*", b"A") or b"A"
    kind = rng.random()
    if kind < 0.1:
        q = bytes(rng.choice(b"ACGT") for _ in range(L))
        quc = q
    else:
        q, quc = mutate(rng, seg, sub=rng.choice([0.01, 0.03, 0.1, 0.3]), indel=rng.choice([0.0, 0.01, 0.04]))
        if len(q) < L:  # pad with random sequence (the unaligned part of a real read end)
            pad = bytes(rng.choice(b"ACGT") for _ in range(L - len(q)))
            q, quc = (q + pad, quc + pad) if end3p else (pad + q, pad + quc)
        q, quc = (q[:L], quc[:L]) if end3p else (q[-L:], quc[-L:])
    rlength = len(q)
    if edge and rng.random() < 0.2:
        rlength = 0 if rng.random() < 0.3 else rlength
    return dict(end3p=int(end3p), q=q, quc=quc, rlength=rlength, glength=glength,
                roffset=rng.randint(0, 3000) + (rlength if not end3p else 0), goffset=goffset,
                chroffset=0, chrhigh=chrhigh, watsonp=int(watsonp), genestrand=0,
                jump_late_p=rng.randint(0, 1), extraband=rng.choice([6, 6, 6, 3, 14]),
                defect_rate=rng.choice([0.001, 0.005, 0.02, 0.05]),
                endalign=rng.choice([0, 1, 1, 2, 3]), require_pos_score_p=int(rng.random() < 0.1),
                dynprogindex=rng.choice([1, 5, -1, -7]))


def call_end(impl, p):
    qpos = 0 if p["end3p"] else max(len(p["q"]) - 1, 0)
    return impl.end_gap(p["end3p"], p["q"] or b"A", p["quc"] or b"A", qpos, p["rlength"], p["glength"],
                        p["roffset"], p["goffset"], p["chroffset"], p["chrhigh"], p["watsonp"], p["genestrand"],
                        p["jump_late_p"], p["extraband"], p["defect_rate"], p["endalign"],
                        p["require_pos_score_p"], p["dynprogindex"])


def call_single(impl, p):
    return impl.single_gap(p["q"], p["quc"], p["rlength"], p["glength"], p["roffset"], p["goffset"],
                           p["chroffset"], p["chrhigh"], p["watsonp"], p["genestrand"], p["jump_late_p"],
                           p["extraband"], p["widebandp"], p["defect_rate"], p["dynprogindex"])


# ---------------------------------------------------------------------------
# Dynprog_genome_gap (dynprog_genome.c:3288)
# ---------------------------------------------------------------------------
GG_FLAG_WATSON, GG_FLAG_LATE, GG_FLAG_HALF, GG_FLAG_FINAL = 1, 2, 8, 16
_GG_ARGS = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint,
            C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]


def _gg_args(p):
    return (p["q"], p["quc"], p["rlength"], p["glengthL"], p["glengthR"], p["roffset"], p["goffsetL"],
            p["rev_goffsetR"], p["chroffset"], p["chrhigh"], p["cdna_direction"], p["flags"], p["genestrand"],
            p["extraband"], p["defect_rate"], p["maxpeelback"], p["dynprogindex"])


def _ref_genome_gap(self, p):
    self._before_call()
    f = self.lib.refh_genome_gap
    if not getattr(self, "_gg_ready", False):
        f.argtypes = _GG_ARGS + [C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(Pair), C.c_int]
        f.restype = C.c_int
        self.lib.refh_maxent.argtypes = [C.c_int, C.c_uint, C.c_uint]
        self.lib.refh_maxent.restype = C.c_double
        self._gg_scal = (C.c_int * 10)()
        self._gg_dscal = (C.c_double * 2)()
        self._gg_ready = True
    n = f(*_gg_args(p), self._gg_scal, self._gg_dscal, self._pairs, MAXPAIRS)
    assert n <= MAXPAIRS
    pairs = None if n < 0 else [self._pairs[i].key() for i in range(n)]
    return tuple(self._gg_scal) + tuple(self._gg_dscal), pairs


def _ref_maxent(self, model, pos, chroffset=0):
    f = self.lib.refh_maxent
    if f.restype is not C.c_double:
        f.argtypes = [C.c_int, C.c_uint, C.c_uint]
        f.restype = C.c_double
    return f(model, pos, chroffset)


Ref.genome_gap = _ref_genome_gap
Ref.maxent = _ref_maxent


def _orc_genome_gap(self, p, probsL, probsR):
    self._before_call()
    f = self.lib.orc_genome_gap
    if not getattr(self, "_gg_ready", False):
        f.argtypes = _GG_ARGS + [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                 C.POINTER(C.c_double), C.POINTER(Pair), C.c_int]
        f.restype = C.c_int
        self._gg_scal = (C.c_int * 10)()
        self._gg_dscal = (C.c_double * 2)()
        self._gg_ready = True
    lp = (C.c_double * max(1, len(probsL)))(*probsL)
    rp = (C.c_double * max(1, len(probsR)))(*probsR)
    n = f(*_gg_args(p), lp, rp, self._gg_scal, self._gg_dscal, self._pairs, MAXPAIRS)
    assert n <= MAXPAIRS
    pairs = None if n < 0 else [self._pairs[i].key() for i in range(n)]
    return tuple(self._gg_scal) + tuple(self._gg_dscal), pairs


def _orc_splice_sites(self, p):
    gL, gR = max(0, p["glengthL"]), max(0, p["glengthR"])
    posL, modL = (C.c_uint * max(1, gL))(), (C.c_int * max(1, gL))()
    posR, modR = (C.c_uint * max(1, gR))(), (C.c_int * max(1, gR))()
    self.lib.orc_genome_splice_sites(gL, gR, p["goffsetL"], p["rev_goffsetR"], C.c_uint(p["chroffset"]),
                                     C.c_uint(p["chrhigh"]), p["cdna_direction"], p["flags"] & 1,
                                     posL, modL, posR, modR)
    return ([(posL[i], modL[i]) for i in range(gL)], [(posR[i], modR[i]) for i in range(gR)])


Oracle.genome_gap = _orc_genome_gap
Oracle.splice_sites = _orc_splice_sites

MAXENT_TABLES = os.path.join(ROOT, "gmap-2024_amd", "lib", "maxent_hr_tables.bin")


def _orc_maxent(self, model, pos, chroffset=0):
    """oracle/maxent_oracle.c: Maxent_hr_<model>_prob over the oracle's genome (tools/make_maxent_tables.py's
    tables)."""
    lib = self.lib
    if not getattr(lib, "_me_ready", False):
        lib.orc_maxent_load.argtypes = [C.c_char_p]
        lib.orc_maxent.argtypes = [C.c_int, C.c_ulonglong, C.c_ulonglong]
        lib.orc_maxent.restype = C.c_double
        assert lib.orc_maxent_load(MAXENT_TABLES.encode()) == 0, "maxent tables not generated"
        lib._me_ready = True
    return lib.orc_maxent(model, pos, chroffset)


def oracle_splice_probs(orc, p):
    """splice_probs with the oracle's MaxEnt restatement instead of the reference's functions."""
    if p["rlength"] <= 1 or p["rlength"] > 660 or p["glengthL"] > 2000 or p["glengthR"] > 2000:
        return [0.0] * max(0, p["glengthL"]), [0.0] * max(0, p["glengthR"])
    sl, sr = orc.splice_sites(p)
    return ([orc.maxent(m, pos, p["chroffset"]) for pos, m in sl],
            [orc.maxent(m, pos, p["chroffset"]) for pos, m in sr])


Oracle.maxent = _orc_maxent

_COMPL = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A"), ord("N"): ord("N")}

# canonical, GC-AG and AT-AC introns in the cDNA's sense / antisense orientation (intron.h)
_MOTIFS_SENSE = [(b"GT", b"AG")] * 8 + [(b"GC", b"AG"), (b"AT", b"AC")]
_MOTIFS_ANTI = [(b"CT", b"AC")] * 8 + [(b"CT", b"GC"), (b"GT", b"AT")]


def _strand_get(genome, p, chroffset, chrhigh, watsonp):
    """get_genomic_nt (dynprog_single.c:116)"""
    q = chroffset + p if watsonp else chrhigh - p
    if not (chroffset <= q < chrhigh):
        return ord("*")
    return genome[q] if watsonp else _COMPL.get(genome[q], ord("N"))


def _strand_set(genome, p, chroffset, chrhigh, watsonp, ch):
    q = chroffset + p if watsonp else chrhigh - p
    if chroffset <= q < chrhigh:
        genome[q] = ch if watsonp else _COMPL[ch]


def genome_gap_problem(rng, genome: bytearray, edge=False):
    """One Dynprog_genome_gap-shaped call (stage3.c:9504-9539): the query gap
    spans the end of one exon and the start of the next; glengthL = glengthR =
    queryjump + extramaterial_paired (8); rev_goffsetR = genomedp3.  A splice
    motif is usually planted into `genome` (mutated in place) at the true
    junction, sometimes with a decoy a few bases away.  The chromosome sits
    1000 nt inside the genome so that segments running past its ends read '*'
    while the host's MaxEnt lookups (which ignore chrhigh) stay in memory."""
    chroffset, chrhigh = 1000, len(genome) - 1000
    chrlen = chrhigh - chroffset
    watsonp = rng.random() < 0.6
    cdna_direction = rng.choice([1, 1, 1, -1, -1, 0])
    if edge:
        rl0 = rng.choice([0, 1, 2, 3, 5, rng.randint(300, 600), rng.randint(600, 700)])
    else:
        rl0 = max(2, min(600, int(rng.gammavariate(2.2, 50))))
    a = rng.randint(0, rl0)
    b = rl0 - a
    intron = rng.randint(12, 4000) if rng.random() < 0.9 else rng.randint(1, 12)
    span = a + intron + b
    if edge and rng.random() < 0.3:
        goffsetL = rng.choice([rng.randint(0, 30), max(1, chrlen - span - rng.randint(-20, 40))])
    else:
        goffsetL = rng.randint(60, max(61, chrlen - span - 1200))
    rev_goffsetR = goffsetL + span - 1
    motifs = _MOTIFS_SENSE if cdna_direction >= 0 else _MOTIFS_ANTI
    x, y = goffsetL + a, rev_goffsetR - b  # first and last intron base (strand coordinates)
    u = rng.random()
    if u < 0.5:
        # strong consensus sites (MaxEnt probabilities near 1): donor CAG|GTAAGT, acceptor
        # pyrimidine tract + CAG|G; antisense genes see them reverse-complemented
        if cdna_direction >= 0:
            left, lx = b"CAG" + b"GTAAGT", x - 3
            right, ry = b"TTCTTTTCTTTCTTTTCCAG" + b"GTA", y - 19
        else:
            left, lx = b"TAC" + b"CTGGAAAAGAAAGAAAAGAA", x - 3
            right, ry = b"ACTTAC" + b"CTG", y - 5
        for k, ch in enumerate(left):
            _strand_set(genome, lx + k, chroffset, chrhigh, watsonp, ch)
        for k, ch in enumerate(right):
            _strand_set(genome, ry + k, chroffset, chrhigh, watsonp, ch)
    elif u < 0.85:
        lm, rm = rng.choice(motifs)
        for k, ch in enumerate(lm):
            _strand_set(genome, x + k, chroffset, chrhigh, watsonp, ch)
        for k, ch in enumerate(rm):
            _strand_set(genome, y - 1 + k, chroffset, chrhigh, watsonp, ch)
    if u < 0.85:
        if rng.random() < 0.3:  # decoy site nearby
            d = rng.choice([-4, -3, -2, -1, 1, 2, 3, 4])
            lm2, rm2 = rng.choice(motifs)
            side = rng.random() < 0.5
            for k, ch in enumerate(lm2 if side else rm2):
                pos = (goffsetL + a + d + k) if side else (rev_goffsetR - b - 1 + d + k)
                _strand_set(genome, pos, chroffset, chrhigh, watsonp, ch)
    left = bytes(_strand_get(genome, goffsetL + i, chroffset, chrhigh, watsonp) for i in range(a))
    right = bytes(_strand_get(genome, rev_goffsetR - b + 1 + i, chroffset, chrhigh, watsonp) for i in range(b))
    seg = (left + right).replace(b"*", b"A")
    if rng.random() < 0.08:
        q = quc = bytes(rng.choice(b"ACGT") for _ in range(len(seg)))
    else:
        q, quc = mutate(rng, seg, sub=rng.choice([0.0, 0.01, 0.03, 0.08]), indel=rng.choice([0.0, 0.0, 0.01, 0.03]))
    if edge and rl0 <= 5:
        q, quc = q[:rl0], quc[:rl0]
    rlength = len(q)
    extra = 8 if (not edge or rng.random() < 0.5) else rng.choice([1, 2, 20, 60])
    glengthL = rlength + extra
    glengthR = rlength + (extra if rng.random() < 0.9 else rng.choice([1, 3, 15]))
    if edge and rng.random() < 0.1:
        glengthL = rng.choice([glengthL, 2001, 2100])
    flags = (GG_FLAG_WATSON if watsonp else 0) | (GG_FLAG_LATE if rng.random() < 0.5 else 0)
    if rng.random() < 0.1:
        flags |= GG_FLAG_HALF
    if rng.random() < 0.3:
        flags |= GG_FLAG_FINAL
    return dict(q=q or b"A", quc=quc or b"A", rlength=rlength, glengthL=glengthL, glengthR=glengthR,
                roffset=rng.randint(0, 3000), goffsetL=goffsetL, rev_goffsetR=rev_goffsetR, chroffset=chroffset,
                chrhigh=chrhigh, cdna_direction=cdna_direction, flags=flags, genestrand=0,
                extraband=rng.choice([14, 14, 14, 15, 18, 3, 6]),
                defect_rate=rng.choice([0.001, 0.005, 0.01, 0.02, 0.05]),
                maxpeelback=rng.choice([60, 60, 20]), dynprogindex=rng.choice([1, 5, -1, -7]))


def splice_probs(ref, orc, p):
    """The host-side MaxEnt probabilities the engine and the oracle take as
    input: the reference's Maxent_hr_*_prob at the restated positions."""
    if p["rlength"] <= 1 or p["rlength"] > 660 or p["glengthL"] > 2000 or p["glengthR"] > 2000:
        return [0.0] * max(0, p["glengthL"]), [0.0] * max(0, p["glengthR"])  # never read (size guard)
    sl, sr = orc.splice_sites(p)
    return ([ref.maxent(m, pos, p["chroffset"]) for pos, m in sl],
            [ref.maxent(m, pos, p["chroffset"]) for pos, m in sr])


# ---------------------------------------------------------------------------
# Dynprog_cdna_gap (dynprog_cdna.c:787)
# ---------------------------------------------------------------------------
_CG_ARGS = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
            C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]


def _cdna_gap(self, p):
    """((dynprogindex, traceback_score, incompletep), pairs-or-None); None for pairs also when the
    oracle reports the call outside its domain (scalars then end with -3)."""
    self._before_call()
    f = getattr(self.lib, self.prefix + "cdna_gap")
    if not getattr(self, "_cg_ready", False):
        f.argtypes = _CG_ARGS + [C.POINTER(C.c_int), C.POINTER(Pair), C.c_int]
        f.restype = C.c_int
        self._cg_scal = (C.c_int * 3)()
        self._cg_ready = True
    n = f(p["q"], p["quc"], p["qposL"], p["qposR"], p["rlengthL"], p["rlengthR"], p["glength"], p["roffsetL"],
          p["rev_roffsetR"], p["goffset"], p["chroffset"], p["chrhigh"], p["watsonp"], p["genestrand"],
          p["jump_late_p"], p["extraband"], p["defect_rate"], p["dynprogindex"], self._cg_scal, self._pairs, MAXPAIRS)
    assert n <= MAXPAIRS
    if n == -3:
        return tuple(self._cg_scal) + (-3,), None
    return tuple(self._cg_scal), (None if n < 0 else [self._pairs[i].key() for i in range(n)])


Ref.cdna_gap = _cdna_gap
Oracle.cdna_gap = _cdna_gap


def cdna_gap_problem(rng, genome: bytes, edge=False):
    """One Dynprog_cdna_gap-shaped call (stage3.c:9270-9285): a cDNA insertion between two anchors.
    The query gap is the genome gap (glength = genomejump) with `ins` extra bases inserted, so
    queryjump > genomejump + MININTRONLEN; both query pieces are queryjump' = glength +
    extramaterial_paired (8) long, the L piece from querydp5 forward, the R piece ending at
    querydp3."""
    # the chromosome sits 1000 nt inside the genome: segments running past its ends read '*'
    # (or, for the Genome_get_segment variant without that bound, genome bytes) but stay in memory
    chroffset, chrhigh = 1000, len(genome) - 1000
    chrlen = chrhigh - chroffset
    watsonp = rng.random() < 0.6
    G = rng.randint(2, 8) if edge and rng.random() < 0.5 else max(2, min(400, int(rng.gammavariate(2.0, 30))))
    if edge and rng.random() < 0.15:
        G = rng.choice([1, 1, 660])  # glength <= 1: NULL; rlength = G + 8 > 660: the size guard
    ins = rng.randint(10, 14) if rng.random() < 0.3 else rng.randint(10, 250)
    goffset = rng.randint(10, chrlen - G - 10)
    if edge and rng.random() < 0.2:
        goffset = rng.choice([0, 1, chrlen - G - rng.randint(-3, 3)])
    seg = bytes(_strand_get(genome, goffset + i, chroffset, chrhigh, watsonp) for i in range(G)).replace(b"*", b"A")
    a = rng.randint(0, G)
    insert = bytes(rng.choice(b"ACGT") for _ in range(ins))
    if rng.random() < 0.15:  # the insertion copies flanking genome (repeats make ties)
        insert = (seg * (ins // max(1, G) + 2))[:ins]
    gap = seg[:a] + insert + seg[a:]
    q, quc = mutate(rng, gap, sub=rng.choice([0.0, 0.01, 0.03, 0.08]), indel=rng.choice([0.0, 0.0, 0.01]))
    block9 = G >= 24 and rng.random() < 0.15
    if block9:
        # a 9 x 9 unaligned block: the bridge leaves queryjump = genomejump = INSERT_PAIRS and the
        # reference pushes the block as SHORTGAP pairs instead of a gap holder (dynprog_cdna.c:1240);
        # both query pieces then reach into the flanks
        a = rng.randint(3, G - 12)
        q = quc = seg[:a] + bytes(rng.choice(b"ACGT") for _ in range(9)) + seg[a + 9:]
    f5 = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(10 if block9 else 0, 20)))
    f3 = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(10 if block9 else 0, 20)))
    Q = len(q)
    rlength = G + 8
    if Q < rlength + 1 and not block9:  # keep queryjump > genomejump + MININTRONLEN after the mutations
        pad = bytes(rng.choice(b"ACGT") for _ in range(rlength + 1 - Q))
        q, quc, Q = q + pad, quc + pad, Q + len(pad)
    qbuf, qucbuf = f5 + q + f3, f5 + quc + f3
    qposL = len(f5)
    qposR = qposL + Q - 1
    roffsetL = rng.randint(0, 3000)
    return dict(q=qbuf, quc=qucbuf, qposL=qposL, qposR=qposR, rlengthL=rlength, rlengthR=rlength, glength=G,
                roffsetL=roffsetL, rev_roffsetR=roffsetL + (qposR - qposL), goffset=goffset, chroffset=chroffset,
                chrhigh=chrhigh, watsonp=int(watsonp), genestrand=0, jump_late_p=rng.randint(0, 1),
                extraband=rng.choice([14, 14, 3, 6]), defect_rate=rng.choice([0.001, 0.005, 0.02, 0.05]),
                dynprogindex=rng.choice([1, 5, -1, -7]))


# ---------------------------------------------------------------------------
# Stage-2 seeding: Oligoindex_hr_tally + Oligoindex_get_mappings (oligoindex_hr.c:33849/34127)
# ---------------------------------------------------------------------------
_OM_ARGS = [C.c_char_p, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int]


def _oligo_mappings(self, p):
    """(scalars (totalpositions, maxnconsecutive, oned_matrix_p, ndiagonals), npositions list,
    positions list, diagonals list of (diagonal, querystart, queryend, nconsecutive)); None for
    everything but the status when the implementation reports the call outside its domain."""
    f = getattr(self.lib, self.prefix + "oligo_mappings")
    if not getattr(self, "_om_ready", False):
        f.argtypes = _OM_ARGS + [C.POINTER(C.c_int), C.POINTER(C.c_uint), C.c_int, C.POINTER(C.c_int),
                                 C.POINTER(C.c_int), C.c_int]
        f.restype = C.c_int
        self._om_cap = 1 << 21
        self._om_pos = (C.c_uint * self._om_cap)()
        self._om_dg = (C.c_int * (4 * 65536))()
        self._om_sc = (C.c_int * 4)()
        self._om_ready = True
    n = len(p["quc"])
    npos = (C.c_int * max(n, 1))()
    r = f(p["quc"], n, C.c_uint(p["chrstart"]), C.c_uint(p["chrend"]), C.c_uint(p["chroffset"]),
          C.c_uint(p["chrhigh"]), int(p["plusp"]), int(p.get("minor", 0)), npos, self._om_pos, self._om_cap,
          self._om_sc, self._om_dg, 65536)
    if r < 0:
        return (r,)
    sc = tuple(self._om_sc)
    return sc, list(npos[:n]), list(self._om_pos[:r]), [tuple(self._om_dg[4 * i:4 * i + 4]) for i in range(sc[3])]


Ref.oligo_mappings = _oligo_mappings
Oracle.oligo_mappings = _oligo_mappings


def oligo_problem(rng, genome: bytes, edge=False):
    """One Stage2_compute-shaped seeding call: a 2-kb-style cDNA (exons cut from the genome on one
    strand, substitutions, an occasional N) against the genomic window [chrstart, chrend) that
    spans it, plus/minus strand, with chromosome bounds inside the genome."""
    chroffset = rng.choice([0, 0, 1000])
    chrhigh = len(genome) - rng.choice([0, 0, 1000])
    chrlen = chrhigh - chroffset
    nex = rng.randint(1, 6)
    exlen = [rng.randint(30, 500) for _ in range(nex)]
    introns = [rng.randint(60, 6000) for _ in range(nex - 1)]
    span = sum(exlen) + sum(introns)
    if span + 400 >= chrlen:
        introns = [60] * (nex - 1)
        span = sum(exlen) + sum(introns)
    s = rng.randint(200, max(200, chrlen - span - 200))
    plusp = rng.random() < 0.5
    parts, pos = [], s
    for e in range(nex):
        parts.append(genome[chroffset + pos:chroffset + pos + exlen[e]])
        if e < nex - 1:
            pos += exlen[e] + introns[e]
    q = bytearray(b"".join(parts))
    for i in range(len(q)):
        u = rng.random()
        if u < 0.02:
            q[i] = rng.choice(b"ACGT")
        elif u < 0.0025 + 0.02 and rng.random() < 0.1:
            q[i] = ord("N")
    chrstart = max(0, s - rng.randint(0, 300))
    chrend = min(chrlen - 1, s + span + rng.randint(0, 300))
    if not plusp:
        # the minus-strand query is the reverse complement; the window is the same interval
        comp = bytes.maketrans(b"ACGTN", b"TGCAN")
        q = bytearray(bytes(q).translate(comp)[::-1])
    if edge:
        k = rng.randint(0, 3)
        if k == 0:
            q = q[:rng.randint(9, 20)]
        elif k == 1:
            chrend = chrstart + rng.randint(0, 9)
        elif k == 2:
            q = bytearray(b"A" * rng.randint(9, 400)) + q  # poly-A: counts past 256 in A-rich windows
        else:
            chrstart, chrend = 0, min(chrlen - 1, chrstart + rng.randint(1000, 40000))
    return dict(quc=bytes(q), chrstart=chrstart, chrend=chrend, chroffset=chroffset, chrhigh=chrhigh,
                plusp=int(plusp), minor=int(rng.random() < 0.3))


# ---------------------------------------------------------------------------
# Stage2_compute (stage2.c:6325): seeding + chaining + convert_to_nucleotides + filter_unique
# ---------------------------------------------------------------------------
S2_PAIR_CAP = 1 << 18
S2_PATH_CAP = 1024


def _stage2_compute(self, p):
    """(number of results, [middle pair list of each result]) or ("err", code).  Each pair is a
    Pair.key() tuple; gap holders carry queryjump / genomejump and gapp = 1."""
    f = getattr(self.lib, self.prefix + "stage2_compute")
    if not getattr(self, "_s2_ready", False):
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
                      C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(Pair), C.c_int]
        f.restype = C.c_int
        self._s2_sc = (C.c_int * 8)()
        self._s2_paths = (C.c_int * (2 * S2_PATH_CAP))()
        self._s2_pairs = (Pair * S2_PAIR_CAP)()
        self._s2_ready = True
    r = f(p["q"], p["quc"], len(p["quc"]), C.c_uint(p["chrstart"]), C.c_uint(p["chrend"]), C.c_uint(p["chroffset"]),
          C.c_uint(p["chrhigh"]), int(p["plusp"]), int(p.get("splicingp", 1)), int(p.get("maxintronlen", 500000)),
          self._s2_sc, self._s2_paths, S2_PATH_CAP, self._s2_pairs, S2_PAIR_CAP)
    if r < 0:
        return ("err", r)
    pr, pa = self._s2_pairs, self._s2_paths
    return r, [[pr[pa[2 * i] + j].key() for j in range(pa[2 * i + 1])] for i in range(r)]


Ref.stage2_compute = _stage2_compute
Oracle.stage2_compute = _stage2_compute

S2B_PATHS = 64   # kept paths per call the batch oracle keeps (MAX_NALIGNMENTS is 10; ties may add more)


def oracle_stage2_batch(orc, probs, qbuf, qucbuf, nthreads=None):
    """orc_stage2_batch (the restatement, several threads) over gmapdp.STAGE2_PROBLEM_DTYPE problems on the
    oracle's current genome (coordinates as given).  Returns (scalars (n, 8): {nkept or < 0, npaths,
    ncovered, status, diag_querystart, diag_queryend}, paths (n, S2B_PATHS, 2): {first record relative to
    the call's slot, records}, pairs (PATH_PAIR layout, 20 B), pair_off (n + 1))."""
    import numpy as np
    n = len(probs)
    f = orc.lib.orc_stage2_batch
    f.restype = C.c_int
    ql = probs["querylength"].astype(np.int64)
    pair_off = np.zeros(n + 1, dtype=np.int64)
    pair_off[1:] = np.cumsum(3 * ql + 256)
    col = lambda k, dt: np.ascontiguousarray(probs[k], dtype=dt)  # noqa: E731
    args = [col("qoff", np.int32), col("querylength", np.int32), col("chrstart", np.uint32), col("chrend", np.uint32),
            col("chroffset", np.uint32), col("chrhigh", np.uint32), col("plusp", np.int32), col("splicingp", np.int32),
            col("maxintronlen", np.int32)]
    scal = np.zeros((n, 8), dtype=np.int32)
    paths = np.zeros((n, S2B_PATHS, 2), dtype=np.int32)
    pairs = np.zeros(int(pair_off[-1]) * 20 + 20, dtype=np.uint8)
    nt = nthreads or min(16, os.cpu_count() or 4)
    f(C.c_int(n), C.c_char_p(qbuf), C.c_char_p(qucbuf), *[C.c_void_p(a.ctypes.data) for a in args],
      C.c_void_p(scal.ctypes.data), C.c_void_p(paths.ctypes.data), C.c_int(S2B_PATHS), C.c_void_p(pairs.ctypes.data),
      C.c_void_p(pair_off.ctypes.data), C.c_int(nt))
    return scal, paths, pairs, pair_off


def stage2_mismatches(results, paths, pairs, orc_out, index=None, records_only=False):
    """Calls whose engine outputs (gmapdp_stage2_batch / plan format: results, path records, 20-B pair
    records) differ from oracle_stage2_batch's: nresults, npaths, ncovered, status, the Diag_compute_bounds
    query bounds (status 2) and every kept path's pair records byte for byte.  index[i]: the oracle row of
    engine call i (default i).  records_only: the result records alone (the kept paths' total record count
    in place of their records), for results whose paths are no longer held.  Returns [(engine call, what)]."""
    import numpy as np
    scal, opaths, opairs, pair_off = orc_out
    pb = pairs.view(np.uint8).reshape(-1) if len(pairs) else np.zeros(0, dtype=np.uint8)
    bad = []
    for i in range(len(results)):
        j = i if index is None else index[i]
        r, o = results[i], scal[j]
        if int(o[0]) < 0:
            bad.append((i, "oracle error %d" % o[0]))
            continue
        got = (int(r["nresults"]), int(r["npaths"]), int(r["ncovered"]), int(r["status"]))
        exp = (int(o[0]), int(o[1]), int(o[2]), int(o[3]))
        if got != exp:
            bad.append((i, "scalars %s vs %s" % (got, exp)))
            continue
        if int(r["status"]) == 2 and (int(r["diag_querystart"]), int(r["diag_queryend"])) != (int(o[4]), int(o[5])):
            bad.append((i, "query bounds"))
            continue
        if records_only:
            if int(r["npairs"]) != sum(int(opaths[j, k, 1]) for k in range(int(r["nresults"]))):
                bad.append((i, "npairs"))
            continue
        for k in range(int(r["nresults"])):
            pr = paths[int(r["path_offset"]) + k]
            eo, en = int(pr["pair_offset"]), int(pr["npairs"])
            oo, on = int(pair_off[j]) + int(opaths[j, k, 0]), int(opaths[j, k, 1])
            if en != on or not np.array_equal(pb[20 * eo:20 * (eo + en)], opairs[20 * oo:20 * (oo + on)]):
                bad.append((i, "path %d" % k))
                break
    return bad


def repeat_genome(rng, n, nfrac=0.002):
    """An i.i.d. genome with planted tandem repeats and duplicated segments (many hits per 8-mer,
    several chains per read)."""
    g = bytearray(random_genome(rng, n, nfrac))
    for _ in range(n // 20000):
        unit = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 12)))
        L = rng.randint(200, 3000)
        s = rng.randint(0, n - L - 1)
        g[s:s + L] = (unit * (L // len(unit) + 1))[:L]
    for _ in range(n // 50000):
        L = rng.randint(300, 3000)
        a, b = rng.randint(0, n - L - 1), rng.randint(0, n - L - 1)
        g[b:b + L] = g[a:a + L]
    return bytes(g)


def stage2_problem(rng, genome: bytes, edge=False):
    """One Stage2_compute call as GMAP makes it (gmap.c:1208): the seeding problem of oligo_problem
    with the major oligoindex, a query in mixed case (queryseq) and upper case (queryuc), sometimes a
    segment of another locus spliced into the read, and the splicing switch / maxintronlen GMAP's
    options set (Stage2_setup)."""
    p = oligo_problem(rng, genome, edge=edge)
    p["minor"] = 0
    q = bytearray(p["quc"])
    if rng.random() < 0.3:
        s = rng.randint(0, len(genome) - 600)
        q[len(q) // 2:len(q) // 2] = genome[s:s + rng.randint(50, 500)]
    for j in range(len(q)):
        if rng.random() < 0.05:
            q[j] = ord(chr(q[j]).lower())
    p["q"] = bytes(q)
    p["quc"] = bytes(q).upper()
    p["splicingp"] = 0 if rng.random() < 0.15 else 1
    p["maxintronlen"] = rng.choice([500000, 500000, 500000, 2000, 200])
    return p


# ---------------------------------------------------------------------------
# Dynprog_microexon_int (dynprog_single.c:900)
# ---------------------------------------------------------------------------
_ME_ARGS = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int]
MAXCANDS = 4096


def _me_args(p):
    return (p["q"], p["quc"], p["rlength"], p["goffsetL"], p["rev_goffsetR"], p["cdna_direction"], p["chroffset"],
            p["chrhigh"], p["watsonp"])


def _orc_microexon_candidates(self, p):
    """[(cL, cR, candidate, middlelength, pos2, model2, pos3, model3)] in the reference's loop order, or
    None for cdna_direction 0."""
    f = self.lib.orc_microexon_candidates
    if not getattr(self, "_mc_ready", False):
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int,
                      C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_int), C.c_int]
        f.restype = C.c_int
        self._mc_c = (C.c_int * (4 * MAXCANDS))()
        self._mc_p = (C.c_uint * (2 * MAXCANDS))()
        self._mc_m = (C.c_int * (2 * MAXCANDS))()
        self._mc_ready = True
    n = f(*_me_args(p), self._mc_c, self._mc_p, self._mc_m, MAXCANDS)
    assert n >= -2 and n != -1
    if n == -2:
        return None
    c, ps, ms = self._mc_c, self._mc_p, self._mc_m
    return [(c[4 * k], c[4 * k + 1], c[4 * k + 2], c[4 * k + 3], ps[2 * k], ms[2 * k], ps[2 * k + 1], ms[2 * k + 1])
            for k in range(n)]


def _orc_microexon_int(self, p, cand_probs):
    """((dynprogindex after, microintrontype), (bestprob2, bestprob3), pairs-or-None); cand_probs: the
    flat [prob2, prob3, ...] list of the candidates."""
    self._before_call()
    f = self.lib.orc_microexon_int
    if not getattr(self, "_me_ready", False):
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint,
                      C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double),
                      C.POINTER(Pair), C.c_int]
        f.restype = C.c_int
        self._me_s = (C.c_int * 2)()
        self._me_d = (C.c_double * 2)()
        self._me_ready = True
    cp = (C.c_double * max(1, len(cand_probs)))(*cand_probs)
    n = f(p["q"], p["quc"], p["rlength"], p["roffset"], p["goffsetL"], p["rev_goffsetR"], p["cdna_direction"],
          p["chroffset"], p["chrhigh"], p["watsonp"], p["genestrand"], p["dynprogindex"], cp, self._me_s, self._me_d,
          self._pairs, MAXPAIRS)
    assert -1 <= n <= MAXPAIRS
    return tuple(self._me_s), tuple(self._me_d), (None if n < 0 else [self._pairs[i].key() for i in range(n)])


def _ref_microexon_int(self, p):
    self._before_call()
    f = self.lib.refh_microexon_int
    if not getattr(self, "_me_ready", False):
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint,
                      C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(Pair), C.c_int]
        f.restype = C.c_int
        self._me_s = (C.c_int * 2)()
        self._me_d = (C.c_double * 2)()
        self._me_ready = True
    n = f(p["q"], p["quc"], p["rlength"], p["roffset"], p["goffsetL"], p["rev_goffsetR"], p["cdna_direction"],
          p["chroffset"], p["chrhigh"], p["watsonp"], p["genestrand"], p["dynprogindex"], self._me_s, self._me_d,
          self._pairs, MAXPAIRS)
    assert -1 <= n <= MAXPAIRS
    return tuple(self._me_s), tuple(self._me_d), (None if n < 0 else [self._pairs[i].key() for i in range(n)])


Oracle.microexon_candidates = _orc_microexon_candidates
Oracle.microexon_int = _orc_microexon_int
Ref.microexon_int = _ref_microexon_int


def microexon_probs(ref, cands, chroffset):
    """The host's Maxent_hr_*_prob at the candidates' splice sites (flat prob2, prob3 list)."""
    out = []
    for c in cands or []:
        out.append(ref.maxent(c[5], c[4], chroffset))
        out.append(ref.maxent(c[7], c[6], chroffset))
    return out


def microexon_problem(rng, genome: bytearray, edge=False, at=None):
    """One Dynprog_microexon_int-shaped call (stage3.c:9664): the query gap between two exons' anchors
    (rlength = queryjump), goffsetL = genomedp5 just after the left anchor, rev_goffsetR = genomedp3 just
    before the right one.  Usually a microexon is planted: left piece | intron (5' GT..AG 3' in the
    cDNA's sense) | microexon | intron | right piece, sometimes with decoy copies of the microexon in the
    introns, lower-case or mismatched query characters, or a random query.  Mutates `genome` in place;
    the chromosome sits 1000 nt inside it.  `at`: a list holding the next free chromosome position, so
    that consecutive problems do not overwrite each other's sites (advanced past this problem)."""
    chroffset, chrhigh = 1000, len(genome) - 1000
    watsonp = rng.random() < 0.6
    cdna_direction = rng.choice([1, 1, -1, -1, 0]) if edge else rng.choice([1, -1])
    i1, i2, i3, i4 = (b"G", b"T", b"A", b"G") if cdna_direction >= 0 else (b"C", b"T", b"A", b"C")
    lenL = rng.randint(1, 14)
    lenM = rng.randint(3, 12)
    lenR = rng.randint(1, 14)
    intronA = rng.randint(12, 1200) if not edge else rng.choice([12, 15, 30, rng.randint(12, 20000)])
    intronB = rng.randint(12, 1200) if not edge else rng.choice([12, 15, 30, rng.randint(12, 20000)])
    span = lenL + intronA + lenM + intronB + lenR
    if at is not None:
        goffsetL = at[0] + rng.randint(0, 50)
        at[0] = goffsetL + span
        assert at[0] < chrhigh - chroffset - 50, "genome too small for the problems"
    else:
        goffsetL = rng.randint(50, chrhigh - chroffset - span - 50)
    seq = bytearray(rng.choice(b"ACGT") for _ in range(span))
    micro = bytes(rng.choice(b"ACGT") for _ in range(lenM))
    a = lenL
    seq[a:a + 2] = i1 + i2
    seq[a + intronA - 2:a + intronA] = i3 + i4
    seq[a + intronA:a + intronA + lenM] = micro
    b = a + intronA + lenM
    seq[b:b + 2] = i1 + i2
    seq[b + intronB - 2:b + intronB] = i3 + i4
    if rng.random() < 0.3:  # decoys: flanked copies of the microexon inside the introns
        for _ in range(rng.randint(1, 3)):
            which = rng.random() < 0.5
            lo, hi = (a + 12, a + intronA - lenM - 12) if which else (b + 12, b + intronB - lenM - 12)
            if hi > lo:
                s = rng.randint(lo, hi)
                seq[s - 2:s] = i3 + i4
                seq[s:s + lenM] = micro
                seq[s + lenM:s + lenM + 2] = i1 + i2
    for k in range(span):
        _strand_set(genome, goffsetL + k, chroffset, chrhigh, watsonp, seq[k])
    q = bytearray(seq[:lenL] + micro + seq[span - lenR:])
    kind = rng.random()
    if kind < 0.1:
        q = bytearray(rng.choice(b"ACGT") for _ in range(len(q)))
    elif kind < 0.25:
        j = rng.randrange(len(q))
        q[j] = rng.choice(b"ACGT")
    quc = bytes(q)
    if rng.random() < 0.1:
        j = rng.randrange(len(q))
        q[j] = ord(chr(q[j]).lower())
    q = bytes(q)
    roffset = rng.randint(0, 1500)
    return dict(q=q, quc=quc, rlength=len(q), roffset=roffset, goffsetL=goffsetL,
                rev_goffsetR=goffsetL + span - 1, cdna_direction=cdna_direction, chroffset=chroffset,
                chrhigh=chrhigh, watsonp=int(watsonp), genestrand=0, dynprogindex=rng.choice([1, 5, -1, -7]))


# ---------------------------------------------------------------------------
# Dynprog_end5_splicejunction / Dynprog_end3_splicejunction (dynprog_end.c:1653/2249)
# ---------------------------------------------------------------------------
_SJ_ARGS = [C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
            C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(Pair),
            C.c_int]


def _end_splicejunction(self, p):
    """((dynprogindex, traceback_score, missscore, nmatches, nmismatches, nopens, nindels, known_index),
    pairs-or-None); scalars the reference leaves unwritten are INT_MIN."""
    self._before_call()
    f = getattr(self.lib, self.prefix + "end_splicejunction")
    f.argtypes = _SJ_ARGS
    f.restype = C.c_int
    scal = (C.c_int * 8)()
    q, quc, j = p["q"] or b"A", p["quc"] or b"A", p["j"] or b"A"
    qpos = 0 if p["end3p"] else len(q) - 1
    jpos = 0 if p["end3p"] else len(j) - 1
    n = f(p["end3p"], q, quc, qpos, j, jpos, p["rlength"], p["glength"], p["roffset"], p["goffset_anchor"],
          p["goffset_far"], p["genestrand"], p["jump_late_p"], p["extraband"], p["defect_rate"], p["contlength"],
          p["dynprogindex"], scal, self._pairs, MAXPAIRS)
    assert n <= MAXPAIRS
    return tuple(scal), (None if n < 0 else [self._pairs[i].key() for i in range(n)])


Oracle.end_splicejunction = _end_splicejunction
Ref.end_splicejunction = _end_splicejunction


def splicejunction_problem(rng, genome: bytes, edge=False):
    """One Splicetrie_solve_end5/end3-shaped call (splicetrie.c via Dynprog_end5/3_known,
    dynprog_end.c:2748/3009): the read end beyond the anchor (rlength), a junction string of glength >=
    rlength built as the reference builds it (Dynprog_make_splicejunction_5/3 + make_contjunction_5/3):
    the contlength characters next to the anchor and the far exon's piece, mostly a real splice of the
    read end (mutated), sometimes random.  end5 strings are given in genome order with the anchor side
    LAST (rev_gsequence points at the last character); end3 strings with the anchor side first."""
    end3p = rng.random() < 0.5
    rlength = max(1, int(rng.gammavariate(1.5, 12))) if not edge else rng.choice([1, 2, 3, rng.randint(40, 700)])
    glength = rlength + rng.choice([0, 0, 1, 3, 10, 25]) if rng.random() < 0.9 else rng.randint(1, 2100)
    contlength = rng.randint(0, max(0, min(rlength, glength) - 1))
    if edge and rng.random() < 0.3:
        contlength = rng.choice([0, max(0, rlength - 1), rlength + 2])
    a = rng.randint(0, len(genome) - 2 * glength - 10) if len(genome) > 2 * glength + 10 else 0
    b = rng.randint(0, len(genome) - glength - 1) if len(genome) > glength + 1 else 0
    prox = genome[a:a + contlength]
    dist = genome[b:b + max(0, glength - contlength)]
    j = (dist + prox) if not end3p else (prox + dist)
    j = j[:glength].ljust(glength, b"A")
    mode = rng.random()
    if mode < 0.7:  # the read end follows the junction
        piece = j[-rlength:] if not end3p else j[:rlength]
        q, quc = mutate(rng, piece, sub=rng.choice([0.0, 0.02, 0.06, 0.15]), indel=rng.choice([0.0, 0.0, 0.03]))
        q, quc = (q or b"A"), (quc or b"A")
        if len(q) > rlength:
            q, quc = (q[-rlength:], quc[-rlength:]) if not end3p else (q[:rlength], quc[:rlength])
        while len(q) < rlength:
            ch = bytes([rng.choice(b"ACGT")])
            q, quc = (ch + q, ch + quc) if not end3p else (q + ch, quc + ch)
    else:
        q = bytes(rng.choice(b"ACGTacgtN") for _ in range(rlength))
        quc = q.upper()
    j = bytes(c if c in b"ACGTN" else ord("N") for c in j)
    roffset = rng.randint(0, 3000) if not edge else rng.choice([0, 1, rng.randint(0, 3000)])
    if not end3p:
        roffset = max(roffset, rlength - 1) if rng.random() < 0.9 else roffset
    ga = rng.randint(0, 200000) if not edge else rng.choice([0, 3, rng.randint(0, 200000)])
    gf = rng.randint(0, 200000)
    return dict(end3p=int(end3p), q=q, quc=quc, j=j, rlength=rlength, glength=glength, roffset=roffset,
                goffset_anchor=ga, goffset_far=gf, genestrand=0,
                jump_late_p=rng.randint(0, 1), extraband=rng.choice([3, 6, 10, 10, 10, 14]),
                defect_rate=rng.choice([0.001, 0.005, 0.02, 0.05]), contlength=contlength,
                dynprogindex=rng.choice([1, 5, -1, -7]))


# ---------------------------------------------------------------------------
# Dynprog_end5_known / Dynprog_end3_known (dynprog_end.c:2748/3009), reference harness only
# ---------------------------------------------------------------------------
_KNOWN_ARGS = [C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_char_p, C.c_int,
               C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int,
               C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(Pair),
               C.c_int]
SPLICETYPES = {"donor": 1, "antidonor": 2, "acceptor": 3, "antiacceptor": 4}  # types.h:130


def _end_known(self, p):
    """((dynprogindex, finalscore, ambig_end_length, ambig_splicetype, nmatches, nmismatches, nopens, nindels,
    knownsplicep), pairs-or-None) of one Dynprog_end{5,3}_known call over p["sites"] / p["types"]."""
    self._before_call()
    f = self.lib.refh_end_known
    f.argtypes = _KNOWN_ARGS
    f.restype = C.c_int
    scal = (C.c_int * 9)()
    ns = len(p["sites"])
    sites = (C.c_uint * max(1, ns))(*p["sites"])
    types = (C.c_int * max(1, ns))(*p["types"])
    qpos = 0 if p["end3p"] else len(p["q"]) - 1
    n = f(p["end3p"], sites, types, ns, p["q"], p["quc"], qpos, p["rlength"], p["glength"], p["roffset"],
          p["goffset"], p["querylength"], p["chroffset"], p["chrhigh"], p["limit_low"], p["limit_high"],
          p["cdna_direction"], p["watsonp"], p["genestrand"], p["jump_late_p"], p["extraband"], p["defect_rate"],
          p["dynprogindex"], scal, self._pairs, MAXPAIRS)
    assert n <= MAXPAIRS
    return tuple(scal), (None if n < 0 else [self._pairs[i].key() for i in range(n)])


Ref.end_known = _end_known


def end_known_problem(rng, genome: bytes):
    """One Dynprog_end5/3_known call shaped as stage 3 makes it with -s (glength >= rlength, the read end
    beyond the anchor) over a sorted list of known sites, some inside the end's genomic span with the
    anchor type the call looks for."""
    p = end_gap_problem(rng, genome)
    p["glength"] = max(p["glength"], p["rlength"])  # dynprog_end.c:2773 asserts glength >= rlength
    end3p = p["end3p"]
    gl = len(genome)
    p["querylength"] = p["roffset"] + p["rlength"] + rng.randint(0, 50)
    p["cdna_direction"] = rng.choice([1, -1])
    p["limit_low"], p["limit_high"] = p["chroffset"], p["chrhigh"]
    # the end's genomic span in chromosome coordinates (either strand)
    lo = p["goffset"] - p["rlength"] if not end3p else p["goffset"]
    if not p["watsonp"]:
        lo = p["chrhigh"] - p["chroffset"] - lo - p["rlength"]
    lo += p["chroffset"]
    sites = sorted(set(max(1, rng.randint(lo - 5, lo + p["rlength"] + 5)) for _ in range(rng.randint(0, 6))) |
                   set(rng.randint(1, gl - 1) for _ in range(rng.randint(0, 6))))
    p["sites"] = sites
    p["types"] = [rng.choice([1, 2, 3, 4]) for _ in sites]
    return p


def _orc_genome_gap_known(self, p, probsL, probsR, known):
    """orc_genome_gap with known-site flags (GMAPDP_KNOWN_SITES layout bytes, or None)."""
    self.lib.orc_set_known.argtypes = [C.c_char_p]
    keep = C.create_string_buffer(bytes(known), len(known)) if known is not None else None
    self.lib.orc_set_known(keep)
    try:
        return self.genome_gap(p, probsL, probsR)
    finally:
        self.lib.orc_set_known(None)


Oracle.genome_gap_known = _orc_genome_gap_known


def random_known_flags(rng, p, density=0.03):
    """Known-site flags for a genome-gap call in the engine's layout: sparse random flags for the bridge's
    windows and genome_gap_simple's rlength windows, set where the reference's IIT ranges can set them
    (left [1, glength-2], right [0, glength-3] on the plus strand; mirrored on the minus strand)."""
    gL, gR, r = p["glengthL"], p["glengthR"], p["rlength"]
    watson = p["flags"] & 1

    def side(n, left):
        lo, hi = (1, n - 2) if (left == bool(watson)) else (0, n - 3)
        return bytes(1 if (lo <= i <= hi and rng.random() < density) else 0 for i in range(n))

    out = side(gL, True) + side(gR, False) + side(r + 1, True) + side(r + 1, False)
    return out


# ---------------------------------------------------------------------------
# Whole-batch DP oracle (oracle/dp_batch_oracle.c: orc_dp_batch) and the engine-side canonical form
# ---------------------------------------------------------------------------
DP_KINDS = {"single": 0, "end": 1, "genome": 2, "microexon": 3}


def oracle_dp_batch(orc, fam, probs, qbuf, qucbuf, nthreads=None):
    """orc_dp_batch over engine descriptors (gmapdp.PROBLEM_DTYPE / END_ / GENOME_ / MICROEXON_PROBLEM_DTYPE)
    on the oracle's current genome, MaxEnt from the oracle's restatement (genome gaps, microexons), the
    oracle's current semantics (orc_set_simd).  Returns (scal (n, 16) int32, dscal (n, 2) float64,
    pairs (gmapdp.PAIR_DTYPE), pair_off (n + 1))."""
    import numpy as np
    import gmapdp
    _orc_maxent(orc, 0, 0, 0)  # loads the MaxEnt tables once
    orc._before_call()
    n = len(probs)
    r = probs["rlength"].astype(np.int64)
    if fam in ("single", "end"):
        cap = r + probs["glength"].astype(np.int64) + 16
    elif fam == "genome":
        cap = 2 * r + probs["glengthL"].astype(np.int64) + probs["glengthR"].astype(np.int64) + 16
    else:
        cap = r + 16
    pair_off = np.zeros(n + 1, dtype=np.int64)
    pair_off[1:] = np.cumsum(np.maximum(cap, 16))
    scal = np.zeros((n, 16), dtype=np.int32)
    dscal = np.zeros((n, 2), dtype=np.float64)
    pairs = np.zeros(int(pair_off[-1]) + 1, dtype=gmapdp.PAIR_DTYPE)
    f = orc.lib.orc_dp_batch
    f.restype = C.c_int
    pr = np.ascontiguousarray(probs)
    nt = nthreads or min(16, os.cpu_count() or 4)
    rc = f(C.c_int(DP_KINDS[fam]), C.c_int(n), C.c_void_p(pr.ctypes.data), C.c_char_p(qbuf), C.c_char_p(qucbuf),
           C.c_void_p(scal.ctypes.data), C.c_void_p(dscal.ctypes.data), C.c_void_p(pairs.ctypes.data),
           C.c_void_p(pair_off.ctypes.data), C.c_int(nt))
    assert rc == 0
    return scal, dscal, pairs, pair_off


def _gather(pairs, offs, counts):
    """records [offs[i], offs[i] + counts[i]) of every problem, concatenated in problem order, and each
    record's problem index"""
    import numpy as np
    counts = np.maximum(counts.astype(np.int64), 0)
    tot = int(counts.sum())
    owner = np.repeat(np.arange(len(counts)), counts)
    start = np.repeat(offs.astype(np.int64), counts)
    first = np.repeat(np.cumsum(counts) - counts, counts)
    return pairs[start + (np.arange(tot) - first)], owner


def _canon_pairs(recs, keep_holder_comp):
    """gap holders (querypos = genomepos = -1): only the jump (and, for microexons, comp '<' / '>') is part
    of the reference's Pair_T the callers read; the other characters are zeroed on both sides"""
    import numpy as np
    v = recs.copy()
    hold = (v["querypos"] == -1) & (v["genomepos"] == -1)
    for k in ("cdna", "genome", "genomealt") + (() if keep_holder_comp else ("comp",)):
        v[k][hold] = b"\0"
    return v


def dp_batch_mismatches(fam, res, pairs, orc_out):
    """Problems whose engine outputs (plan / batch results in problem order; `pairs` the engine's pair
    arena) differ from oracle_dp_batch's.  Returns [(problem, what)] (at most 64)."""
    import numpy as np
    scal, dscal, opairs, pair_off = orc_out
    n = len(res)
    bad = {}

    def flag(mask, what):
        for i in np.nonzero(mask)[0][:64]:
            bad.setdefault(int(i), what)

    flag(scal[:, 0] < -1, "oracle error")
    flag(scal[:, 15] != 0, "oracle record the engine format cannot express")
    onp = scal[:, 0].astype(np.int64)
    if fam == "microexon":
        enp = res["npairs"].astype(np.int64)
        flag(enp != onp, "npairs")
        flag(res["dynprogindex"] != scal[:, 1], "dynprogindex")
        flag(res["microintrontype"] != scal[:, 2], "microintrontype")
        flag(res["bestprob2"].view(np.int64) != dscal[:, 0].view(np.int64), "bestprob2")
        flag(res["bestprob3"].view(np.int64) != dscal[:, 1].view(np.int64), "bestprob3")
    else:
        onp = np.maximum(onp, 0)  # the engine's NULL list is npairs 0
        enp = res["npairs"].astype(np.int64)
        flag(enp != onp, "npairs")
        names = ["dynprogindex", "traceback_score", "nmatches", "nmismatches", "nopens", "nindels"]
        if fam == "genome":
            names += ["new_leftgenomepos", "new_rightgenomepos", "exonhead", "introntype"]
        for k, nm in enumerate(names):
            flag(res[nm] != scal[:, 1 + k], nm)
        if fam == "genome":
            live = enp > 0
            flag(res["left_prob"].view(np.int64) != dscal[:, 0].view(np.int64), "left_prob")
            flag(res["right_prob"].view(np.int64) != dscal[:, 1].view(np.int64), "right_prob")
            # the intron gap holder's queryjump (every other holder has none)
            flag(live & (scal[:, 14] > 1), "two holders with a queryjump")
            eq = np.where(res["gap_index"] >= 0, res["gap_queryjump"], 0)
            eg = np.where(eq != 0, res["gap_index"], -1)
            flag(live & ((eg != scal[:, 12]) | (eq != scal[:, 13])), "gap holder queryjump")
    same = enp == onp
    cnt = np.where(same & (onp > 0), onp, 0)
    e, owner = _gather(pairs, res["pair_offset"], cnt)
    o, _ = _gather(opairs, pair_off[:-1], cnt)
    hc = fam == "microexon"
    diff = _canon_pairs(e, hc) != _canon_pairs(o, hc)
    flag(np.bincount(owner[diff], minlength=n) > 0 if diff.any() else np.zeros(n, dtype=bool), "pair records")
    return sorted(bad.items())[:64]
