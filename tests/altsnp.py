"""The alternate-allele (gmap --use-snps) test helper: the SNP genome pair and the calls that the goldens
(tests/golden/make_alt_golden.py) and the GPU tests share, the golden loader, and the recount of the cases the
committed goldens must contain.

Two sequences of one length: `ref` (the primary genome) and `alt` (the alternate genome's sequence).  What the
reference -- and the engine -- read as the alternate allele at a position (effective_alt) is the alternate
sequence's 2-bit code with 'N' wherever the *reference* sequence is flagged (uncompress_mmap_snps_subst,
genome.c:9419): a non-ACGT character of `alt` loses its flag and reads as its code ('X' -> T, anything else
-> A), and an ACGT character of `alt` under a reference 'N' reads 'N'."""
import importlib.util
import os
import random

import numpy as np

from dpbind import (COMP, edge_single_gap_problem, end_gap_problem, mutate, random_genome, single_gap_problem)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_SINGLE = os.path.join(HERE, "golden", "alt_single_gap_golden.npz")
GOLDEN_END = os.path.join(HERE, "golden", "alt_end_gap_golden.npz")
GENOME_LEN = 20000
DENSE = (5000, 6000)  # a stretch with a SNP every ~4 nt: alignments there change path, not just characters
TAGS = ("ref_alt", "ref_same", "ref_alt_mode1")  # outputs kept per call: both alleles, genomealt == genome, mode 1
ACGT = b"ACGT"


def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def effective_alt(ref: bytes, alt: bytes) -> bytes:
    out = bytearray(len(ref))
    for i, (r, a) in enumerate(zip(ref, alt)):
        if r not in ACGT:
            out[i] = ord("N")
        elif a in ACGT:
            out[i] = a
        else:
            out[i] = ord("T") if a in b"Xx" else ord("A")
    return bytes(out)


def snp_genomes(seed=77, n=GENOME_LEN):
    """(ref, alt): SNPs at ~3 % of the positions, denser in DENSE; forced SNPs at the low / high word and block
    boundaries (offsets 15 / 16, 31 / 32 of a block) every 640 nt, adjacent pairs every 500 nt, at both ends of
    the chromosome; alternate ACGT under half of the reference's N; alternate 'N' over ~0.2 % of the
    reference's ACGT."""
    rng = random.Random(seed)
    ref = bytearray(random_genome(rng, n))
    for p in (0, 1, 2, n - 3, n - 2, n - 1):
        if ref[p] not in ACGT:
            ref[p] = ord("A")
    alt = bytearray(ref)

    def snp(p):
        if ref[p] in ACGT:
            alt[p] = rng.choice([c for c in ACGT if c != ref[p]])

    for p in range(n):
        dense = DENSE[0] <= p < DENSE[1]
        if ref[p] not in ACGT:
            if rng.random() < 0.5:
                alt[p] = rng.choice(ACGT)
        elif rng.random() < (0.25 if dense else 0.03):
            snp(p)
        elif rng.random() < 0.002:
            alt[p] = ord("N")
    for b in range(0, n - 64, 640):
        for o in (15, 16, 31, 32):
            snp(b + o)
    for b in range(100, n - 2, 500):
        snp(b)
        snp(b + 1)
    for p in (0, 1, n - 2, n - 1):
        snp(p)
    return bytes(ref), bytes(alt)


def haplotype(rng, ref: bytes, eff: bytes) -> bytes:
    """The sequence the queries are drawn from: at every SNP, either allele."""
    return bytes(a if (a != r and a != ord("N") and rng.random() < 0.5) else r for r, a in zip(ref, eff))


def _snp_positions(ref, eff):
    return [i for i in range(len(ref)) if ref[i] != eff[i]]


def single_calls(ref: bytes, alt: bytes, seed=78, n_typical=262, n_edge=30):
    rng = random.Random(seed)
    eff = effective_alt(ref, alt)
    hap = haplotype(rng, ref, eff)
    n = len(ref)
    calls = [single_gap_problem(rng, hap) for _ in range(n_typical)]
    calls += [edge_single_gap_problem(rng, hap) for _ in range(n_edge)]
    snps = _snp_positions(ref, eff)
    base = dict(roffset=17, chroffset=0, chrhigh=n, watsonp=1, genestrand=0, jump_late_p=0, extraband=6, widebandp=1,
                defect_rate=0.005, dynprogindex=1)
    # single_gap_simple answers that hold only through the alternate allele: the query is the alternate
    # haplotype of a stretch with at least two SNPs (glength == rlength)
    made = 0
    for s in snps:
        seg = range(s - 5, s + 35)
        if s < 10 or s + 40 > n or sum(1 for i in seg if ref[i] != eff[i]) < 2 or any(ref[i] not in ACGT for i in seg):
            continue
        q = bytes(eff[i] for i in seg)
        calls.append(dict(base, q=q, quc=q, rlength=len(q), glength=len(q), goffset=s - 5, jump_late_p=made & 1))
        made += 1
        if made == 4:
            break
    # SNP columns at c == 1 and c == glength, both strands
    made = 0
    for a, s1 in enumerate(snps):
        s2 = next((s for s in snps[a + 1:] if 30 <= s - s1 <= 200), None)
        if s2 is None or not (DENSE[1] < s1 or s2 < DENSE[0]):
            continue
        glength = s2 - s1 + 1
        for watsonp in (1, 0):
            seg = hap[s1:s2 + 1]
            if not watsonp:
                seg = bytes(ord(COMP.get(c, "N")) for c in reversed(seg))
            q, quc = mutate(rng, seg, sub=0.03, indel=0.01)
            goffset = s1 if watsonp else n - s2
            calls.append(dict(base, q=q, quc=quc, rlength=len(q), glength=glength, goffset=goffset, watsonp=watsonp))
        made += 1
        if made == 3:
            break
    # the dense stretch: both alleles' haplotype as the query, with an indel, so that the larger of the two
    # table entries moves the path
    for k in range(12):
        g0 = rng.randint(DENSE[0], DENSE[1] - 130)
        glength = rng.randint(40, 120)
        seg = hap[g0:g0 + glength]
        cut = rng.randint(5, glength - 8)
        q = seg[:cut] + seg[cut + rng.randint(1, 3):]
        calls.append(dict(base, q=q, quc=q, rlength=len(q), glength=glength, goffset=g0, jump_late_p=k & 1,
                          defect_rate=rng.choice([0.001, 0.005, 0.02])))
    # a segment that runs past chrhigh with SNPs beside the '*' columns, and one that starts before chroffset
    for glength, goffset in ((30, n - 27), (25, -3)):
        lo, hi = max(goffset, 0), min(goffset + glength, n)
        q = hap[lo:hi]
        calls.append(dict(base, q=q, quc=q, rlength=len(q), glength=glength, goffset=goffset, extraband=8))
    return calls


def end_calls(ref: bytes, alt: bytes, seed=79, n_typical=250, n_edge=40):
    rng = random.Random(seed)
    eff = effective_alt(ref, alt)
    hap = haplotype(rng, ref, eff)
    n = len(ref)
    calls = [end_gap_problem(rng, hap) for _ in range(n_typical)]
    calls += [end_gap_problem(rng, hap, edge=True) for _ in range(n_edge)]
    calls = [p for p in calls if not (p["end3p"] and p["goffset"] < 0)]  # (the reference asserts)
    base = dict(chroffset=0, chrhigh=n, genestrand=0, jump_late_p=0, extraband=6, defect_rate=0.005,
                require_pos_score_p=0, dynprogindex=1)
    # every endalign on both strands in the dense stretch, end5 and end3
    for k in range(16):
        end3p, watsonp, endalign = k & 1, (k >> 1) & 1, (k >> 2) & 3
        L = rng.randint(20, 90)
        g0 = rng.randint(DENSE[0] + 100, DENSE[1] - 200)
        if end3p:
            seg = bytes(_genomic(hap, g0 + i, n, watsonp) for i in range(L))
        else:
            seg = bytes(_genomic(hap, g0 - L + 1 + i, n, watsonp) for i in range(L))
        q, quc = mutate(rng, seg, sub=0.02, indel=0.02 if endalign != 2 else 0.0)
        calls.append(dict(base, end3p=end3p, q=q, quc=quc, rlength=len(q), glength=len(q) + 10,
                          roffset=100 + (0 if end3p else len(q)), goffset=g0, watsonp=watsonp, endalign=endalign,
                          jump_late_p=k & 1))
    # end3 past chrhigh and end5 before chroffset, SNPs beside the '*' columns
    q = hap[n - 20:n]
    calls.append(dict(base, end3p=1, q=q, quc=q, rlength=20, glength=30, roffset=50, goffset=n - 20, watsonp=1,
                      endalign=1))
    q = hap[0:20]
    calls.append(dict(base, end3p=0, q=q, quc=q, rlength=20, glength=30, roffset=70, goffset=19, watsonp=1,
                      endalign=1))
    return calls


def _genomic(g: bytes, p: int, chrhigh: int, watsonp) -> int:
    """get_genomic_nt with chroffset 0 over sequence g."""
    if watsonp:
        return g[p] if 0 <= p < chrhigh else ord("*")
    pos = chrhigh - p
    return ord(COMP.get(g[pos], "N")) if 0 <= pos < chrhigh else ord("*")


def columns(ref: bytes, eff: bytes, p, kind):
    """Per DP column c = 1..glength of a call: (gsequence[c], gsequence_alt[c], universal position or -1)."""
    n, w = p["chrhigh"], p["watsonp"]
    sgn = -1 if (kind == "end" and not p["end3p"]) else 1
    out = []
    for c in range(1, p["glength"] + 1):
        gp = p["goffset"] + sgn * (c - 1)
        pos = gp if w else n - gp
        out.append((_genomic(ref, gp, n, w), _genomic(eff, gp, n, w), pos if 0 <= pos < n else -1))
    return out


# the engine's launch rule, restated: band words per lane and whether the direction planes fit in LDS
def bands(p, kind):
    r, g, e = p["rlength"], p["glength"], p["extraband"]
    if kind == "single":
        wide = p["widebandp"]
    else:
        if p["endalign"] == 2:
            return None
        r, g = min(r, 660), min(g, 2000)  # (GMAPDP_MAX_RLENGTH / _GLENGTH)
        wide = p["endalign"] != 1
    if not wide:
        lband = uband = e
    elif g >= r:
        lband, uband = e, g - r + e
    else:
        lband, uband = r - g + e, e
    if kind == "single":
        uband, lband = min(uband, g), min(lband, r)
    return lband, uband


def pick_R(W):
    R = 1
    while R * 64 < W:
        R <<= 1
    return R


def lds_bytes_alt(r, g, R, dirs):
    a16 = lambda x: (x + 15) & ~15  # noqa: E731
    off = a16(8 * (r + 2)) + 2 * a16(r + 1) + 4 * a16(g + 1)
    return off + (a16((g + 1) * 4 * R * 8) if dirs else 0)


def load(path):
    """(ref, alt, calls, {tag: [(scalars, pairs-or-None)]}) of a golden file."""
    g, probs, outs = _make_golden().load(path)
    alt = np.load(path, allow_pickle=False)["genome_alt"].tobytes()
    return g, alt, probs, outs


def count_cases(ref, alt, kind, calls, outs):
    """Recount, from the inputs and the reference's outputs, the cases the golden set must contain."""
    eff = effective_alt(ref, alt)
    n = len(ref)
    k = dict.fromkeys(["snp_c1", "snp_cglen", "snp_band_rows", "snp_adjacent", "off15", "off16", "off31", "off32",
                       "refN_altACGT", "altN_refACGT", "past_chrhigh_snp", "before_chroffset_snp",
                       "end5_plus", "end5_minus", "end3_plus", "end3_minus", "match_alt_only", "mismatch_both",
                       "mode1_amb_alt_only", "simple_alt_only", "path_changed", "nogaps", "indels", "gap", "local",
                       "null", "R1", "R2", "R4", "Wgt256", "dirs_global"], 0)
    for i, p in enumerate(calls):
        if p["rlength"] <= 0 or p["glength"] <= 0:
            k["null"] += outs["ref_alt"][i][1] is None
            continue
        cols = columns(ref, eff, p, kind)
        snp = [a != b for a, b, _ in cols]
        star = [a == ord("*") for a, _, _ in cols]
        k["snp_c1"] += snp[0]
        k["snp_cglen"] += snp[-1]
        k["snp_adjacent"] += any(snp[c] and snp[c + 1] for c in range(len(snp) - 1))
        for a, b, pos in cols:
            if pos < 0:
                continue
            if a != b and pos > 0 and pos % 32 in (15, 16, 31, 0):
                k["off%d" % (pos % 32 or 32)] += 1
            k["refN_altACGT"] += ref[pos] not in ACGT and alt[pos] in ACGT
            k["altN_refACGT"] += alt[pos] not in ACGT and ref[pos] in ACGT
        for c in range(len(cols) - 1):
            if star[c] != star[c + 1] and (snp[c] or snp[c + 1]):
                pos = cols[c][2] if star[c + 1] else cols[c + 1][2]
                k["past_chrhigh_snp" if pos > n // 2 else "before_chroffset_snp"] += 1
        b = bands(p, kind)
        if kind == "end":
            k[("end3_" if p["end3p"] else "end5_") + ("plus" if p["watsonp"] else "minus")] += 1
            k[("gap", "indels", "nogaps", "local")[p["endalign"]]] += 1
        if b is not None:
            lband, uband = b
            r = min(p["rlength"], 660) if kind == "end" else p["rlength"]
            g = min(p["glength"], 2000) if kind == "end" else p["glength"]
            k["snp_band_rows"] += sum(1 for c in range(1, g + 1) if snp[c - 1] and c - uband >= 1 and c + lband <= r)
            W = lband + uband + 1
            R = pick_R(W)
            k["R1"] += R == 1
            k["R2"] += R == 2
            k["R4"] += R >= 4
            k["Wgt256"] += W > 256
            k["dirs_global"] += lds_bytes_alt(r, g, R, True) > 65536
        sa, pa = outs["ref_alt"][i]
        ss, ps = outs["ref_same"][i]
        k["null"] += pa is None
        for rec in pa or []:
            if rec[9]:
                continue
            c1, comp, g1, g2 = rec[5].upper(), rec[6], rec[7], rec[8]
            k["match_alt_only"] += comp == b"*" and c1 != g1 and c1 == g2
            k["mismatch_both"] += comp == b" " and g1 != g2 and g1 != b" "
        for rec in outs["ref_alt_mode1"][i][1] or []:
            # CMET_STRANDED: a query T over a genomic C is consistent (ambiguous), over anything else but T is not
            k["mode1_amb_alt_only"] += (not rec[9] and rec[6] == b":" and rec[5].upper() == b"T" and rec[8] == b"C"
                                        and rec[7] not in (b"C", b"T"))
        if kind == "single" and p["rlength"] == p["glength"] and pa is not None:
            simple = sa[4] == 0 and sa[3] <= 1 and len(pa) == sum(1 for s in star if not s)
            k["simple_alt_only"] += simple and (ps is None or ss[3] > 1 or ss[4] > 0)
        if pa is not None and ps is not None:
            k["path_changed"] += [x[:2] for x in pa] != [x[:2] for x in ps]
    return {a: int(v) for a, v in k.items()}


# what one file must reach by itself (floors): every case of the list that applies to its kind
FLOORS_BOTH = ["snp_c1", "snp_cglen", "snp_band_rows", "snp_adjacent", "off15", "off16", "off31", "off32",
               "refN_altACGT", "altN_refACGT", "past_chrhigh_snp", "before_chroffset_snp", "match_alt_only",
               "mismatch_both", "mode1_amb_alt_only", "path_changed", "R1"]
FLOORS = {"single": FLOORS_BOTH + ["simple_alt_only", "R2", "R4", "Wgt256", "dirs_global"],
          "end": FLOORS_BOTH + ["end5_plus", "end5_minus", "end3_plus", "end3_minus", "nogaps", "indels", "gap", "local",
                                "null"]}


def missing_cases(kind, counts):
    return [c for c in FLOORS[kind] if counts[c] < 1]
