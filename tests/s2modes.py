"""Inputs and expected values of the stage-2 tests in GMAP's stranded cmet / atoi / ttoc modes (shared by
tests/test_stage2_modes_power.py on the CPU and tests/test_gpu_stage2_modes.py on the GPU).

The statement under test: stage 2 in mode M over the genome G equals STANDARD stage 2 over the reduced
genome G' -- Oligoindex_hr_tally reduces the genome words of a plus- / minus-strand window (ct / ga, tc /
ag, ag / tc for modes 1, 3, 5) and leaves the query alone -- with convert_to_nucleotides' pair characters
rewritten from the real genome (stage2.c:5403-5452).  The oracle restates STANDARD only, so the expected
value of a call is the oracle's on G' of the call's strand, and a mode-blind engine fails wherever the
oracle's results on G and on G' differ (test_stage2_modes_power.py checks that they do).

In read orientation both strands of a mode reduce alike (C->T, T->C, A->G); the reads here carry that
conversion, so a read 8-mer matches the reduced genome exactly when all its convertible bases are converted."""
import numpy as np

MODES = (1, 3, 5)                      # CMET_STRANDED, ATOI_STRANDED, TTOC_STRANDED (mode.h)
NAMES = {1: "cmet", 3: "atoi", 5: "ttoc"}
# forward-strand reduction of a (plus, minus) window, as (from, to) letters
REDUCTION = {1: ((b"C", b"T"), (b"G", b"A")), 3: ((b"T", b"C"), (b"A", b"G")), 5: ((b"A", b"G"), (b"T", b"C"))}
READ_CONVERSION = {1: (b"C", b"T"), 3: (b"T", b"C"), 5: (b"A", b"G")}
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def reduced_genome(g, mode, plusp):
    """G' of a plus- / minus-strand window."""
    a, b = REDUCTION[mode][0 if plusp else 1]
    return bytes(g).translate(bytes.maketrans(a, b))


def _convert(rng, read, mode, frac):
    a, b = READ_CONVERSION[mode]
    r = bytearray(read)
    for i in range(len(r)):
        if r[i] == a[0] and rng.random() < frac:
            r[i] = b[0]
    return r


def _substitute(rng, r, rate):
    for i in np.nonzero(rng.random(len(r)) < rate)[0]:
        r[i] = int(ACGT[rng.integers(0, 4)])
    return bytes(r)


def _no_long_runs(g):
    """Break every homopolymer run of 8 or more."""
    run = 1
    for i in range(1, len(g)):
        run = run + 1 if g[i] == g[i - 1] else 1
        if run == 8:
            g[i] = ord("C") if g[i] != ord("C") else ord("G")
            run = 1


def _two_letter_mix(rng, a, b, n):
    """n letters of {a, b}, no run of 8."""
    s = bytearray((a, b)[int(x)] for x in rng.integers(0, 2, n))
    run = 1
    for i in range(1, n):
        run = run + 1 if s[i] == s[i - 1] else 1
        if run == 7:
            s[i] = a if s[i] == b else b
            run = 1
    return s


# ---- seeding (Oligoindex_hr_tally + Oligoindex_get_mappings) ----
SEED_GENOME = 40000
STRETCH_CT, STRETCH_AG, STRETCH_LEN = 10000, 25000, 400


def seeding_genome():
    """40 kb of ACGT without homopolymer 8-mers, with a 400-nt C/T mix and a 400-nt A/G mix: each becomes a
    homopolymer only under the reduction of one strand of every mode (C/T: cmet plus -> T, atoi plus -> C,
    ttoc minus -> C; A/G: the other strands), so that homopolymer's 8-mer count passes 255 (Count_T wraps) in
    the mode and is 0 in STANDARD."""
    rng = np.random.default_rng(20240222)
    g = bytearray(ACGT[rng.integers(0, 4, SEED_GENOME)].tobytes())
    _no_long_runs(g)
    g[STRETCH_CT:STRETCH_CT + STRETCH_LEN] = _two_letter_mix(rng, ord("C"), ord("T"), STRETCH_LEN)
    g[STRETCH_AG:STRETCH_AG + STRETCH_LEN] = _two_letter_mix(rng, ord("A"), ord("G"), STRETCH_LEN)
    for at in (STRETCH_CT, STRETCH_AG):  # no run across the stretch's borders either
        g[at - 1], g[at + STRETCH_LEN] = ord("G" if at == STRETCH_CT else "C"), ord("G" if at == STRETCH_CT else "C")
    return bytes(g)


def homopolymer_stretch(mode, plusp):
    """(start of the stretch that reduces to a homopolymer for this strand, that homopolymer's letter in
    read orientation)."""
    a, b = REDUCTION[mode][0 if plusp else 1]
    at = STRETCH_CT if a in b"CT" else STRETCH_AG
    return at, (b if plusp else b.translate(COMP))


def seeding_calls(g, mode, n=48):
    """n seeding calls: queries of 40-600 nt drawn from their window (300-8 000 nt, both strands, major and
    minor index) with the mode's read conversion on about half the convertible bases and 2 % substitutions.
    The first eight (four per strand) lie over the strand's homopolymer stretch and carry ten of its letter,
    so one query position's count wraps."""
    rng = np.random.default_rng(7000 + mode)
    calls = []
    for k in range(n):
        plusp = k % 2 == 0
        wlen = int(rng.integers(300, 8001))
        if k < 8:
            at, letter = homopolymer_stretch(mode, plusp)
            wlen = max(wlen, 1200)
            start = at - int(rng.integers(100, wlen - STRETCH_LEN - 100))
        else:
            start = int(rng.integers(0, len(g) - wlen - 1))
        qlen = int(rng.integers(40, min(600, wlen) + 1))
        loc = start + int(rng.integers(0, wlen - qlen + 1))
        read = g[loc:loc + qlen] if plusp else revcomp(g[loc:loc + qlen])
        q = bytearray(_substitute(rng, _convert(rng, read, mode, 0.5), 0.02))
        if k < 8:
            i = int(rng.integers(0, len(q) - 10))
            q[i:i + 10] = letter * 10
        calls.append(dict(quc=bytes(q), chrstart=start, chrend=start + wlen, chroffset=0, chrhigh=len(g) - 1,
                          plusp=int(plusp), minor=int(k % 3 == 0)))
    return calls


def oracle_by_strand(orc, g, mode, calls, f):
    """[f(orc, call)] with the oracle's genome set to G' of the call's strand (mode 0: G itself)."""
    out = [None] * len(calls)
    for plusp in (1, 0):
        orc.set_genome(reduced_genome(g, mode, plusp) if mode else bytes(g))
        for i, c in enumerate(calls):
            if int(c["plusp"]) == plusp:
                out[i] = f(orc, c)
    return out


def seeding_expected(orc, g, mode, calls):
    return oracle_by_strand(orc, g, mode, calls, lambda o, c: o.oligo_mappings(c))


# ---- Stage2_compute ----
S2_GENOME = 100000
# the convertible base (and its complement, for minus-strand reads) at 35 % each: with 90 % of them
# converted about 0.9 * 0.35 = 31 % of a read's bases differ from the genome, so more than a quarter of the
# pair records carry ':' (a uniform genome would give 22 %)
_RICH = {1: b"CG", 3: b"TA", 5: b"AT"}


def stage2_genome(mode):
    rng = np.random.default_rng(9000 + mode)
    p = [0.35 if bytes([c]) in _RICH[mode] else 0.15 for c in b"ACGT"]
    g = bytearray(ACGT[rng.choice(4, S2_GENOME, p=p)].tobytes())
    return bytes(g)


def stage2_calls(g, mode, n=40):
    """n + 2 Stage2_compute calls: upper-case reads of 2 or 3 exons, 300-900 nt, 90 % of the convertible bases
    converted and 1 % substitutions, in windows of 20-60 kb, both strands, splicing on and off, maxintronlen
    2 000 / 500 000."""
    rng = np.random.default_rng(11000 + mode)
    calls = []
    for k in range(n + 2):
        plusp = k % 2 == 0
        # (the last two, one per strand: 70-kb windows, the seeding's 32-bit counter class)
        wlen = int(rng.integers(20000, 60001)) if k < n else 70000
        start = int(rng.integers(0, len(g) - wlen - 1))
        nex = 2 + (k // 2) % 2
        total = int(rng.integers(300, 901))
        cuts = sorted(int(x) for x in rng.integers(60, total - 60, nex - 1))
        exlen = [b - a for a, b in zip([0] + cuts, cuts + [total])]
        exlen = [max(e, 40) for e in exlen]
        introns = [int(rng.integers(100, 3001)) for _ in range(nex - 1)]
        span = sum(exlen) + sum(introns)
        pos = start + int(rng.integers(100, wlen - span - 100))
        parts = []
        for e in range(nex):
            parts.append(g[pos:pos + exlen[e]])
            pos += exlen[e] + (introns[e] if e < nex - 1 else 0)
        read = b"".join(parts)
        if not plusp:
            read = revcomp(read)
        q = _substitute(rng, _convert(rng, read, mode, 0.9), 0.01)
        calls.append(dict(q=q, quc=q, chrstart=start, chrend=start + wlen, chroffset=0, chrhigh=len(g) - 1,
                          plusp=int(plusp), splicingp=int(k % 8 not in (3, 6)), maxintronlen=2000 if k % 5 == 0 else 500000))
    return calls


def stage2_expected(orc, g, mode, probs, qbuf, qucbuf, rewrite=True):
    """oracle_stage2_batch's tuple for `probs` in mode `mode`: each call on G' of its strand and, in a mode,
    every non-gap record rewritten as convert_to_nucleotides does outside STANDARD: genome = genomealt = the
    real genome's character (G at chroffset + pos on the plus strand, the complement of G at chrhigh - pos on
    the minus strand), comp '|' where the upper-case query character equals it, else ':'.  Also returns the
    numbers of non-gap records and of those carrying ':'."""
    import gmapdp
    from dpbind import oracle_stage2_batch
    n = len(probs)
    scal = paths = pairs = pair_off = None
    for plusp in (1, 0):
        orc.set_genome(reduced_genome(g, mode, plusp) if mode else bytes(g))
        s, pa, pr, po = oracle_stage2_batch(orc, probs, qbuf, qucbuf, nthreads=8)
        if scal is None:
            scal, paths, pairs, pair_off = s.copy(), pa.copy(), pr.copy(), po
        sel = np.nonzero(probs["plusp"] == plusp)[0]
        for i in sel:
            scal[i], paths[i] = s[i], pa[i]
            pairs[20 * int(po[i]):20 * int(po[i + 1])] = pr[20 * int(po[i]):20 * int(po[i + 1])]
    nrec = ncolon = 0
    if mode and rewrite:
        gv = np.frombuffer(bytes(g), dtype=np.uint8)
        comp = np.frombuffer(COMP, dtype=np.uint8)
        quc = np.frombuffer(qucbuf, dtype=np.uint8)
        assert gmapdp.PATH_PAIR_DTYPE.itemsize == 20
        rec = pairs[:20 * int(pair_off[-1])].view(gmapdp.PATH_PAIR_DTYPE)
        raw = pairs[:20 * int(pair_off[-1])].reshape(-1, 20)  # bytes 16..19: cdna, comp, genome, genomealt
        for i in range(n):
            if int(scal[i, 0]) <= 0:
                continue
            p = probs[i]
            for k in range(int(scal[i, 0])):
                o = int(pair_off[i]) + int(paths[i, k, 0])
                r = rec[o:o + int(paths[i, k, 1])]
                real = np.nonzero(~((r["querypos"] == -1) & (r["genomepos"] == -1)))[0]
                gp = r["genomepos"][real].astype(np.int64)
                if int(p["plusp"]):
                    c = gv[int(p["chroffset"]) + gp]
                else:
                    c = comp[gv[int(p["chrhigh"]) - gp]]
                qc = quc[int(p["qoff"]) + r["querypos"][real]]
                mark = np.where(qc == c, ord("|"), ord(":")).astype(np.uint8)
                raw[o + real, 17] = mark
                raw[o + real, 18] = c
                raw[o + real, 19] = c
                nrec += len(real)
                ncolon += int(np.count_nonzero(mark == ord(":")))
    return (scal, paths, pairs, pair_off), nrec, ncolon
