"""Inputs for the long-query tests (queries with more than 16 384 distinct 8-mers: the seeding's long launch
class, GMAPDP_CTX_LONG_QUERIES).  Deterministic; shared by the oracle tests, the GPU tests and the golden
fixture's generator, so that all three speak about the same calls."""
import random

from dpbind import random_genome

GENOME_NT = 300000
POLYA = (150000, 600)     # a poly-A run: AAAAAAAA counted past Count_T's 255 (poly-T on the minus strand)
POLYT = (152000, 600)     # a poly-T run: TTTTTTTT, the highest oligo of all, so the highest id of its query
TANDEM = (154000, 300)    # 300 copies of ACGTACGT
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
BOUNDARY_N = (16384, 16385, 32768, 32769, 65535, 65536)


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def genome():
    g = bytearray(random_genome(random.Random(20240), GENOME_NT))
    g[POLYA[0]:POLYA[0] + POLYA[1]] = b"A" * POLYA[1]
    g[POLYT[0]:POLYT[0] + POLYT[1]] = b"T" * POLYT[1]
    g[TANDEM[0]:TANDEM[0] + 8 * TANDEM[1]] = b"ACGTACGT" * TANDEM[1]
    return bytes(g)


_DB = []


def de_bruijn():
    """B(4, 8) over ACGT (the Lyndon-word construction), 65 536 characters followed by its first 7 again: every
    8-mer occurs exactly once, so the first n + 7 characters hold exactly n distinct 8-mers."""
    if not _DB:
        k, n = 4, 8
        a, seq = [0] * (k * n), []

        def db(t, p):
            if t > n:
                if n % p == 0:
                    seq.extend(a[1:p + 1])
            else:
                a[t] = a[t - p]
                db(t + 1, p)
                for j in range(a[t - p] + 1, k):
                    a[t] = j
                    db(t + 1, t)
        db(1, 1)
        s = bytes(b"ACGT"[x] for x in seq)
        assert len(s) == 65536
        _DB.append(s + s[:7])
    return _DB[0]


def prefix(n):
    return de_bruijn()[:n + 7]


def distinct_8mers(q):
    return len({q[i:i + 8] for i in range(len(q) - 7) if b"N" not in q[i:i + 8]})


def call(quc, chrstart, chrend, plusp, minor=0):
    return dict(quc=bytes(quc), q=bytes(quc), chrstart=chrstart, chrend=chrend, chroffset=0, chrhigh=GENOME_NT,
                plusp=int(plusp), minor=int(minor), splicingp=1, maxintronlen=500000)


def boundary_calls():
    """Case A: de Bruijn prefixes at the id boundaries against a 5 000-nt window (the old classes' 16-bit counter
    rule) and a 70 000-nt one (32-bit), both strands, major and minor index.  [(n, call)]."""
    out = []
    for n in BOUNDARY_N:
        for w in (5000, 70000):
            for plusp in (1, 0):
                for minor in (0, 1):
                    out.append((n, call(prefix(n), 20000, 20000 + w, plusp, minor)))
    return out


def spliced_read(g, rng, start, plusp, nexons=8, exon=3000, sub=0.02):
    """Case B's read: nexons exons of `exon` nt from the genome, introns of 500-5 000 nt, substitutions; the call's
    window spans the locus with 200 nt either side.  Returns (call, [(query start, genome start) per exon])."""
    parts, exons, pos, qpos = [], [], start, 0
    for e in range(nexons):
        parts.append(g[pos:pos + exon])
        exons.append((qpos, pos))
        qpos += exon
        pos += exon + (rng.randint(500, 5000) if e < nexons - 1 else 0)
    q = bytearray(b"".join(parts))
    for i in range(len(q)):
        if rng.random() < sub:
            q[i] = rng.choice(b"ACGT")
    q = bytes(q) if plusp else revcomp(q)
    return call(q, start - 200, pos + 200, plusp), exons


def spliced_calls(g):
    """Case B: four reads, two per strand, away from the planted runs."""
    rng = random.Random(20241)
    return [spliced_read(g, rng, s, plusp) for s, plusp in ((30000, 1), (90000, 0), (200000, 1), (240000, 0))]


def random_call():
    """Case C: GMAP's allocation bound, 100 000 random nt against a 100 000-nt window."""
    rng = random.Random(20242)
    return call(bytes(rng.choice(b"ACGT") for _ in range(100000)), 160000, 260000, 1)


def wrap_calls(g):
    """Case D: a case-B read over the planted runs with the planted 8-mers spliced in, followed by 60 000 nt of the
    de Bruijn sequence: a case-B read alone has about 20 000 ids, and the wrap has to be seen on an id of the
    last quarter of the id space (TTTTTTTT is the query's highest).  Both strands."""
    rng = random.Random(20243)
    out = []
    for plusp in (1, 0):
        c, _ = spliced_read(g, rng, 120000, plusp)
        assert c["chrstart"] < POLYA[0] and c["chrend"] > TANDEM[0] + 8 * TANDEM[1]
        q = bytearray(c["quc"])
        q[5000:5000] = b"A" * 20 + b"ACGTACGT" * 3 + b"T" * 20
        q += de_bruijn()[:60000]
        out.append(call(q, c["chrstart"], c["chrend"], plusp))
    return out


def wide_call(g):
    """Case F: a long read against a 270 000-nt window (more than 2^18 starts)."""
    c, _ = spliced_read(g, random.Random(20244), 60000, 1)
    return call(c["quc"], 10000, 280000, 1)


def mixed_calls(g):
    """Case E: [100 nt, long, 2 kb, long]."""
    rng = random.Random(20245)
    b = spliced_calls(g)
    short = call(g[40000:40100], 39000, 42000, 1)
    mid = call(revcomp(g[100000:102000]), 95000, 110000, 0)
    del rng
    return [short, b[0][0], mid, b[1][0]]
