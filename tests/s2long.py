"""Inputs of the long-segment tests of Stage2_compute_one / _ends / _starts (gmapdp_stage2x_batch, kinds 1-3): calls
of 65 543 and 65 544 nt, i.e. 65 536 and 65 537 query positions, the two sides of the path kernel's 16-bit position
fields and of its choice between the LDS link table, the diagonal walk over the global arrays and the walk on lane 0
alone (s2c_kernel).  Built on s2x.genome() and s2x._call, so both chain oracles (tests/s2xoracle, tests/s2soracle)
apply unchanged.  tests/test_stage2x_long_inputs.py shows on the CPU that every call reaches what it is there for.

Everything is seeded; what the lru_cache'd functions return must not be modified."""
import functools
import random

import numpy as np

import s2modes
import s2starts
import s2x

ONE, ENDS, STARTS = s2x.ONE, s2x.ENDS, s2starts.STARTS
KINDS = (ONE, ENDS, STARTS)
LENGTHS = (65543, 65544)              # nq = querylength - 7 = 65 536 (the last that fits 16 bits) and 65 537
PIECE = 100                           # nt taken from a duplicated segment
# hit class: (index into s2x.DUPS, window before the source copy, window after the destination copy)
SMALL, LARGE = "small", "large"       # at most 4 096 seeded hits (kS2cCap), more than 4 096
WINDOWS = {SMALL: (0, 150, 150), LARGE: (2, 3000, 4000)}
IID, PERIODIC = "iid", "periodic"
PERIOD = 12000                        # the periodic fill's unit: about 11 000 distinct 8-mers in the whole query
_OFFSETS = (0, 37, 0, 2999, 512, 0)   # query_offset, cycled over the calls of a kind


@functools.lru_cache(maxsize=None)
def _fill(which):
    """max(LENGTHS) nucleotides: i.i.d. (about 41 000 distinct 8-mers: the long seeding class) or a PERIOD-nt
    i.i.d. unit repeated (the seeding stays in its LDS classes)."""
    rng = random.Random(20250107 + (which == PERIODIC))
    n = max(LENGTHS)
    if which == IID:
        return bytes(rng.choice(b"ACGT") for _ in range(n))
    unit = bytes(rng.choice(b"ACGT") for _ in range(PERIOD))
    return (unit * (n // PERIOD + 1))[:n]


def _long_call(kind, head, ql, fill, co, chrhigh, ws, we, plusp, rng, query_offset):
    """`head` (genome orientation) at the end of a ql-nt query that `kind` chains from on the plus strand -- the 3'
    end for ENDS, the 5' end for ONE and STARTS --, the rest from `fill`.  s2x._call reverse-complements the query of
    a minus call, which puts `head` at the opposite end."""
    rest = _fill(fill)[:ql - len(head)]
    q = rest + head if kind == ENDS else head + rest
    p = s2x._call(kind, q, co, chrhigh, ws, we, plusp, rng, query_offset)
    p["splicingp"], p["maxintronlen"] = 1, 500000
    return p


@functools.lru_cache(maxsize=None)
def boundary_calls(kind):
    """(calls, tags): PIECE nt of a duplicated segment at the query's chaining end, the window over both copies (tied
    best cells: two traced paths, the several-paths walk), over querylength x hit class x strand x fill.
    tags[i] = (querylength, hit class, plusp, fill)."""
    g = s2x.genome()
    rng = random.Random(4100 + kind)
    calls, tags = [], []
    for ql in LENGTHS:
        for hc in (SMALL, LARGE):
            a0, b0, n = s2x.DUPS[WINDOWS[hc][0]]
            co, chrhigh = s2x._chrom_of(a0)
            ws, we = a0 - WINDOWS[hc][1], b0 + n + WINDOWS[hc][2]
            for plusp in (1, 0):
                for fill in (IID, PERIODIC):
                    calls.append(_long_call(kind, g[a0 + 60:a0 + 60 + PIECE], ql, fill, co, chrhigh, ws, we, plusp, rng,
                                            _OFFSETS[len(calls) % len(_OFFSETS)]))
                    tags.append((ql, hc, plusp, fill))
    return tuple(calls), tuple(tags)


@functools.lru_cache(maxsize=None)
def several_lists_calls(kind):
    """ENDS and STARTS calls of 65 544 nt (and one of 65 543) that return two lists after one was eliminated: three
    units of the short tandem repeat s2x.SMALL_REPEATS[1] at the chaining end, the window of s2x.edge_calls (four
    overlapping copies and three more further on).  STARTS on the plus strand; ENDS as its mirror, the same query
    on the minus strand (s2starts.mirrored_ends_call)."""
    assert kind in (ENDS, STARTS)
    g = s2x.genome()
    rng = random.Random(4200 + kind)
    at, unit, c, more = s2x.SMALL_REPEATS[1]
    co, chrhigh = s2x._chrom_of(at)
    calls = []
    for ql, fill, qo in ((65544, IID, 40), (65544, PERIODIC, 0), (65543, IID, 7)):
        calls.append(_long_call(STARTS, g[at:at + 3 * unit], ql, fill, co, chrhigh, at - 300, more + 3 * unit + 300,
                                1 if kind == STARTS else 0, rng, qo))
        calls[-1]["kind"] = kind
    return tuple(calls)


def short_calls(kind, n, seed):
    """n calls of a few hundred nt at the most: s2x.random_calls / s2starts.random_calls."""
    return s2starts.random_calls(n, seed) if kind == STARTS else s2x.random_calls(kind, n, seed)


@functools.lru_cache(maxsize=None)
def mixed_batch(kind):
    """(calls, tags): the i.i.d. boundary calls of one strand per cell and the periodic 65 544 ones, each followed by
    a short call: all three walks of the path kernel in one batch, and large scratch offsets beside small ones.
    tags[i]: the boundary call's tag, None for a short call."""
    calls, tags = boundary_calls(kind)
    pick = []
    for cell, (ql, hc) in enumerate((ql, hc) for ql in LENGTHS for hc in (SMALL, LARGE)):
        pick.append(tags.index((ql, hc, cell % 2, IID)))
    pick += [tags.index((LENGTHS[1], LARGE, plusp, PERIODIC)) for plusp in (1, 0)]
    short = short_calls(kind, len(pick), seed=53)
    out, otags = [], []
    for i, s in zip(pick, short):
        out += [calls[i], s]
        otags += [tags[i], None]
    return tuple(out), tuple(otags)


def oracle_for(kind, orc=None):
    """The chain oracle of `kind` and its batch function with the signature batch(probs, qbuf, qucbuf)."""
    if kind == STARTS:
        o = s2starts.S2SOracle(orc)
        return o, lambda probs, qbuf, qucbuf: o.batch(probs, qbuf, qucbuf, nthreads=4)
    o = s2x.S2XOracle(orc)
    return o, lambda probs, qbuf, qucbuf: o.batch(kind, probs, qbuf, qucbuf, nthreads=4)


def seeded_hits(seed_orc, p):
    """The seeding's totalpositions of a stage-2x call (the minor oligoindex), by dpbind.Oracle."""
    return seed_orc.oligo_mappings(dict(p, minor=1))[0][0]


def walk_of(seeded, ql):
    """The walk s2c_kernel takes, by the host-side rule (s2c_lds_class and the walks' `nq <= 65536`)."""
    nq = ql - 7
    if nq > 65536:
        return "lane0"
    return "lds" if seeded <= 4096 else "diag"


# ---------------------------------------------------------------------------------------------------------
# The stranded-mode expectation
# ---------------------------------------------------------------------------------------------------------
def stranded_expected(set_genome, batch, g, mode, probs, qbuf, qucbuf):
    """What a stranded-mode context returns for a stage-2x batch of upper-case queries: batch(probs, qbuf, qucbuf)
    (an oracle's batch function; set_genome sets that oracle's genome) on the reduced genome of each call's strand,
    the pair characters rewritten from the real genome g as convert_to_nucleotides does outside STANDARD.  Gap
    holders (ONE) keep their characters.  Returns ((scalars, paths, pairs, pair_off), number of ':' pairs, number of
    lists)."""
    import gmapdp
    scal = opaths = opairs = pair_off = None
    for plusp in (1, 0):
        set_genome(s2modes.reduced_genome(g, mode, plusp))
        s, pa, pr, po = batch(probs, qbuf, qucbuf)
        if scal is None:
            scal, opaths, opairs, pair_off = s.copy(), pa.copy(), pr.copy(), po
        for i in np.nonzero(probs["plusp"] == plusp)[0]:
            scal[i], opaths[i] = s[i], pa[i]
            opairs[20 * int(po[i]):20 * int(po[i + 1])] = pr[20 * int(po[i]):20 * int(po[i + 1])]
    gv = np.frombuffer(g, dtype=np.uint8)
    comp = np.frombuffer(s2modes.COMP, dtype=np.uint8)
    quc = np.frombuffer(qucbuf, dtype=np.uint8)
    rec = opairs[:20 * int(pair_off[-1])].view(gmapdp.PATH_PAIR_DTYPE)
    raw = opairs[:20 * int(pair_off[-1])].reshape(-1, 20)
    ncolon = nlists = 0
    for i in range(len(probs)):
        p = probs[i]
        for k in range(max(int(scal[i, 0]), 0)):
            a = int(pair_off[i]) + int(opaths[i, k, 0])
            r = rec[a:a + int(opaths[i, k, 1])]
            real = np.nonzero(~((r["querypos"] == -1) & (r["genomepos"] == -1)))[0]
            gp = r["genomepos"][real].astype(np.int64)
            c = gv[int(p["chroffset"]) + gp] if int(p["plusp"]) else comp[gv[int(p["chrhigh"]) - gp]]
            qc = quc[int(p["qoff"]) + r["querypos"][real] - int(p["query_offset"])]
            mark = np.where(qc == c, ord("|"), ord(":")).astype(np.uint8)
            raw[a + real, 17] = mark
            raw[a + real, 18] = c
            raw[a + real, 19] = c
            ncolon += int(np.count_nonzero(mark == ord(":")))
            nlists += 1
    return (scal, opaths, opairs, pair_off), ncolon, nlists
