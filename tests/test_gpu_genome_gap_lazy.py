"""Dynprog_genome_gap on the engine vs the CPU oracle where the kernel stages lazily and where the Fgap
direction plane is read one band offset up.

A gap flagged for genome_gap_simple (!finalp, defect_rate < DEFECT_MEDQ) stages only what the simple test
reads; the test takes its two probabilities on demand (device MaxEnt, the host arena, or 1.0 at a known
site), and only a gap it declines stages the rest.  The cases below are built so that the simple test
answers, or declines at each of its three exits, at rlength 2, 3, 63, 64, 65 and 129 (more rows than
staging threads), glength = rlength + 8, extraband 14; which exit a gap takes is read from the oracle's
result (see _outcome), and every group asserts that the outcome it is about occurs.

The second half is about plane 3: vertical (query-insertion) chains that run up to row 1 or to the band's
top row, in each placement of the direction planes (global 64-bit ballots, LDS packed words, R = 2 bands
wider than a wave), and the segmented fills of narrow single and end gaps (S = 16 and 32, every segment of
the wave filled, in every single gap an insertion hanging from band offset 0)."""
import random

import pytest

import gmapdp
from dpbind import (GG_FLAG_HALF, Oracle, call_end, call_single, genome_gap_problem, oracle_splice_probs,
                    random_genome)

pytestmark = pytest.mark.gpu

GG_WATSON, GG_LATE = 1, 2  # dpbind's GG_FLAG_WATSON / GG_FLAG_LATE
CHROFF = 1000
RLENGTHS = (2, 3, 63, 64, 65, 129)
ND = {16: (3, 4), 32: (8, 8)}  # (inserted rows, deleted columns) of the segmented single gaps
DONOR, ACCEPTOR = b"CAGGTAAGT", b"TTCTTTTCTTTCTTTTCCAGGTA"  # strong sites (gmapdp/splice_contexts.txt's consensus)


@pytest.fixture(scope="module")
def engine():
    e = gmapdp.Engine(0)
    yield e
    e.close()


def _gap(rng, g, at, rlen, kind, extraband=14, extra=8, late=None):
    """One sense, plus-strand genome gap written into `g` at chromosome position at[0] (advanced past it):
    exons of a and rlen - a bases around a 300-nt intron.
      strong: consensus donor and acceptor at the junction      weak: bare GT..AG in random context
      nosite: the whole locus over {A, C}: no donor dinucleotide anywhere, introntype 0 at every row
      poor:   strong sites, but the query mismatches the exons nearly everywhere (score <= 0)
      ins:    strong sites and a query insertion of 2-4 rows right after the first / before the last base"""
    a = rng.randint(1, rlen - 1)
    b = rlen - a
    intron = 300
    goffsetL = at[0]
    span = a + intron + b
    rev_goffsetR = goffsetL + span - 1
    at[0] += span + 2 * (rlen + extra) + 80
    lo, hi = CHROFF + goffsetL - 40, CHROFF + rev_goffsetR + 40
    if kind == "nosite":
        for i in range(lo - rlen - 40, hi + rlen + 40):
            g[i] = rng.choice(b"AC")
    x, y = CHROFF + goffsetL + a, CHROFF + rev_goffsetR - b  # first and last intron base
    if kind in ("strong", "poor", "ins"):
        g[x - 3:x - 3 + len(DONOR)] = DONOR
        g[y - 19:y - 19 + len(ACCEPTOR)] = ACCEPTOR
    elif kind == "weak":
        g[x:x + 2] = b"GT"
        g[y - 1:y + 1] = b"AG"
    q = bytes(g[x - a:x]) + bytes(g[y + 1:y + 1 + b])
    if kind == "poor":
        q = bytes({65: 67, 67: 65, 71: 84, 84: 71}.get(ch, 65) if rng.random() < 0.8 else ch for ch in q)
    if kind == "ins" and rlen >= 8:
        n = rng.randint(2, 4)
        k = rng.choice([1, 1, rlen - n - 1])
        q = (q[:k] + bytes(rng.choice(b"ACGT") for _ in range(n)) + q[k:])[:rlen]
    flags = GG_WATSON | (GG_LATE if (rng.random() < 0.5 if late is None else late) else 0)
    return dict(q=q, quc=q, rlength=rlen, glengthL=rlen + extra, glengthR=rlen + extra, roffset=rng.randint(0, 3000),
                goffsetL=goffsetL, rev_goffsetR=rev_goffsetR, chroffset=CHROFF, chrhigh=len(g) - CHROFF,
                cdna_direction=1, flags=flags, genestrand=0, extraband=extraband, defect_rate=0.001, maxpeelback=60,
                dynprogindex=rng.choice([1, 5, -1, -7]), a=a)


def _outcome(p, res):
    """Which way the oracle took a gap.  genome_gap_simple's answer is the only result whose exonhead is a
    genome position (= new_rightgenomepos) and whose list has no indel; a declined gap keeps the introntype
    the test looked at (0: no intron-type site with a score >= 0) and, when the fills give nothing, its
    two probabilities (both 0.0: it stopped at finalscore <= 0 before looking at them)."""
    (dpi, score, nm, nmm, nopens, nindels, new_left, new_right, exonhead, introntype, lp, rp), pairs = res
    if pairs is not None and exonhead == new_right and nopens == 0 and new_left - p["goffsetL"] + 1 + (
            p["rev_goffsetR"] - new_right + 1) == p["rlength"]:
        return "answered"
    if introntype == 0:
        return "nosite"
    return "declined"


def _arena(p, v):
    return [v] * p["glengthL"], [v] * p["glengthR"]


def _known(p, simple_sites):
    """Known-site flag bytes (bridge left, bridge right, simple left [0, rlength], simple right): the simple
    test's own flags at the true junction when `simple_sites`, else only a bridge flag elsewhere."""
    gL, gR, r, a = p["glengthL"], p["glengthR"], p["rlength"], p["a"]
    k = bytearray(gL + gR + 2 * (r + 1))
    if simple_sites:
        k[gL + gR + a] = 1
        k[gL + gR + (r + 1) + (r - a)] = 1
    else:
        k[min(gL - 2, a + 2)] = 1
    return bytes(k)


def _first_diff(got, exp):
    for i, (x, y) in enumerate(zip(got, exp)):
        if x != y:
            return i, x, y
    return None


def _check(probs, got, exp, what):
    d = _first_diff(got, exp)
    assert d is None, "%s: problem %d (%s): gpu %s vs oracle %s" % (
        what, d[0], {k: v for k, v in probs[d[0]].items() if k not in ("q", "quc")}, d[1], d[2])


def _flagged_cases(seed):
    """Per rlength: flagged gaps of every kind, an unflagged copy (defect_rate 0.02) for the mixed launch, and
    -- searched with the oracle over mutated copies of a strong gap's query, half of them with the HALF flag
    (finalscore = score - intron score / 2) -- gaps that the simple test declines with a candidate in hand
    although both probabilities are 0.95: its finalscore <= 0 exit."""
    rng = random.Random(seed)
    g = bytearray(random_genome(rng, 400000, nfrac=0.0))
    at = [2000]
    probs = []
    for rlen in RLENGTHS:
        for kind in ("strong", "strong", "weak", "weak", "nosite", "poor", "ins"):
            probs.append((kind, _gap(rng, g, at, rlen, kind)))
        u = _gap(rng, g, at, rlen, "strong")
        u["defect_rate"] = 0.02
        probs.append(("unflagged", u))
    g = bytes(g)
    orc = Oracle()
    orc.set_genome(g)
    swap = {65: 67, 67: 65, 71: 84, 84: 71}
    for rlen in RLENGTHS:
        base = next(p for k, p in probs if k == "strong" and p["rlength"] == rlen)
        found = 0
        for t in range(600):
            pos = set(rng.sample(range(rlen), rng.randint(0, rlen)))
            q = bytes(swap[ch] if i in pos else ch for i, ch in enumerate(base["q"]))
            c = dict(base, q=q, quc=q, flags=base["flags"] | (GG_FLAG_HALF if t & 1 else 0))
            if _outcome(c, orc.genome_gap(c, *_arena(c, 0.95))) == "declined":
                probs.append(("score", c))
                found += 1
                if found == 2:
                    break
    return g, probs


@pytest.fixture(scope="module")
def flagged():
    g, kp = _flagged_cases(9100)
    orc = Oracle()
    orc.set_genome(g)
    return g, kp, orc


def _run_mode(engine, flagged, mode):
    """One launch of all the flagged cases (answered, declined and unflagged gaps mixed) in one probability
    mode; returns per case (kind, problem, oracle result, outcome)."""
    g, kp, orc = flagged
    engine.set_genome(g)
    probs = [p for _, p in kp]
    if mode == "device":
        got = engine.genome_gap_batch(probs, gmapdp.DEVICE)
        exp = [orc.genome_gap(p, *oracle_splice_probs(orc, p)) for p in probs]
    elif mode == "arena":
        # 0.95 everywhere except under the weak gaps (0.5): the test declines those on the probability
        sp = [_arena(p, 0.5 if kind == "weak" else 0.95) for kind, p in kp]
        got = engine.genome_gap_batch(probs, sp)
        exp = [orc.genome_gap(p, lp, rp) for p, (lp, rp) in zip(probs, sp)]
    else:
        # arena 0.5 everywhere: only the simple test's own known flags (forced 1.0) let it answer; the
        # other gaps carry one bridge flag elsewhere and none of the simple test's
        sp = [_arena(p, 0.5) for p in probs]
        known = [_known(p, kind in ("strong", "ins", "unflagged")) for kind, p in kp]
        got = engine.genome_gap_batch_known(probs, sp, known)
        exp = [orc.genome_gap_known(p, lp, rp, k) for p, (lp, rp), k in zip(probs, sp, known)]
    _check(probs, got, exp, mode)
    return [(kind, p, e, _outcome(p, e)) for (kind, p), e in zip(kp, exp)]


@pytest.mark.parametrize("mode", ["device", "arena", "known"])
def test_lazy_staging_every_exit_of_the_simple_test(engine, flagged, mode):
    rows = _run_mode(engine, flagged, mode)
    flagged_rows = [r for r in rows if r[0] != "unflagged"]
    for rlen in RLENGTHS:
        here = [r for r in flagged_rows if r[1]["rlength"] == rlen]
        # the simple test answers (left_prob / right_prob compared bit for bit by _check) ...
        assert any(o == "answered" for k, p, e, o in here if k == "strong"), (mode, rlen, "answered")
        # ... and declines with no intron-type site
        assert any(o == "nosite" for k, p, e, o in here if k == "nosite"), (mode, rlen, "nosite")
    # declines on a probability below 0.90: an exact query over weak sites (score > 0, so not the score exit)
    weak = [r for r in flagged_rows if r[0] == "weak" and r[3] == "declined"]
    assert len({r[1]["rlength"] for r in weak}) >= (3 if mode == "device" else len(RLENGTHS)), (mode, "probability")
    if mode != "device":  # (the arena's value is known: below 0.90 at both sites)
        assert all(r[3] == "declined" for r in flagged_rows if r[0] == "weak")
    # declines on finalscore <= 0: strong sites (probabilities >= 0.90; in the known mode the exit comes before
    # the probabilities; with the device MaxEnt a mutated query may also move the best row to a weaker site), a
    # candidate with score >= 0 was seen (introntype kept) and the gap was not answered
    score = [r for r in flagged_rows if r[0] == "score"]
    assert score and all(r[3] == "declined" for r in score), (mode, "finalscore <= 0")
    print("%s: finalscore <= 0 exits at rlength %s" % (mode, sorted({r[1]["rlength"] for r in score})))
    # declined gaps that the fills then aligned, and declined gaps they gave up (the leaked fields alone)
    declined = [r for r in flagged_rows if r[3] != "answered"]
    assert any(r[2][1] is not None for r in declined) and any(r[2][1] is None for r in declined)
    assert any(r[3] == "answered" for r in rows) and any(r[0] == "unflagged" for r in rows)


def _filled_pool(seed, n, edge_every=4, keep=lambda p: True):
    rng = random.Random(seed)
    g = bytearray(random_genome(rng, 200000))
    probs = []
    for i in range(n):
        p = genome_gap_problem(rng, g, edge=(i % edge_every == 0))
        if i % 2:
            p["defect_rate"] = 0.001
        if keep(p):
            probs.append(p)
    return bytes(g), probs


def test_filled_gaps_at_the_edges_of_the_two_tracebacks(engine):
    """Filled gaps whose R traceback leaves nothing (the gap holder is the list's first record: short queries
    in long segments), with finalscore < 0 (no traceback at all) and with Pair_maxnegscore below -10."""
    orc = Oracle()
    n_r0 = n_neg = n_maxneg = 0
    for seed, n, every, keep in ((9200, 2000, 4, lambda p: True),
                                 (77, 8000, 1, lambda p: 2 <= p["rlength"] <= 5 and p["glengthL"] <= 2000)):
        g, probs = _filled_pool(seed, n, every, keep)
        orc.set_genome(g)
        engine.set_genome(g)
        sp = [_arena(p, 0.95) for p in probs]
        exp = [orc.genome_gap(p, lp, rp) for p, (lp, rp) in zip(probs, sp)]
        got = engine.genome_gap_batch(probs, sp)
        _check(probs, got, exp, "filled")
        n_r0 += sum(1 for s, pairs in exp if pairs and pairs[0][9] == 1)
        n_neg += sum(1 for s, pairs in exp if pairs is None and s[1] == -100 and s[6] < 0)
        n_maxneg += sum(1 for s, pairs in exp if pairs is None and s[1] == -100 and s[6] >= 0)
    print("nR = 0: %d, finalscore < 0: %d, maxnegscore < -10: %d" % (n_r0, n_neg, n_maxneg))
    assert n_r0 and n_neg and n_maxneg
    # Left out: a list of the gap holder alone (npairs 0).  The bridge chooses rows 1 .. rlength - 1 on both
    # sides, so it needs every record of both tracebacks dropped; none of 40 000 oracle calls over these
    # generators produced one.


def _vertical_runs(p, pairs):
    """Query-insertion runs (comp '-', no genome character) of the oracle's list as (rows, first row on the L
    side or None, first row on the R side or None)."""
    runs = []
    cur = []
    for rec in pairs + [None]:
        if rec is not None and rec[6] == b"-" and rec[7] == b" " and rec[9] == 0:
            cur.append(rec[0])
        else:
            if len(cur) >= 2:
                runs.append((min(cur), max(cur)))
            cur = []
    return runs


@pytest.mark.parametrize("cls", ["global", "lds", "r2"])
def test_fgap_chains_to_row_one_and_to_the_band_top(engine, monkeypatch, cls):
    """Query insertions of >= 2 rows that end on the fill's row 1 (the band top clipped at row 1), and ones
    at columns past uband (the chain's cells sit at the low band offsets), in each placement of the planes."""
    monkeypatch.setenv("GMAPDP_GG_LDS_DIRS_MAX", "163840" if cls == "lds" else "0")
    rng = random.Random(9300)
    g = bytearray(random_genome(rng, 400000, nfrac=0.0))
    at = [2000]
    probs = []
    for i in range(240):
        rlen = rng.choice([24, 40, 63, 65, 90, 129])
        # a narrow band brings the band top down to the insertion: extraband 1-3 (W <= 15); R = 2 needs W > 64
        eb = rng.choice([29, 30, 34]) if cls == "r2" else rng.choice([1, 2, 3, 14])
        p = _gap(rng, g, at, rlen, "ins", extraband=eb)
        p["defect_rate"] = rng.choice([0.001, 0.02])
        probs.append(p)
    g = bytes(g)
    orc = Oracle()
    orc.set_genome(g)
    engine.set_genome(g)
    sp = [_arena(p, 0.95) for p in probs]
    exp = [orc.genome_gap(p, lp, rp) for p, (lp, rp) in zip(probs, sp)]
    got = engine.genome_gap_batch(probs, sp)
    _check(probs, got, exp, cls)
    row1 = deep = 0
    for p, (s, pairs) in zip(probs, exp):
        if not pairs:
            continue
        for lo, hi in _vertical_runs(p, pairs):
            # fill row 1 is query position roffset on the L side, roffset + rlength - 1 on the R side
            if lo == p["roffset"] or hi == p["roffset"] + p["rlength"] - 1:
                row1 += 1
            else:
                deep += 1
    print("%s: insertions reaching row 1: %d, others: %d" % (cls, row1, deep))
    assert row1 > 0 and deep > 0
    # (whether a chain's top cell sits on the band's top row past uband cannot be read from the list; the
    # extraband 1-3 gaps put the band top within the insertion's reach, and the segmented test below plants
    # that shape exactly)


@pytest.mark.parametrize("S", [16, 32])
def test_fgap_plane_of_the_segmented_fills(engine, S):
    """Narrow single and end gaps, 64 / S problems per wave with every segment filled, each with a query
    insertion of >= 2 rows: the Fgap bit of a segment's first lane must not come from the neighbouring
    problem's last lane."""
    from dpbind import end_gap_problem
    rng = random.Random(9400 + S)
    g = random_genome(rng, 60000, nfrac=0.0)
    orc = Oracle()
    orc.set_genome(g)
    engine.set_genome(g)
    # Single gaps: a deletion of d genome bases, 14 matching bases, then n inserted query rows.  With
    # extraband = n the wide band is uband = glength - rlength + n = d, so after the deletion the path runs on
    # band offset 0 and the insertion hangs from the band's top row.  W = n + d + 1: 8 (S = 16), 17 (S = 32).
    n, d = ND[S]
    singles, ends = [], []
    for i in range(64):
        G = rng.randint(50, 70)
        goffset = rng.randint(10, len(g) - 200)
        seg = g[goffset:goffset + G]
        a = rng.randint(6, 12)
        b = a + d + 14
        q = seg[:a] + seg[a + d:b] + bytes(rng.choice(b"ACGT") for _ in range(n)) + seg[b:]
        singles.append(dict(q=q, quc=q, rlength=len(q), glength=G, roffset=rng.randint(0, 3000), goffset=goffset,
                            chroffset=0, chrhigh=len(g), watsonp=1, genestrand=0, jump_late_p=i & 1, extraband=n,
                            widebandp=1, defect_rate=rng.choice([0.001, 0.005, 0.02]),
                            dynprogindex=rng.choice([1, 5, -1, -7])))
    while len(ends) < 64:
        p = end_gap_problem(rng, g)
        p["extraband"] = 6 if S == 16 else 14  # W = 13 / 29
        if 8 <= p["rlength"] <= 120 and p["glength"] <= 140:
            ends.append(p)
    exp_s = [call_single(orc, p) for p in singles]
    exp_e = [call_end(orc, p) for p in ends]
    got_s = engine.single_gap_batch(singles)
    got_e = engine.end_gap_batch(ends)
    dd = _first_diff(got_s, exp_s)
    assert dd is None, ("single", dd)
    dd = _first_diff(got_e, exp_e)
    assert dd is None, ("end", dd)
    # the planted shape was taken: a genome skip and a query insertion of n rows in most single gaps
    taken = sum(1 for s, pairs in exp_s if pairs and s[4] == 2 and
                sum(1 for rec in pairs if rec[6] == b"-" and rec[7] == b" ") == n)
    print("S = %d: %d of 64 single gaps took the deletion + %d-row insertion" % (S, taken, n))
    assert taken >= 32
