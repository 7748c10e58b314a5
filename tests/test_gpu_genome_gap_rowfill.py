"""Dynprog_genome_gap on the engine vs the CPU oracle where the row-held fill (fill_stretch, dp_device.h) can go
wrong, once with the default and once with GMAPDP_GG_ROWFILL=0 (every fill in the band-lane layout).

fill_stretch keeps a query row in one lane for T columns and then moves its state down T lanes (the re-base);
T = 16, 8 or 4 is the largest power of two with T + W - 1 <= 64 for a band of W = lband + uband + 1 lanes, and
a band with W >= 62 (or wider than a wave, R = 2) keeps fill_band.  _stretch below restates that rule; the
groups:

  boundaries   rlength around the multiples of T and around W = 37, glength - rlength in {1, 8, 12} on each
               side independently, extraband 14, both jump_late values, and one gap of rlength 600: fills that
               end on, right after and right before a re-base column, and bands clipped by the query's end
  indels       query insertions of 2-4 rows and genome deletions of 2-5 columns planted so that the chain lies
               in, or runs across, the columns T, T + 1, 2T, 2T + 1 of each fill (the oracle's list shows
               where they were taken); insertions that reach row 1 and the band's top row (extraband 1-3)
  widths       bands of 2-6 lanes, 37, and both sides of every change of T: 49 | 50, 57 | 58, 61 | 62 (the
               first band that keeps fill_band), and an R = 2 band; at least 50 fills at each width
  ties         coarse probabilities on 2 000 random gaps, a fifth at chromosome edges: the carried candidate's
               "> score, or = score and > probability, else the earlier column" rule, updated in place
  ends         rows that are still in the band after the last column (retired after the loop) beside gaps in
               which every row has left it (extraband 0), fills of three columns (glength - 2 = 1: one
               candidate column).  glength - 2 < 1 cannot reach the kernel: the engine refuses
               glength <= rlength and answers rlength <= 1 on the host

Every gap here has defect_rate 0.02 unless said otherwise, so genome_gap_simple is not tried and both fills
run."""
import functools
import random

import pytest

import gmapdp
from dpbind import Oracle, genome_gap_problem, random_genome
from test_gpu_genome_gap import _synthetic_probs
from test_gpu_genome_gap_lazy import (ACCEPTOR, CHROFF, DONOR, GG_LATE, GG_WATSON, _arena, _check, _gap,
                                      _vertical_runs)

pytestmark = pytest.mark.gpu

MODES = ("rowfill", "bandfill")


def _stretch(W):
    """Columns per stretch of the row-held fill for a band of W lanes; 0: the band keeps fill_band."""
    for T in (16, 8, 4):
        if T + W - 1 <= 64:
            return T
    return 0


def _widths(p):
    """(WL, WR): lband = extraband, uband = glength - rlength + extraband (Dynprog_compute_bands)."""
    return tuple(2 * p["extraband"] + p[k] - p["rlength"] + 1 for k in ("glengthL", "glengthR"))


@pytest.fixture(scope="module")
def engine():
    e = gmapdp.Engine(0)
    yield e
    e.close()


def _sides(p, eL, eR):
    p["glengthL"] = p["rlength"] + eL
    p["glengthR"] = p["rlength"] + eR
    p["defect_rate"] = 0.02
    return p


def _expected(g, probs, sp):
    orc = Oracle()
    orc.set_genome(g)
    return [orc.genome_gap(p, lp, rp) for p, (lp, rp) in zip(probs, sp)]


def _run(engine, monkeypatch, mode, case):
    g, probs, sp, exp = case
    monkeypatch.setenv("GMAPDP_GG_ROWFILL", "1" if mode == "rowfill" else "0")
    engine.set_genome(g)
    _check(probs, engine.genome_gap_batch(probs, sp), exp, mode)


# ---- stretch boundaries ----
BOUNDARY_RLENGTHS = (2, 3, 15, 16, 17, 31, 32, 33, 36, 37, 38, 63, 64, 65, 129)
EXTRAS = (1, 8, 12)


@functools.lru_cache(maxsize=None)
def boundary_case():
    rng = random.Random(11100)
    g = bytearray(random_genome(rng, 600000, nfrac=0.0))
    at = [2000]
    probs = []
    for rlen in BOUNDARY_RLENGTHS + (600,):
        for eL in EXTRAS:
            for eR in EXTRAS:
                if rlen == 600 and (eL, eR) != (8, 8):
                    continue
                for late in (False, True):
                    kind = rng.choice(["strong", "strong", "weak", "ins"])
                    probs.append(_sides(_gap(rng, g, at, rlen, kind, extra=12, late=late), eL, eR))
    g = bytes(g)
    sp = [_synthetic_probs(rng, p) for p in probs]
    return g, probs, sp, _expected(g, probs, sp)


@pytest.mark.parametrize("mode", MODES)
def test_stretch_boundaries(engine, monkeypatch, mode):
    case = boundary_case()
    g, probs, sp, exp = case
    T = _stretch(37)
    assert T == 16 and all(_stretch(w) == T for p in probs for w in _widths(p))
    glens = {p[k] for p in probs for k in ("glengthL", "glengthR")}
    # fills that end on a re-base column, one column after it and one before it; a fill of one stretch only
    assert {0, 1, T - 1} <= {gl % T for gl in glens} and min(glens) < T
    assert sum(1 for s, pairs in exp if pairs) >= len(probs) // 2  # (most gaps are aligned, not given up)
    _run(engine, monkeypatch, mode, case)


# ---- insertions and deletions across a re-base ----
def _planted(rng, g, at, a, b, side, pos, ins, dele, late):
    """A strong-site gap (exons a and b around a 300-nt intron, extraband 14, glength = rlength + 8) whose query
    carries, `pos` bases from its start (side L) or its end (side R), `ins` inserted bases or a deletion of
    `dele` genome bases: in that side's fill the first pos columns are a diagonal, then the insertion hangs in
    column pos, or the deletion skips the columns pos + 1 .. pos + dele of row pos."""
    goffsetL = at[0]
    span = a + 300 + b
    rev_goffsetR = goffsetL + span - 1
    at[0] += span + 2 * (a + b + 24) + 80
    x, y = CHROFF + goffsetL + a, CHROFF + rev_goffsetR - b
    g[x - 3:x - 3 + len(DONOR)] = DONOR
    g[y - 19:y - 19 + len(ACCEPTOR)] = ACCEPTOR
    e1, e2 = bytes(g[x - a:x]), bytes(g[y + 1:y + 1 + b])
    new = bytes(rng.choice(b"ACGT") for _ in range(ins))
    if side == "L":
        e1 = e1[:pos] + new + e1[pos + dele:]
    else:
        e2 = e2[:b - pos - dele] + new + e2[b - pos:]
    q = e1 + e2
    rlen = len(q)
    return dict(q=q, quc=q, rlength=rlen, glengthL=rlen + 8, glengthR=rlen + 8, roffset=rng.randint(0, 3000),
                goffsetL=goffsetL, rev_goffsetR=rev_goffsetR, chroffset=CHROFF, chrhigh=len(g) - CHROFF,
                cdna_direction=1, flags=GG_WATSON | (GG_LATE if late else 0), genestrand=0, extraband=14,
                defect_rate=0.02, maxpeelback=60, dynprogindex=rng.choice([1, 5, -1, -7]))


def _indel_columns(p, pairs):
    """Per side the fill columns of the oracle's query insertions (the column the rows hang in) and genome
    deletions (the columns skipped): ({"L": set, "R": set} insertions, the same for pairs of neighbouring
    deleted columns (c, c + 1))."""
    ins = {"L": set(), "R": set()}
    dele = {"L": set(), "R": set()}
    mid = (p["goffsetL"] + p["rev_goffsetR"]) // 2
    for rec in pairs:
        if rec[9] or rec[6] != b"-":
            continue
        side = "L" if rec[1] < mid else "R"
        c = rec[1] - p["goffsetL"] + 1 if side == "L" else p["rev_goffsetR"] - rec[1] + 1
        if rec[7] == b" ":
            ins[side].add(c)
        elif rec[5] == b" ":
            dele[side].add(c)
    return ins, {s: {c for c in dele[s] if c + 1 in dele[s]} for s in dele}


@functools.lru_cache(maxsize=None)
def indel_case():
    rng = random.Random(11200)
    g = bytearray(random_genome(rng, 400000, nfrac=0.0))
    at = [2000]
    T = 16
    probs = []
    for side in ("L", "R"):
        for col in (T, T + 1, 2 * T, 2 * T + 1):
            for n in (2, 3, 4):
                for late in (False, True):
                    probs.append(_planted(rng, g, at, rng.randint(45, 70), rng.randint(45, 70), side, col, n, 0, late))
        for col in (T, 2 * T):  # deleted columns start before the re-base column and end after it
            for d in (2, 3, 5):
                for late in (False, True):
                    pos = col - rng.randint(1, d - 1)
                    probs.append(_planted(rng, g, at, rng.randint(45, 70), rng.randint(45, 70), side, pos, 0, d, late))
    # insertions that reach row 1 and, in narrow bands, the band's top row (the lazy-staging test's shapes)
    for i in range(120):
        p = _gap(rng, g, at, rng.choice([24, 40, 63, 65, 90, 129]), "ins", extraband=rng.choice([1, 2, 3, 14]))
        p["defect_rate"] = 0.02
        probs.append(p)
    g = bytes(g)
    sp = [_arena(p, 0.95) for p in probs]
    return g, probs, sp, _expected(g, probs, sp)


@pytest.mark.parametrize("mode", MODES)
def test_indels_across_a_rebase(engine, monkeypatch, mode):
    case = indel_case()
    g, probs, sp, exp = case
    T = 16
    ins = {"L": set(), "R": set()}
    dele = {"L": set(), "R": set()}
    row1 = deep = 0
    for p, (s, pairs) in zip(probs, exp):
        if not pairs:
            continue
        if p["extraband"] == 14 and _widths(p) == (37, 37):
            i, d = _indel_columns(p, pairs)
            for side in ("L", "R"):
                ins[side] |= i[side]
                dele[side] |= d[side]
        for lo, hi in _vertical_runs(p, pairs):
            if lo == p["roffset"] or hi == p["roffset"] + p["rlength"] - 1:
                row1 += 1
            else:
                deep += 1
    for side in ("L", "R"):
        # a vertical chain in the last column of a stretch and in the first column of the next one ...
        assert {T, T + 1, 2 * T, 2 * T + 1} <= ins[side], (side, sorted(ins[side]))
        # ... and a horizontal chain through the columns (T, T + 1) and (2T, 2T + 1)
        assert {T, 2 * T} <= dele[side], (side, sorted(dele[side]))
    assert row1 > 0 and deep > 0
    _run(engine, monkeypatch, mode, case)


# ---- band widths round the rule ----
# (extraband, glength - rlength) per band width W = 2 extraband + (glength - rlength) + 1
WIDTHS = {2: (0, 1), 4: (1, 1), 6: (2, 1), 37: (14, 8), 49: (20, 8), 50: (20, 9), 57: (24, 8), 58: (24, 9),
          61: (26, 8), 62: (26, 9), 69: (30, 8)}
# the two sides' widths of one gap (one extraband: the widths differ by the sides' glength)
WIDTH_PAIRS = ((2, 2), (4, 4), (6, 6), (37, 37), (49, 49), (49, 50), (50, 49), (50, 50), (57, 57), (57, 58),
               (58, 57), (58, 58), (61, 61), (61, 62), (62, 61), (62, 62), (69, 69))


@functools.lru_cache(maxsize=None)
def width_case():
    rng = random.Random(11300)
    g = bytearray(random_genome(rng, 900000, nfrac=0.0))
    at = [2000]
    probs = []
    for wl, wr in WIDTH_PAIRS:
        eb, eL = WIDTHS[wl]
        eR = WIDTHS[wr][1]
        assert WIDTHS[wr][0] == eb
        for i in range(40):
            rlen = rng.choice([20, 33, 47, 64, 80, 100])
            kind = rng.choice(["strong", "strong", "weak", "ins"])
            probs.append(_sides(_gap(rng, g, at, rlen, kind, extraband=eb, extra=12), eL, eR))
    g = bytes(g)
    sp = [_synthetic_probs(rng, p) for p in probs]
    return g, probs, sp, _expected(g, probs, sp)


@pytest.mark.parametrize("mode", MODES)
def test_band_widths_round_the_rule(engine, monkeypatch, mode):
    case = width_case()
    g, probs, sp, exp = case
    fills = {}
    for p in probs:
        for w in _widths(p):
            fills[w] = fills.get(w, 0) + 1
    assert [(w, _stretch(w)) for w in sorted(WIDTHS)] == [(2, 16), (4, 16), (6, 16), (37, 16), (49, 16), (50, 8),
                                                          (57, 8), (58, 4), (61, 4), (62, 0), (69, 0)]
    assert _stretch(48) == 16 and _stretch(63) == 0 and _stretch(64) == 0
    assert all(fills.get(w, 0) >= 50 for w in WIDTHS), fills
    assert sum(1 for s, pairs in exp if pairs) >= len(probs) // 2
    _run(engine, monkeypatch, mode, case)


# ---- ties in the carried candidate ----
@functools.lru_cache(maxsize=None)
def tie_case():
    rng = random.Random(11400)
    g = bytearray(random_genome(rng, 200000))
    probs = [genome_gap_problem(rng, g, edge=(i % 5 == 0)) for i in range(2000)]
    g = bytes(g)
    sp = [_synthetic_probs(rng, p) for p in probs]
    return g, probs, sp, _expected(g, probs, sp)


@pytest.mark.parametrize("mode", MODES)
def test_ties_in_the_carried_candidate(engine, monkeypatch, mode):
    case = tie_case()
    g, probs, sp, exp = case
    assert sum(1 for s, pairs in exp if pairs) >= 500
    _run(engine, monkeypatch, mode, case)


# ---- rows still in the band after the last column; the shortest fills ----
def _rows_left(p, side):
    """Rows 1 .. rlength - 1 of a fill that have not passed band offset 0 by its last column."""
    glen = p["glength" + side]
    uband = glen - p["rlength"] + p["extraband"]
    return sum(1 for r in range(1, p["rlength"]) if r + uband > glen)


@functools.lru_cache(maxsize=None)
def end_case():
    rng = random.Random(11500)
    g = bytearray(random_genome(rng, 400000, nfrac=0.0))
    at = [2000]
    probs = []
    for eb in (0, 1, 14, 20):
        for rlen in (2, 3, 5, 17, 40, 70):
            for e in ((1, 1), (1, 8), (8, 1), (8, 8)):
                for late in (False, True):
                    kind = rng.choice(["strong", "weak", "ins"])
                    probs.append(_sides(_gap(rng, g, at, rlen, kind, extraband=eb, extra=8, late=late), *e))
    g = bytes(g)
    sp = [_synthetic_probs(rng, p) for p in probs]
    return g, probs, sp, _expected(g, probs, sp)


@pytest.mark.parametrize("mode", MODES)
def test_rows_in_the_band_after_the_last_column(engine, monkeypatch, mode):
    case = end_case()
    g, probs, sp, exp = case
    left = [_rows_left(p, s) for p in probs for s in ("L", "R")]
    # gaps that end with rows in the band (as many as extraband allows), and gaps whose rows have all left it
    assert max(left) >= 19 and any(n == 0 for p, n in zip([p for p in probs for _ in "LR"], left) if p["rlength"] >= 17)
    assert any(p["glengthL"] == 3 for p in probs) and any(p["glengthR"] == 3 for p in probs)
    assert sum(1 for s, pairs in exp if pairs) >= len(probs) // 3
    _run(engine, monkeypatch, mode, case)
