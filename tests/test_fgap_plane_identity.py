"""The Fgap direction plane of the banded fill, stored one row up.

Dynprog_standard decides Fgap(r, c) from the cell above, `F(r-1, c) > H(r-1, c) + open` (`>=` for
jump_late), while it walks down column c.  fill_band stores that bit with cell (r-1, c), formed from
the registers of the lane that owns that cell, and every reader takes the bit of (r, c) from band
offset k-1 of the same column.  This test restates a plain banded fill on the CPU and checks, over a
grid of shapes, bands and penalties, that the two are the same plane:

  * for every valid cell (r, c) with a valid cell above it, the bit the reference forms at (r, c)
    equals the bit formed at (r-1, c) from that cell's own F and H;
  * at a column's first valid row, where the moved plane reads 0, the reference's bit is either
    false or belongs to a cell whose F is -infinity: no traceback can be in the F state there.
"""
import random

import numpy as np

NEG = -(1 << 28)  # the fill's -infinity; finite scores stay within a few hundred of zero


def banded_fill(rng, rlen, glen, lband, uband, late):
    """One Dynprog_standard fill (upper and lower band, score saturation at NEG).  Returns the valid mask,
    F, H (after the F chain) and the Fgap bit as the reference forms it, all indexed [r, c]."""
    open_, ext = -rng.randint(1, 12), -rng.randint(1, 3)
    q = [rng.randrange(4) for _ in range(rlen + 1)]
    g = [rng.randrange(4) for _ in range(glen + 1)]
    match, mismatch = rng.randint(1, 3), -rng.randint(1, 5)
    H = np.full((rlen + 1, glen + 1), NEG, dtype=np.int64)
    E = np.full((rlen + 1, glen + 1), NEG, dtype=np.int64)
    F = np.full((rlen + 1, glen + 1), NEG, dtype=np.int64)
    valid = np.zeros((rlen + 1, glen + 1), dtype=bool)
    old = np.zeros((rlen + 1, glen + 1), dtype=bool)
    H[0, 0] = 0
    for r in range(1, min(lband, rlen) + 1):
        H[r, 0] = open_ + r * ext
    for c in range(1, min(uband, glen) + 1):
        H[0, c] = open_ + c * ext
    for c in range(1, glen + 1):
        rlo, rhigh = max(1, c - uband), min(rlen, c + lband)
        # the nogap value above row rlo: row 0 inside the band, nothing once the band top has left it
        if c == 1:
            hprev = NEG - open_ + 1
        elif c <= uband:
            hprev = int(H[0, c])
        else:
            hprev = NEG
        fprev = NEG
        for r in range(rlo, rhigh + 1):
            valid[r, c] = True
            e = max(int(E[r, c - 1]), int(H[r, c - 1]) + open_) + ext
            s = match if q[r] == g[c] else mismatch
            hp = max(e, int(H[r - 1, c - 1]) + s)
            old[r, c] = fprev > hprev + open_ - late
            f = max(NEG, max(fprev, hprev + open_)) + ext
            h = max(f, hp)
            E[r, c], F[r, c], H[r, c] = e, f, max(h, NEG)
            fprev, hprev = f, h
    return valid, F, H, old, open_


def test_fgap_bit_is_a_property_of_the_cell_above():
    rng = random.Random(20240607)
    cells = tops = tops_set = 0
    for rlen in range(1, 13):
        for glen in range(1, 15):
            for lband in range(6):
                for uband in range(6):
                    for late in (0, 1):
                        valid, F, H, old, open_ = banded_fill(rng, rlen, glen, lband, uband, late)
                        new = valid & (F > H + open_ - late)  # each cell's own registers
                        below = valid[1:, :] & valid[:-1, :]  # (r, c) with a valid (r-1, c)
                        assert np.array_equal(old[1:, :][below], new[:-1, :][below]), (rlen, glen, lband, uband, late)
                        cells += int(below.sum())
                        top = valid.copy()
                        top[1:, :] &= ~valid[:-1, :]  # a column's first valid row
                        bad = top & old & (F > NEG // 2)
                        assert not bad.any(), (rlen, glen, lband, uband, late, np.argwhere(bad)[:4])
                        tops += int(top.sum())
                        tops_set += int((top & old).sum())
    # the grid does reach both situations: interior cells, and set top-row bits past uband
    assert cells > 100000 and tops > 50000 and tops_set > 1000
