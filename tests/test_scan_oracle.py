"""The Stage2_scan tests' yardstick (tests/scanref.py) against the reference's own objects, on the CPU.

Stage2_scan (stage2.c:5610) is one seeding with the major index plus Diag_update_coverage; Stage2_compute
(stage2.c:6325) seeds with the same index and takes the same coverage before its proceed test.  So, on 300
seeded problems: the helper over the reference objects' diagonals (Ref.oligo_mappings, minor 0) equals the
helper over the oracle's, and both equal the ncovered orc_stage2_compute reports (scalars[2]) wherever that
call's status is 1 or 2.  refh_stage2_compute exports only its result count and the start/end-list flag
(scalars[0..1]; oracle/refharness.c), not Stage2_compute's local ncovered, so the reference's own
Diag_update_coverage is pinned through what it decides: where the helper's ncovered fails the proceed test
(querylength > 150, under 30 % and under 200 positions covered: status 1), the reference's Stage2_compute
returns no result, and wherever the reference returns a result the helper's ncovered passes the test."""
import random

import pytest

from dpbind import Oracle, Ref, oligo_problem, random_genome, ref_available, repeat_genome, stage2_problem
from scanref import ncovered_from_diagonals

pytestmark = pytest.mark.skipif(not ref_available("nosimd"), reason="reference objects (oracle/_ref) not built here")


def test_ncovered_rule_on_hand_made_lists():
    assert ncovered_from_diagonals([], 50) == 0
    assert ncovered_from_diagonals([(7, 3, 10, 8)], 50) == 7                      # [3, 10)
    assert ncovered_from_diagonals([(7, 3, 10, 8), (9, 10, 20, 11)], 50) == 17    # touching
    assert ncovered_from_diagonals([(7, 3, 10, 8), (9, 5, 8, 4), (1, 40, 49, 9)], 50) == 16  # nested + apart
    assert ncovered_from_diagonals([(7, 0, 49, 50)], 50) == 49                    # queryend = querylength - 1
    assert ncovered_from_diagonals([(7, 4, 4, 1)], 50) == 0                       # querystart == queryend


@pytest.mark.parametrize("kind", ["random", "repeat"])
def test_scan_yardstick_matches_reference(kind):
    rng = random.Random(9200 + (kind == "repeat"))
    g = random_genome(rng, 300000) if kind == "random" else repeat_genome(rng, 300000)
    ref, orc = Ref("nosimd"), Oracle()
    ref.set_genome(g)
    orc.set_genome(g)
    nstat = {0: 0, 1: 0, 2: 0}
    npos = 0
    for i in range(150):
        p = stage2_problem(rng, g, edge=(i % 5 == 0)) if i % 2 else dict(oligo_problem(rng, g, edge=(i % 4 == 0)), minor=0)
        p.setdefault("q", p["quc"])
        ql = len(p["quc"])
        r, o = ref.oligo_mappings(p), orc.oligo_mappings(p)
        assert len(r) == 4 and len(o) == 4, i
        nr, no = ncovered_from_diagonals(r[3], ql), ncovered_from_diagonals(o[3], ql)
        assert nr == no, (i, nr, no)
        assert r[0][:2] == o[0][:2], i  # totalpositions, maxnconsecutive: the other two result fields
        npos += nr > 0
        orc.stage2_compute(p)
        ncov, status = orc._s2_sc[2], orc._s2_sc[3]
        nstat[status] += 1
        if status in (1, 2):
            assert ncov == nr, (i, ncov, nr)
        gate_fails = ql > 150 and nr / ql < 0.3 and nr < 200
        assert (status == 1) == (r[0][0] > 0 and gate_fails), i
        rr = ref.stage2_compute(p)
        assert rr[0] != "err", i
        if gate_fails:
            assert rr[0] == 0, i
        if rr[0] > 0:
            assert not gate_fails and nr > 0, i
    assert npos > 100 and nstat[2] > 80 and nstat[1] + nstat[0] > 0, (npos, nstat)
