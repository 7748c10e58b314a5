"""The yardstick of the Stage2_scan tests: ncovered from a diagonal list by Diag_update_coverage's rule
(diag.c:230-244 with coveredp all false), and the expected gmapdp_scan_result of a call from an oracle's
Oligoindex_get_mappings output (Oracle.oligo_mappings / Ref.oligo_mappings with the major index).  Nothing
here calls the engine."""
import numpy as np


def ncovered_from_diagonals(diagonals, querylength):
    """diagonals: (diagonal, querystart, queryend, nconsecutive) records.  scores[querystart] += 1 and
    scores[queryend] -= 1 per record; a query position is covered where the running sum is > 0."""
    scores = np.zeros(querylength + 1, dtype=np.int64)
    for _, qs, qe, _ in diagonals:
        scores[qs] += 1
        scores[qe] -= 1
    return int(np.count_nonzero(np.cumsum(scores[:querylength]) > 0))


def expected_scan(impl, p):
    """(ncovered, stage2_source, totalpositions, maxnconsecutive) of Stage2_scan on call p, from impl's
    seeding with the major index (minor 0)."""
    q = dict(p)
    q["minor"] = 0
    out = impl.oligo_mappings(q)
    assert len(out) == 4, "oracle status %s for %s" % (out, {k: v for k, v in p.items() if k != "quc"})
    sc, _, _, dg = out
    return (ncovered_from_diagonals(dg, len(p["quc"])), 1, int(sc[0]), int(sc[1]))


def expected_scans(impl, probs):
    return np.array([expected_scan(impl, p) for p in probs], dtype=np.int32).reshape(len(probs), 4)
