"""What the stage-2 seeding entry points refuse, and with which words: gmapdp_oligo_plan_create,
gmapdp_scan_plan_create, gmapdp_stage2_plan_create and gmapdp_stage2_batch share one per-problem validation
(length, query slice, window inside the genome, distinct 8-mers), and the first bad problem in index order
decides the message.  Every case is refused before any seeding kernel is launched: the device work here is the
context's set-up and the genome upload."""
import ctypes as C
import random

import numpy as np
import pytest

import gmapdp
from dpbind import random_genome

pytestmark = pytest.mark.gpu

EINVAL = -1
GENOME_NT = 5000
SHORT = "stage-2 seeding needs querylength > 8 (Oligoindex_set_inquery)"
SLICE = "query outside the arena"
WINDOW = "stage-2 window past the genome"
DISTINCT = "query with more than 16384 distinct 8-mers"
MINOR = "Stage2_scan takes the major oligoindex only (minor must be 0)"
INTRON = "stage 2: negative maxintronlen"
FLAGS = "stage 2: unknown bits in flags"

_RNG = random.Random(4711)
QUC = bytes(_RNG.choice(b"ACGT") for _ in range(40000))  # about 30 000 of the 65 536 8-mers
QBYTES = len(QUC)


def _p(qoff=0, querylength=100, chrstart=0, chrend=4000, plusp=1, minor=0, maxintronlen=1000, flags=0):
    return dict(qoff=qoff, querylength=querylength, chrstart=chrstart, chrend=chrend, chroffset=0,
                chrhigh=GENOME_NT, plusp=plusp, minor=minor, splicingp=1, maxintronlen=maxintronlen, flags=flags)


GOOD = _p()
BAD_SHORT = _p(querylength=8)
BAD_SLICE = _p(qoff=QBYTES - 50, querylength=100)
BAD_WINDOW = _p(chrend=20000)
BAD_DISTINCT = _p(querylength=QBYTES)


def _array(problems, dtype):
    a = np.zeros(len(problems), dtype=dtype)
    for i, p in enumerate(problems):
        for k in dtype.names:
            a[i][k] = p[k]
    return a


@pytest.fixture(scope="module")
def eng():
    e = gmapdp.Engine(0)
    e.set_genome(random_genome(random.Random(4712), GENOME_NT))
    yield e
    e.close()


def _err(eng):
    return eng.lib.gmapdp_last_error(eng.h).decode()


def _oligo_plan(eng, problems):
    a, plan = _array(problems, gmapdp.OLIGO_PROBLEM_DTYPE), C.c_void_p()
    rc = eng.lib.gmapdp_oligo_plan_create(eng.h, a.ctypes.data, len(a), QUC, QBYTES, C.byref(plan))
    if plan:
        eng.lib.gmapdp_oligo_plan_destroy(plan)
    return rc, _err(eng) if rc else ""


def _scan_plan(eng, problems):
    a, plan = _array(problems, gmapdp.OLIGO_PROBLEM_DTYPE), C.c_void_p()
    rc = eng.lib.gmapdp_scan_plan_create(eng.h, a.ctypes.data, len(a), QUC, QBYTES, C.byref(plan))
    if plan:
        eng.lib.gmapdp_scan_plan_destroy(plan)
    return rc, _err(eng) if rc else ""


def _stage2_plan(eng, problems):
    a, plan = _array(problems, gmapdp.STAGE2_PROBLEM_DTYPE), C.c_void_p()
    rc = eng.lib.gmapdp_stage2_plan_create(eng.h, a.ctypes.data, len(a), QUC, QUC, QBYTES, C.byref(plan))
    if plan:
        eng.lib.gmapdp_stage2_plan_destroy(plan)
    return rc, _err(eng) if rc else ""


def _stage2_batch(eng, problems):
    a = _array(problems, gmapdp.STAGE2_PROBLEM_DTYPE)
    results = np.zeros(len(a), dtype=gmapdp.STAGE2_RESULT_DTYPE)
    pn, qn = C.c_size_t(), C.c_size_t()
    rc = eng.lib.gmapdp_stage2_batch(eng.h, a.ctypes.data, len(a), QUC, QUC, QBYTES, results.ctypes.data, None, 0,
                                     None, 0, C.byref(pn), C.byref(qn))
    return rc, _err(eng) if rc else ""


ALL = (_oligo_plan, _scan_plan, _stage2_plan, _stage2_batch)
STAGE2 = (_stage2_plan, _stage2_batch)

# (problems, entry points, message)
CASES = {
    "querylength_8": ([BAD_SHORT], ALL, SHORT),
    "slice_past_qbytes": ([BAD_SLICE], ALL, SLICE),
    "negative_qoff": ([_p(qoff=-1)], ALL, SLICE),
    "window_past_genome": ([BAD_WINDOW], ALL, WINDOW),
    "window_past_genome_minus": ([_p(chrend=20000, plusp=0)], ALL, WINDOW),
    "distinct_8mers": ([BAD_DISTINCT], ALL, DISTINCT),
    # within one problem: the slice before the window, the window before the distinct 8-mers
    "slice_then_window": ([_p(qoff=QBYTES - 50, chrend=20000)], ALL, SLICE),
    "window_then_distinct": ([_p(querylength=QBYTES, chrend=20000)], ALL, WINDOW),
    # the first bad problem in index order decides, whichever pass over the problems finds it
    "earlier_window_later_short": ([GOOD, BAD_WINDOW, BAD_SHORT], ALL, WINDOW),
    "earlier_short_later_window": ([BAD_SHORT, GOOD, BAD_WINDOW], ALL, SHORT),
    "earlier_distinct_later_slice": ([BAD_DISTINCT, BAD_SLICE], ALL, DISTINCT),
    "earlier_slice_later_distinct": ([BAD_SLICE, BAD_DISTINCT], ALL, SLICE),
    # Stage2_scan alone: the minor index, tested before the length
    "scan_minor": ([_p(minor=1)], (_scan_plan,), MINOR),
    "scan_minor_before_length": ([_p(minor=1, querylength=8)], (_scan_plan,), MINOR),
    "scan_earlier_window_later_minor": ([BAD_WINDOW, _p(minor=1)], (_scan_plan,), WINDOW),
    "scan_earlier_minor_later_window": ([_p(minor=1), BAD_WINDOW], (_scan_plan,), MINOR),
    # Stage2_compute: the flags, then every problem's maxintronlen, then the seeding's validation
    "stage2_flags_before_intron": ([_p(maxintronlen=-1, flags=2)], STAGE2, FLAGS),
    "stage2_later_intron_before_earlier_short": ([BAD_SHORT, _p(maxintronlen=-1)], STAGE2, INTRON),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal(eng, name):
    problems, entries, message = CASES[name]
    for entry in entries:
        assert entry(eng, problems) == (EINVAL, message), entry.__name__


def test_minor_index_is_the_scan_plans_rule_only(eng):
    """The seeding plan takes the minor index: the same problems pass there (and fail on the length alone)."""
    assert _oligo_plan(eng, [_p(minor=1)]) == (0, "")
    assert _oligo_plan(eng, [_p(minor=1, querylength=8)]) == (EINVAL, SHORT)
