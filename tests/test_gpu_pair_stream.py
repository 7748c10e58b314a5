"""The compact pair stream of the shipped kernel (pc_kernel.hip, through gmapdp_compact_pairs and
gmapdp_compact_path_pairs) against the plain-Python reference of the format (tests/pcstream.py), on small
caller-made lists at the kernel's edges, for both record types.  For every case:
  (a) the stream is byte-equal to the reference encoder's;
  (b) the offsets are the reference's prefix sums;
  (c) gmapdp_expand_* of the kernel's stream restores the exact records and leaves the arena outside the
      lists untouched;
  (d) the total is at most gmapdp_compact_bound;
  (e) the guard bytes behind the stream are intact.
The output buffer is sized from the kernel's own sizing pass, never from the bound."""
import numpy as np
import pytest

import gmapdp
import pcstream as pc

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("path", [False, True], ids=["pairs", "path_pairs"])


@pytest.fixture(scope="module")
def eng():
    e = gmapdp.Engine(0)
    yield e
    e.close()


def check(eng, name, lists, path, got, nrecords, effective=None):
    """(a)-(e) for one launch: got = (stream, offsets, guard intact); effective: the lists as the stream must
    hold them (default: as given); nrecords: the arena's records, for the bound."""
    stream, offs, guard = got[:3]
    effective = lists if effective is None else effective
    want, woffs = pc.encode(effective)
    assert guard, "%s: (e) bytes written past the sizing pass's total" % name
    assert int(offs[-1]) <= eng.lib.gmapdp_compact_bound(nrecords, int(path)), \
        "%s: (d) %d bytes for %d records, the bound is %d" % (name, int(offs[-1]), nrecords,
                                                             eng.lib.gmapdp_compact_bound(nrecords, int(path)))
    assert np.array_equal(offs, woffs), "%s: (b) offsets differ from the reference's, first at list %d" % (
        name, int(np.flatnonzero(offs != woffs)[0]) - 1)
    assert stream == want, "%s: (a) %s" % (name, pc.first_difference(stream, want, woffs))
    rc, arena, expected = pc.expand(stream, offs, effective, path, nthreads=4)
    assert rc == 0, "%s: (c) gmapdp_expand refuses the kernel's stream (%d)" % (name, rc)
    assert arena.tobytes() == expected.tobytes(), "%s: (c) the expansion differs from the records" % name


def run_cases(eng, cases, path, gap=3):
    for name, lists in cases.items():
        got = pc.run_kernel(eng, lists, path, gap=gap)
        check(eng, name, lists, path, got, len(got[3]))


@BOTH
def test_list_lengths(eng, path):
    run_cases(eng, pc.length_cases(path), path)
    # and all of them in one launch
    lists = [x for c in pc.length_cases(path).values() for x in c]
    got = pc.run_kernel(eng, lists, path)
    check(eng, "all lengths", lists, path, got, len(got[3]))


@BOTH
def test_step_boundaries(eng, path):
    run_cases(eng, pc.boundary_cases(path), path)


@BOTH
def test_steps(eng, path):
    run_cases(eng, pc.step_cases(path), path)


@BOTH
def test_characters(eng, path):
    run_cases(eng, pc.char_cases(path), path)


@BOTH
def test_worst_case_list_fills_the_arena(eng, path):
    """Escaped records whose step alternates: 18 B per record (less 13), the whole arena one list."""
    run_cases(eng, pc.worst_case(path), path, gap=0)


@BOTH
def test_run_cap(eng, path):
    """Diagonal runs of 65 534 ... 131 071 records and an indel run of 70 000 escaped ones, one launch: a run
    holds 65 535 records at the most."""
    run_cases(eng, pc.run_cap_cases(path), path)


def test_negative_npairs_is_an_empty_list(eng):
    lists = [pc.diagonal(False, 5), pc.diagonal(False, 70, 9, 9), pc.diagonal(False, 4, 50, 50, (1, 0))]
    arena, offs = pc.lay_out(lists, False)
    res = np.zeros(3, dtype=gmapdp.RESULT_DTYPE)
    res["npairs"] = [5, -70, 4]
    res["pair_offset"] = offs
    gres = np.zeros(2, dtype=gmapdp.GENOME_RESULT_DTYPE)
    gres["npairs"] = [-1, -2 ** 31]
    gres["pair_offset"] = [offs[1], -5]
    got = pc.compact_pairs(eng, res, gres, arena)
    empty = pc.diagonal(False, 0)
    check(eng, "negative npairs", None, False, got, len(arena), effective=[lists[0], empty, lists[2], empty, empty])


@pytest.mark.parametrize("n0,n1", [(0, 3), (3, 0), (0, 0), (2, 2), (1, 1)])
def test_dp_segments(eng, n0, n1):
    """The two result segments and their strides: gmapdp_result records, then gmapdp_genome_result records."""
    lists = [pc.diagonal(False, 3 + 40 * i, 10 * i, 1000 * i, chars=pc.mixed_chars(3 + 40 * i, i))
             for i in range(n0 + n1)]
    got = pc.run_kernel(eng, lists, False, n0=n0)
    assert len(got[1]) == n0 + n1 + 1
    check(eng, "segments %d + %d" % (n0, n1), lists, False, got, len(got[3]))


@BOTH
@pytest.mark.parametrize("count", [1, 2, 1023, 1024, 1025, 2049])
def test_list_counts_of_the_scan(eng, path, count):
    """The offsets scan (one workgroup of 1024, ceil(count / 1024) lists per thread): mostly empty lists, a
    few non-empty ones at the first, last and chunk-boundary indices."""
    per = (count + 1023) // 1024
    at = {0, 1, per - 1, per, 2 * per - 1, 2 * per, 511 * per, 512 * per, 1022, 1023, 1024, 1025, count // 2,
          count - per - 1, count - per, count - 2, count - 1}
    n = [1 + i % 7 if i in at else 0 for i in range(count)]
    lists = [pc.diagonal(path, n[i], i, 3 * i, chars=pc.mixed_chars(n[i], i)) for i in range(count)]
    got = pc.run_kernel(eng, lists, path, gap=1)
    check(eng, "%d lists" % count, lists, path, got, len(got[3]))


def test_path_guards(eng):
    """PcPaths::list: lists past *npaths are empty; a path with a negative offset or count, or one that ends
    past pair_cap, is an empty list, and its neighbours are unaffected."""
    lists = [pc.diagonal(True, 5 + 30 * i, 100 * i, 7 * i, chars=pc.mixed_chars(5 + 30 * i, i)) for i in range(8)]
    arena, offs = pc.lay_out(lists, True, gap=2)
    cap = offs[7] + len(lists[7])          # pair_cap: the last list ends exactly at it (the arena is longer)
    empty = pc.diagonal(True, 0)

    def paths_of(npairs, offsets):
        p = np.zeros(len(npairs), dtype=gmapdp.PATH_DTYPE)
        p["npairs"], p["pair_offset"] = npairs, offsets
        return p
    n = [len(x) for x in lists]
    # all valid, the last one ending at pair_cap
    got = pc.compact_path_pairs(eng, paths_of(n, offs), 8, arena, pair_cap=cap)
    check(eng, "all paths", None, True, got, cap, effective=lists)
    # lists past *npaths
    for npaths in (0, 1, 5, 7):
        got = pc.compact_path_pairs(eng, paths_of(n, offs), npaths, arena, pair_cap=cap)
        check(eng, "npaths %d" % npaths, None, True, got, cap, effective=lists[:npaths] + [empty] * (8 - npaths))
    # bad paths between good ones
    bad_n, bad_o, eff = list(n), list(offs), list(lists)
    bad_o[1] = -1
    bad_n[3] = -n[3]
    bad_o[5] = cap - n[5] + 1               # ends one record past pair_cap
    bad_o[7] = offs[7] + 1                  # the same, at the arena's end
    for i in (1, 3, 5, 7):
        eff[i] = empty
    got = pc.compact_path_pairs(eng, paths_of(bad_n, bad_o), 8, arena, pair_cap=cap)
    check(eng, "bad paths", None, True, got, cap, effective=eff)
    # offsets and counts that overflow a sum of 32 or 64 bits
    huge_n, huge_o = list(n), list(offs)
    huge_o[2] = 2 ** 63 - 1
    huge_o[4] = 2 ** 32
    huge_n[6], huge_o[6] = 2 ** 31 - 1, cap
    eff = list(lists)
    for i in (2, 4, 6):
        eff[i] = empty
    got = pc.compact_path_pairs(eng, paths_of(huge_n, huge_o), 8, arena, pair_cap=cap)
    check(eng, "huge paths", None, True, got, cap, effective=eff)


@BOTH
def test_random_lists(eng, path):
    """A few thousand lists of 0-300 records from a persistent random walk over the nine steps, with a few
    percent each of RAW records, position jumps and escaped characters (fixed seed)."""
    lists = pc.random_case(path)
    got = pc.run_kernel(eng, lists, path, gap=1)
    check(eng, "random", lists, path, got, len(got[3]))
