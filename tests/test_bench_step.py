"""CPU side of the bench-step tests (tests/benchstep.py, tests/test_gpu_bench_step.py):

  * the comparator is sensitive: the oracle's own outputs of the 200-read block, re-expressed in the engine's
    formats, compare clean; one flipped byte of one pair record, one status, one npairs, one stage-2 path's
    npairs are each reported for exactly that call and nothing else;
  * the blocks are what the GPU tests take them for: the 200-read block's call mix, every Stage2_compute
    call of every block chains (status 2), and at least 90 % of every block's genome gaps emit pairs, in
    both builds' semantics -- so the GPU tests' premises on the engine's outputs follow from parity."""
import numpy as np
import pytest

import gmapdp

import benchstep as BS


def oracle_as_engine(oracle):
    """oracle_block's outputs in the formats Bench.fetch returns the engine's in"""
    dp, s2 = oracle
    got = {}
    for fam in ("single", "end", "genome"):
        scal, dscal, pairs, pair_off = dp[fam]
        res = np.zeros(len(scal), dtype=gmapdp.GENOME_RESULT_DTYPE if fam == "genome" else gmapdp.RESULT_DTYPE)
        res["npairs"] = np.maximum(scal[:, 0], 0)
        res["pair_offset"] = pair_off[:-1]
        names = ["dynprogindex", "traceback_score", "nmatches", "nmismatches", "nopens", "nindels"]
        if fam == "genome":
            names += ["new_leftgenomepos", "new_rightgenomepos", "exonhead", "introntype"]
            res["left_prob"], res["right_prob"] = dscal[:, 0], dscal[:, 1]
            res["gap_index"], res["gap_queryjump"] = scal[:, 12], scal[:, 13]
        for k, nm in enumerate(names):
            res[nm] = scal[:, 1 + k]
        got[fam] = (res, pairs.copy())
    scal, dscal, pairs, pair_off = dp["microexon"]
    res = np.zeros(len(scal), dtype=gmapdp.MICROEXON_RESULT_DTYPE)
    res["npairs"], res["dynprogindex"], res["microintrontype"] = scal[:, 0], scal[:, 1], scal[:, 2]
    res["bestprob2"], res["bestprob3"] = dscal[:, 0], dscal[:, 1]
    res["pair_offset"] = pair_off[:-1]
    got["microexon"] = (res, pairs.copy())
    scal, opaths, opairs, pair_off = s2
    res = np.zeros(len(scal), dtype=gmapdp.STAGE2_RESULT_DTYPE)
    for k, nm in enumerate(("nresults", "npaths", "ncovered", "status", "diag_querystart", "diag_queryend")):
        res[nm] = scal[:, k]
    paths = []
    for j in range(len(scal)):
        res["path_offset"][j] = len(paths)
        for k in range(int(scal[j, 0])):
            paths.append((int(pair_off[j]) + int(opaths[j, k, 0]), int(opaths[j, k, 1]), 0))
        res["npairs"][j] = sum(int(opaths[j, k, 1]) for k in range(int(scal[j, 0])))
    n = len(opairs) // 20
    got["stage2"] = (res, np.array(paths, dtype=gmapdp.PATH_DTYPE),
                     np.frombuffer(opairs[:20 * n].tobytes(), dtype=gmapdp.PATH_PAIR_DTYPE).copy())
    return got


def _copy(got):
    return {k: tuple(a.copy() for a in v) for k, v in got.items()}


@pytest.fixture(scope="module")
def oracle200():
    return BS.block200_oracle()


def test_comparator_accepts_the_oracle(oracle200):
    assert BS.step_mismatches(oracle_as_engine(oracle200), oracle200) == []
    assert BS.step_mismatches(oracle_as_engine(oracle200), oracle200, stage2_paths=False) == []


@pytest.mark.parametrize("fam", ["single", "end", "genome", "microexon"])
def test_comparator_reports_one_flipped_pair_byte(oracle200, fam):
    got = _copy(oracle_as_engine(oracle200))
    res, pairs = got[fam]
    # the last problem with records whose first record is an ordinary pair (a gap holder's characters are
    # not part of what the reference's callers read; the comparator blanks them on both sides)
    for i in range(len(res) - 1, -1, -1):
        if res["npairs"][i] > 0 and pairs["querypos"][int(res["pair_offset"][i])] >= 0:
            break
    else:
        pytest.fail("no %s problem with records" % fam)
    at = int(res["pair_offset"][i]) + int(res["npairs"][i]) - 1   # its last record
    raw = pairs.view(np.uint8).reshape(-1, 16)
    for byte in (0, 4, 8, 12, 13, 14, 15) if pairs["querypos"][at] >= 0 else (0, 4, 8):
        saved = raw[at, byte]
        raw[at, byte] ^= 0x01
        assert BS.step_mismatches(got, oracle200) == [(fam, i, "pair records")], (at, byte)
        raw[at, byte] = saved
    assert BS.step_mismatches(got, oracle200) == []


def test_comparator_reports_one_status_one_npairs_one_path(oracle200):
    base = oracle_as_engine(oracle200)
    # one status
    got = _copy(base)
    i = len(got["stage2"][0]) // 2
    got["stage2"][0]["status"][i] = 1
    assert [b[:2] for b in BS.step_mismatches(got, oracle200)] == [("stage2", i)]
    assert [b[:2] for b in BS.step_mismatches(got, oracle200, stage2_paths=False)] == [("stage2", i)]
    # one npairs, in every DP family
    for fam in BS.DP_FAMS:
        got = _copy(base)
        res = got[fam][0]
        i = int(np.nonzero(res["npairs"] > 1)[0][-1])
        res["npairs"][i] -= 1
        assert BS.step_mismatches(got, oracle200) == [(fam, i, "npairs")]
    # one stage-2 path's npairs (the call's last kept path)
    got = _copy(base)
    res, paths, _ = got["stage2"]
    i = int(np.nonzero(res["nresults"] > 0)[0][-1])
    k = int(res["nresults"][i]) - 1
    paths["npairs"][int(res["path_offset"][i]) + k] -= 1
    assert BS.step_mismatches(got, oracle200) == [("stage2", i, "path %d" % k)]
    # one byte of one stage-2 pair record
    got = _copy(base)
    res, paths, pairs = got["stage2"]
    at = int(paths["pair_offset"][int(res["path_offset"][i])]) + 3
    pairs.view(np.uint8).reshape(-1, 20)[at, 17] ^= 0x20
    assert BS.step_mismatches(got, oracle200) == [("stage2", i, "path 0")]
    # the total record count of a result whose paths are gone
    got = _copy(base)
    got["stage2"][0]["npairs"][i] += 1
    assert BS.step_mismatches(got, oracle200, stage2_paths=False) == [("stage2", i, "npairs")]


def test_scratch_overlaps_sees_overlap_and_overrun():
    z = np.zeros(0, dtype=np.int64)
    a = (0, 0, 512, np.array([0, 256]), np.array([256, 256]))
    b = (1, 512, 256, np.array([512]), np.array([256]))
    assert BS.scratch_overlaps([a, b, (2, 0, 0, z, z)], 768) == []
    assert len(BS.scratch_overlaps([a, b], 700)) == 1                      # past the total
    c = (1, 256, 512, np.array([256 + 128]), np.array([256]))              # into a's second member
    assert any("overlap" in m for m in BS.scratch_overlaps([a, c], 1024))
    d = (1, 512, 256, np.array([256]), np.array([256]))                    # a member outside its launch's range
    assert any("outside" in m for m in BS.scratch_overlaps([a, d], 1024))


def _close(x, ref):
    return abs(x - ref) <= 0.01 * ref


def test_block200_is_the_bench_call_mix(oracle200):
    """A 200-read CDNA2K block on the two-chromosome layout: bench.py's call mix and window shape at 1/50 of
    the size (counts as measured when the step tests were written, within 1 %)."""
    genome, d = BS.block200()
    dp, s2 = oracle200
    assert _close(len(d["single"]), 4220) and _close(len(d["end"]), 2632) and _close(len(d["genome"]), 9940)
    assert _close(len(d["microexon"]), 1506) and _close(len(d["oligo"]), 317)
    assert _close(int((dp["genome"][0][:, 0] > 0).sum()), 9869)
    win = (d["oligo"]["chrend"].astype(np.int64) - d["oligo"]["chrstart"].astype(np.int64))
    assert win.min() >= 199_000 and win.max() <= 237_000
    assert np.all(s2[0][:, 3] == 2), "every Stage2_compute call chains"
    assert len(set(int(x) for x in d["genome"]["chroffset"])) == 2     # both chromosomes


@pytest.mark.parametrize("simd", [False, True])
def test_blocks3_premises(simd):
    """The 120 / 200 / 120-read blocks of the pipelined-step test: every Stage2_compute call chains and at
    least 90 % of the genome gaps emit pairs, so the GPU test's parity is over real work.  In the nosimd
    semantics that holds for every block (99.5 %, 99.6 %, 99.8 %); the reference's SIMD builds return NULL for
    more of these gaps (89.2 %, 90.7 %, 92.8 % emit), so there it holds over the test's three blocks together
    (90.9 %) and each block stays above 85 %."""
    genome, data = BS.blocks3()
    assert [int(d["reads"]) for d in data] == [120, 200, 120]
    emit = []
    for d, (dp, s2) in zip(data, BS.blocks3_oracle(simd)):
        assert len(s2[0]) == len(d["oligo"]) > 150 and np.all(s2[0][:, 3] == 2)
        emit.append(dp["genome"][0][:, 0] > 0)
        assert emit[-1].mean() >= (0.85 if simd else 0.9)
        assert len(d["microexon"]) > 500 and len(d["single"]) > 2000 and len(d["end"]) > 1000
        for fam in BS.DP_FAMS:
            assert np.all(dp[fam][0][:, 0] >= -1) and np.all(dp[fam][0][:, 15] == 0)   # no oracle error
    assert np.concatenate(emit).mean() >= 0.9
