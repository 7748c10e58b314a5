"""CPU tests of the Stage2_scan entry points' C ABI and their Python mirror (no device compute here)."""
import ctypes as C
import os
import subprocess

import numpy as np

import gmapdp

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = ("gmapdp_stage2_scan_batch", "gmapdp_scan_plan_create", "gmapdp_scan_plan_run", "gmapdp_scan_plan_nlaunches",
           "gmapdp_scan_plan_destroy")
FIELDS = ("ncovered", "stage2_source", "totalpositions", "maxnconsecutive")


def test_scan_symbols_are_declared_and_exported():
    lib = gmapdp.load_library()
    declared = gmapdp.exported_symbols()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s  # the binding gives every entry point a signature


def test_scan_result_layout_matches_the_c_header(tmp_path):
    """sizeof(gmapdp_scan_result) == 16 and the fields at 0, 4, 8, 12 in the declared order, as a C compiler lays
    out include/gmapdp.h; the ctypes structure and the numpy dtype match."""
    src = tmp_path / "scan_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmapdp.h"\nint main(void) {\n'
                   'printf("%zu\\n", sizeof(gmapdp_scan_result));\n' +
                   "".join('printf("%%zu\\n", offsetof(gmapdp_scan_result, %s));\n' % f for f in FIELDS) +
                   'return 0; }\n')
    exe = tmp_path / "scan_layout"
    subprocess.run(["gcc", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [16, 0, 4, 8, 12]
    assert C.sizeof(gmapdp.ScanResult) == 16
    assert [n for n, _ in gmapdp.ScanResult._fields_] == list(FIELDS)
    assert [getattr(gmapdp.ScanResult, f).offset for f in FIELDS] == out[1:]
    assert all(t is C.c_int32 for _, t in gmapdp.ScanResult._fields_)
    assert gmapdp.SCAN_RESULT_DTYPE.itemsize == 16 and gmapdp.SCAN_RESULT_DTYPE.names == FIELDS
    # the (n, 4) int32 array Engine.stage2_scan_batch returns is the same memory as n records
    a = np.arange(8, dtype=np.int32).reshape(2, 4)
    assert a.view(gmapdp.SCAN_RESULT_DTYPE)["totalpositions"].ravel().tolist() == [2, 6]


def test_scan_batch_builder_shares_a_reads_slice():
    """Engine.build_scan_batch: calls carrying the same query object get one slice of the arena."""
    q1, q2 = b"ACGTACGTACGT", b"TTTTACGTACGTAA"
    calls = [dict(quc=q1, chrstart=0, chrend=100, chroffset=0, chrhigh=1000, plusp=1),
             dict(quc=q2, chrstart=5, chrend=50, chroffset=0, chrhigh=1000, plusp=0),
             dict(quc=q1, chrstart=200, chrend=300, chroffset=0, chrhigh=1000, plusp=1)]
    probs, buf = gmapdp.Engine.build_scan_batch(calls)
    assert buf == q1 + q2
    assert probs["qoff"].tolist() == [0, len(q1), 0]
    assert probs["querylength"].tolist() == [len(q1), len(q2), len(q1)]
    assert probs["minor"].tolist() == [0, 0, 0]
    assert probs["chrend"].tolist() == [100, 50, 300]
