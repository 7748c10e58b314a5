"""The compact pair stream on the host (no GPU): the plain-Python reference of the format (tests/pcstream.py)
against the C expander, the expander's refusals of bad input, and the decoder under a memory checker."""
import os
import struct
import subprocess

import numpy as np
import pytest

import gmapdp
import pcstream as pc

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -1
BOTH = pytest.mark.parametrize("path", [False, True], ids=["pairs", "path_pairs"])


def _round_trip(lists, path, name):
    stream, offs = pc.encode(lists)
    n = sum(len(x) for x in lists)
    assert len(stream) <= pc.bound(n, path), "%s: %d bytes for %d records" % (name, len(stream), n)
    for i, x in enumerate(lists):
        back = pc.decode_list(stream[int(offs[i]):int(offs[i + 1])], len(x), path)
        assert back.tobytes() == x.tobytes(), "%s: the reference decoder does not restore list %d" % (name, i)
    rc, arena, want = pc.expand(stream, offs, lists, path, nthreads=2)
    assert rc == 0, "%s: gmapdp_expand refuses the reference's stream (%d)" % (name, rc)
    assert arena.tobytes() == want.tobytes(), "%s: the C expander differs (records, or the arena around them)" % name


@BOTH
def test_reference_stream_expands_to_the_records(path):
    """Every small case: encoder -> the reference decoder and the C expander, exact records, the arena outside
    the lists untouched, at most the documented bound."""
    cases = pc.small_cases(path)
    assert len(cases) > 50
    for name, lists in cases.items():
        _round_trip(lists, path, name)


@BOTH
def test_reference_random_lists_expand_to_the_records(path):
    lists = pc.random_case(path)
    _round_trip(lists, path, "random")
    # the walk does exercise what it is for
    stream, offs = pc.encode(lists)
    assert stream.count(b"\x02") > 1000 and stream.count(b"\xff") > 1000 and max(len(x) for x in lists) > 290


@BOTH
def test_reference_run_cap(path):
    """A run holds at most 65 535 records; the next record starts a run of its own."""
    for name, lists in pc.run_cap_cpu_cases(path).items():
        _round_trip(lists, path, name)
    for n, want in ((65534, [65534]), (65535, [65535]), (65536, [65535, 1]), (65537, [65535, 2]),
                    (131071, [65535, 65535, 1]), (70000, [65535, 4465])):
        s = pc.encode_list(pc.diagonal(path, n, 7, 1000))
        runs, p = [], 0
        while p < len(s):
            assert s[p] == 1
            q, g, dq, dg, ln = struct.unpack("<iibbH", s[p + 1:p + 13])
            assert (q, g) == (7 + sum(runs), 1000 + sum(runs)) and (dq, dg) == ((1, 1) if ln > 1 else (0, 0))
            runs.append(ln)
            p += 13 + ln
        assert runs == want, (n, runs)


def test_reference_encodes_the_hand_made_streams():
    """The encoder against streams written out by hand (the ones tests/test_capi.py decodes)."""
    def run(q, g, dq, dg, n):
        return b"\x01" + struct.pack("<iibbH", q, g, dq, dg, n)
    recs = pc.cat(pc.records(False, [10, 11, 12], [100, 101, 102], [b"A*AA", b"C GG", b"n- N"]),
                  pc.records(False, [13, 14], [103, 103], [b"A- A", b"C- C"]),
                  pc.records(False, [-1], [-1], b" > .", jump=250))
    want = run(10, 100, 1, 1, 4) + bytes([0 | 0 << 2 | 0 << 4, 1 | 2 << 2 | 2 << 4]) + b"\xffn- N" + b"\xffA- A"
    want += run(14, 103, 0, 0, 1) + b"\xffC- C" + b"\x02" + struct.pack("<iii", -1, -1, 250) + b" > ."
    # (13,103) continues the diagonal; (14,103) changes step, so it starts a run of one record
    assert pc.encode_list(recs) == want
    precs = pc.cat(pc.records(True, [0, 1, 2], [500, 501, 502], [b"A|AA", b"C|CC", b"G|GG"]),
                   pc.records(True, [-1], [-1], b" - .", jump=7, gjump=130))
    pwant = run(0, 500, 1, 1, 3) + bytes([0 | 0 << 2 | 1 << 4, 1 | 1 << 2 | 1 << 4, 2 | 2 << 2 | 1 << 4])
    pwant += b"\x02" + struct.pack("<iiii", -1, -1, 7, 130) + b" - ."
    assert pc.encode_list(precs) == pwant


def test_worst_case_list_needs_18_bytes_per_record():
    """A list whose step alternates and whose characters need the escape: 13 + 5 B for every record but the
    first two; gmapdp_compact_bound covers it, for one record and for many."""
    lib = gmapdp.load_library()
    for n in (1, 2, 3, 77, 78, 1000):
        size = len(pc.encode_list(pc.alternating(False, n)))
        assert size == (18 * n - 13 if n > 1 else 18)
        assert size <= lib.gmapdp_compact_bound(n, 0) == pc.bound(n, False)
        psize = len(pc.encode_list(pc.records(True, [-1] * n, [-1] * n, b" - .", jump=1)))
        assert psize == 21 * n <= lib.gmapdp_compact_bound(n, 1) == pc.bound(n, True)


def _small(path):
    """A small valid case: two lists, RUNs with coded and escaped records, a RAW record."""
    a = pc.cat(pc.diagonal(path, 4, 10, 100, chars=[b"A|AA", b"C GT", b"n|N.", b"T|TT"]), pc.gapholder(path),
               pc.diagonal(path, 2, 40, 900, (1, 0), [b"G-GG", b"A*CC"]))
    b = pc.diagonal(path, 3, 5, 6, (0, 1))
    return [a, b]


def _refused(stream, offs, lists, path, **kw):
    rc, arena, want = pc.expand(stream, offs, lists, path, **kw)
    return rc == EINVAL


@BOTH
def test_expand_refuses_every_proper_prefix(path):
    lists = _small(path)
    stream, offs = pc.encode(lists)
    assert pc.expand(stream, offs, lists, path)[0] == 0
    a = int(offs[1])
    for k in range(a):          # list 0 cut short (list 1 whole, after it)
        cut = stream[:k] + stream[a:]
        assert _refused(cut, [0, k, k + len(stream) - a], lists, path), "prefix of %d bytes" % k
        with pytest.raises(pc.StreamError):
            pc.decode_list(stream[:k], len(lists[0]), path)
    for k in range(a, len(stream)):   # the last list cut short: the stream ends there
        assert _refused(stream[:k], [0, a, k], lists, path), "prefix of %d bytes" % k


@BOTH
def test_expand_refuses_malformed_streams(path):
    lists = _small(path)
    stream, offs = pc.encode(lists)
    a = int(offs[1])
    raw_at = 13 + 1 + 5 + 5 + 1         # list 0: a RUN of 4 (two of them escaped), then the RAW record
    assert stream[0] == 1 and stream[11:13] == b"\x04\x00" and stream[raw_at] == 2

    def with_bytes(at, new):
        return stream[:at] + new + stream[at + len(new):]
    bad = {
        "RUN length 0": with_bytes(11, b"\x00\x00"),
        "RUN length larger than the list": with_bytes(11, b"\x08\x00"),
        "RUN length larger than its codes": with_bytes(11, b"\x05\x00"),
        "unknown op 0x00": with_bytes(0, b"\x00"),
        "unknown op 0x03": with_bytes(raw_at, b"\x03"),
        "unknown op 0xff": with_bytes(0, b"\xff"),
        "a code with high bits": with_bytes(13, b"\x40"),
    }
    for name, s in bad.items():
        assert _refused(s, offs, lists, path), name
        with pytest.raises(pc.StreamError):
            pc.decode_list(s[:a], len(lists[0]), path)
    # a RUN that claims more records than the list, with the bytes to go with it
    longer = pc.encode_list(pc.diagonal(path, 5))
    assert _refused(longer, [0, len(longer)], [pc.diagonal(path, 4)], path)
    # trailing bytes after a list's last record
    for extra in (b"\x00", b"\x15", b"\x01", b"\x02" + bytes(lists[0].dtype.itemsize)):
        s = stream[:a] + extra + stream[a:]
        assert _refused(s, [0, a + len(extra), len(s)], lists, path), "trailing %r" % extra
        with pytest.raises(pc.StreamError):
            pc.decode_list(stream[:a] + extra, len(lists[0]), path)
    # offsets that decrease
    assert _refused(stream, [0, len(stream) + 5, len(stream)], lists, path)
    assert _refused(stream, [a, 0, len(stream)], lists, path)
    # an empty list takes no bytes; bytes for it are refused
    assert pc.expand(b"", [0, 0], [pc.diagonal(path, 0)], path)[0] == 0
    assert _refused(b"\x15", [0, 1], [pc.diagonal(path, 0)], path)


@BOTH
def test_expand_refuses_records_outside_the_arena(path):
    """pair_offset < 0 and pair_offset + npairs > capacity: GMAPDP_EINVAL, and nothing is written."""
    lists = _small(path)
    stream, offs = pc.encode(lists)
    n0, n1 = len(lists[0]), len(lists[1])
    cap = n0 + n1
    rc, arena, want = pc.expand(stream, offs, lists, path, pair_offsets=[0, n0], capacity=cap)
    assert rc == 0 and arena.tobytes() == want.tobytes()          # exactly full: accepted
    blank = bytes([pc.FILL]) * (cap * arena.dtype.itemsize)
    for po in ([-1, n0], [-n0, n0], [-2 ** 40, n0], [0, n0 + 1], [0, cap], [0, 2 ** 40], [n1 + 1, 0],
               [2 ** 62, n0], [-2 ** 63, n0]):
        # (list 1 first, so that a refusal of list 1 alone shows too; one thread: lists in order)
        rc, arena, _ = pc.expand(stream, offs, lists, path, pair_offsets=po, capacity=cap)
        assert rc == EINVAL, po
        bad_first = po[0] < 0 or po[0] + n0 > cap
        if bad_first:
            assert arena.tobytes() == blank, "records written for offsets %r" % (po,)
    # a list of no records may sit anywhere
    assert pc.expand(b"", [0, 0], [pc.diagonal(path, 0)], path, pair_offsets=[-5], capacity=1)[0] == 0
    # the Python wrappers pass their capacity through
    with pytest.raises(gmapdp.GmapdpError):
        if path:
            p = np.zeros(2, dtype=gmapdp.PATH_DTYPE)
            p["pair_offset"], p["npairs"] = [0, n0], [n0, n1]
            gmapdp.expand_path_pairs(np.frombuffer(stream, dtype=np.uint8), offs, p, cap - 1)
        else:
            gmapdp.expand_pairs(np.frombuffer(stream, dtype=np.uint8), offs, [n0, n1], [0, n0], cap - 1)


def test_decoder_under_address_and_undefined_sanitizers(tmp_path):
    """tests/pc_expand_check.cpp (host code only: csrc/pc_expand.h and include/gmapdp.h) built with
    -fsanitize=address,undefined and run as a child process over the small cases of both record types: the
    whole stream, every prefix and single-byte corruptions, in exactly sized heap buffers."""
    blob = bytearray()
    ncases = 0
    for path in (False, True):
        cases = dict(pc.small_cases(path))
        cases["small"] = _small(path)
        cases["random"] = pc.random_case(path)[:40]
        for lists in cases.values():
            for x in lists:
                s = pc.encode_list(x)
                blob += struct.pack("<BII", int(path), len(x), len(s)) + x.tobytes() + s
                ncases += 1
    casefile = tmp_path / "cases.bin"
    casefile.write_bytes(b"PCX1" + struct.pack("<I", ncases) + bytes(blob))
    exe = tmp_path / "pc_expand_check"
    # (the sanitizers' runtimes linked in, so that the program depends on no library order at start-up)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", os.path.join(HERE, "pc_expand_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), str(casefile)], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("%d cases" % ncases), r.stdout
