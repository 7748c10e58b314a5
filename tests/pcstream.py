"""The compact pair stream as a unit of its own: a plain-Python reference of the format (pc_kernel.hip's
header comment, one list at a time), the case lists shared by the CPU and GPU tests, and a driver that runs
the shipped kernel (gmapdp_compact_pairs / gmapdp_compact_path_pairs) on caller-made lists.

A list is a numpy array of gmapdp.PAIR_DTYPE (DP pairs, 16 B) or gmapdp.PATH_PAIR_DTYPE (stage 2's path
pairs, 20 B) records; a case is a list of such lists, one stream list each."""
import ctypes as C
import functools
import random
import struct

import numpy as np

import gmapdp

MAX_RUN = 65535          # records per RUN (its length is a uint16); the next record starts a run of its own
HEADER = 13
INT32_MAX = 2 ** 31 - 1
NT = b"ACGT"
COMP = b"*| :"


def dtype_of(path):
    return gmapdp.PATH_PAIR_DTYPE if path else gmapdp.PAIR_DTYPE


def bound(nrecords, path):
    """The documented bound: 18 B per DP pair, 21 B per path pair, + 64."""
    return (21 if path else 18) * nrecords + 64


# ---- the reference encoder and decoder ----

def _fields(recs):
    """(querypos, genomepos, has a jump, the four characters) of every record, as Python lists."""
    path = recs.dtype == gmapdp.PATH_PAIR_DTYPE
    q = recs["querypos"].tolist()
    g = recs["genomepos"].tolist()
    if path:
        jump = [a != 0 or b != 0 for a, b in zip(recs["queryjump"].tolist(), recs["genomejump"].tolist())]
    else:
        jump = [a != 0 for a in recs["jump"].tolist()]
    raw = recs.tobytes()
    size = recs.dtype.itemsize
    chars = [raw[i * size + size - 4:i * size + size] for i in range(len(recs))]
    return q, g, jump, chars, raw, size


def _code(ch):
    """The one-byte code of (cdna, comp, genome, genomealt), or None: escaped."""
    cdna, comp, genome, alt = ch[0:1], ch[1:2], ch[2:3], ch[3:4]
    a, b, c = NT.find(cdna), NT.find(genome), COMP.find(comp)
    if a < 0 or b < 0 or c < 0 or alt != genome:
        return None
    return a | (b << 2) | (c << 4)


def encode_list(recs):
    """One list's ops."""
    q, g, jump, chars, rawbytes, size = _fields(recs)
    n = len(q)
    raw = [jump[i] or q[i] < 0 or g[i] < 0 for i in range(n)]
    step = [None] * n
    stepok = [False] * n
    for i in range(1, n):
        step[i] = (q[i] - q[i - 1], g[i] - g[i - 1])
        stepok[i] = (not raw[i] and not raw[i - 1] and -1 <= step[i][0] <= 1 and -1 <= step[i][1] <= 1)
    cont = [False] * n
    for i in range(1, n):
        cont[i] = stepok[i] and (not stepok[i - 1] or step[i] == step[i - 1])
    out = bytearray()
    i = 0
    while i < n:
        if raw[i]:
            out += b"\x02" + rawbytes[i * size:(i + 1) * size]
            i += 1
            continue
        j = i + 1                      # the run [i, j): its continuing records, MAX_RUN at the most
        while j < n and cont[j] and j - i < MAX_RUN:
            j += 1
        dq, dg = step[i + 1] if j - i > 1 else (0, 0)
        out += b"\x01" + struct.pack("<iibbH", q[i], g[i], dq, dg, j - i)
        for k in range(i, j):
            c = _code(chars[k])
            out += b"\xff" + chars[k] if c is None else bytes((c,))
        i = j
    return bytes(out)


def encode(lists):
    """(stream bytes, offsets: the len(lists) + 1 prefix sums) of a case."""
    parts = [encode_list(x) for x in lists]
    offs = np.zeros(len(parts) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return b"".join(parts), offs


class StreamError(ValueError):
    pass


def decode_list(data, n, path):
    """One list's ops back to its n records; StreamError unless they decode to exactly n records and all of
    data."""
    dt = dtype_of(path)
    size = dt.itemsize
    out = bytearray()
    k = p = 0
    while k < n and p < len(data):
        op = data[p]
        if op == 2:
            if len(data) - p < 1 + size:
                raise StreamError("short RAW")
            out += data[p + 1:p + 1 + size]
            p += 1 + size
            k += 1
            continue
        if op != 1 or len(data) - p < HEADER:
            raise StreamError("bad op")
        q, g, dq, dg, ln = struct.unpack("<iibbH", data[p + 1:p + HEADER])
        p += HEADER
        if ln == 0 or ln > n - k:
            raise StreamError("bad RUN length")
        for r in range(ln):
            if p >= len(data):
                raise StreamError("short RUN")
            if data[p] == 0xFF:
                if len(data) - p < 5:
                    raise StreamError("short escape")
                ch = data[p + 1:p + 5]
                p += 5
            else:
                b = data[p]
                if b & 0xC0:
                    raise StreamError("bad code")
                p += 1
                ch = bytes((NT[b & 3], COMP[(b >> 4) & 3], NT[(b >> 2) & 3], NT[(b >> 2) & 3]))
            out += struct.pack("<ii", q + r * dq, g + r * dg) + bytes(size - 12) + ch
        k += ln
    if k != n or p != len(data):
        raise StreamError("records or bytes left over")
    return np.frombuffer(bytes(out), dtype=dt).copy()


# ---- making lists ----

def records(path, q, g, chars=b"A|AA", jump=0, gjump=0):
    """A list from positions (sequences of equal length), one 4-character string for all records or one per
    record (cdna, comp, genome, genomealt), and the jump(s) (a scalar or one per record)."""
    n = len(q)
    r = np.zeros(n, dtype=dtype_of(path))
    r["querypos"] = np.asarray(q, dtype=np.int64).astype(np.int32)
    r["genomepos"] = np.asarray(g, dtype=np.int64).astype(np.int32)
    if path:
        r["queryjump"] = jump
        r["genomejump"] = gjump
    else:
        r["jump"] = jump
    if isinstance(chars, bytes):
        chars = [chars] * n
    ch = np.frombuffer(b"".join(chars), dtype="S1").reshape(n, 4) if n else np.zeros((0, 4), dtype="S1")
    for x, name in enumerate(("cdna", "comp", "genome", "genomealt")):
        r[name] = ch[:, x]
    return r


def walk(path, steps, q0=100, g0=5000, chars=b"A|AA"):
    """len(steps) + 1 records: (q0, g0), then one (dq, dg) step each."""
    q, g = [q0], [g0]
    for dq, dg in steps:
        q.append(q[-1] + dq)
        g.append(g[-1] + dg)
    return records(path, q, g, chars)


def diagonal(path, n, q0=100, g0=5000, step=(1, 1), chars=b"A|AA"):
    k = np.arange(n, dtype=np.int64)
    return records(path, q0 + k * step[0], g0 + k * step[1], chars)


def gapholder(path, jump=7, gjump=130):
    """A gap holder: positions -1, its jump(s)."""
    return records(path, [-1], [-1], b" - .", jump=jump, gjump=gjump)


def cat(*parts):
    return np.concatenate(parts)


MIXED = [b"A|AA", b"C|CC", b"G GT", b"T*TT", b"A:GG", b"n|N.", b"C-CC", b"G|GA"]


def mixed_chars(n, at=0):
    return [MIXED[(at + i) % len(MIXED)] for i in range(n)]


def alternating(path, n, chars=b"a|AA"):
    """The costliest list: the step changes at every record (each record from the third on starts a run)
    and every record's characters need the escape."""
    return walk(path, [((1, 0), (1, 1))[i % 2] for i in range(n - 1)], chars=chars) if n else diagonal(path, 0)


# ---- the cases (name -> list of lists); the CPU tests and the GPU tests run the same ones ----

def length_cases(path):
    return {"len%d" % n: [diagonal(path, n, chars=mixed_chars(n))] for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 192)}


def boundary_cases(path):
    d = lambda n, q0=100, g0=5000, step=(1, 1): diagonal(path, n, q0, g0, step, mixed_chars(n, q0))  # noqa: E731
    c = {
        "start63_continues": [cat(d(63), d(20, 400, 7000))],
        "start63_alone": [cat(d(63), d(1, 400, 7000), d(20, 800, 9000))],
        "start63_last": [cat(d(63), d(1, 400, 7000))],
        "raw63": [cat(d(63), gapholder(path), d(16, 400, 7000))],
        "raw63_jumpless": [cat(d(63), records(path, [-1], [3], b"A|AA"), d(16, 400, 7000))],
        "raw64": [cat(d(64), gapholder(path), d(15, 400, 7000))],
        "closed_by_lane0_jump": [cat(d(64), d(10, 400, 7000))],
        "closed_by_lane0_step": [cat(d(64), d(10, 164, 5063, (1, 0)))],
        "one_record_run_carried_new_step": [cat(d(63), d(12, 400, 7000, (1, 0)))],
        "one_record_run_carried_closed": [cat(d(63), d(1, 400, 7000), d(5, 402, 7000))],
        "two_raw_across_edge": [cat(d(63), gapholder(path), gapholder(path, 9, 0), d(3, 400, 7000))],
    }
    for steps in (3, 4):
        n = 64 * steps
        c["open_%d_steps_list_ends" % steps] = [d(n)]
        c["open_%d_steps_closed_at_edge" % steps] = [cat(d(n), d(5, 900, 9000))]
        c["open_%d_steps_list_ends_one_past" % steps] = [d(n + 1)]
        c["open_%d_steps_closed_one_past" % steps] = [cat(d(n + 1), d(5, 900, 9000))]
        c["open_%d_steps_from_lane5" % steps] = [cat(d(5, 10, 20), d(n - 5), gapholder(path))]
    return c


def step_cases(path):
    nine = [(dq, dg) for dq in (-1, 0, 1) for dg in (-1, 0, 1)]
    c = {"step_%+d_%+d" % s: [diagonal(path, 7, 50, 60, s, mixed_chars(7)), diagonal(path, 70, 500, 600, s)]
         for s in nine}
    c["step_changes_every_record"] = [walk(path, [nine[(5 * i) % 9] for i in range(150)], 400, 400, mixed_chars(151))]
    c["step_changes_every_second"] = [walk(path, [nine[(2 * (i // 2)) % 9] for i in range(150)], 400, 400)]
    c["alternating_1_0_and_1_1"] = [alternating(path, 130, b"A|AA")]
    c["deltas_of_2"] = [walk(path, [(1, 1), (2, 1), (1, 1), (1, 2), (1, 1), (-2, 0), (0, -2), (0, 0), (2, 2), (-2, -2),
                                    (1, 1), (1, 1), (1, -2), (-1, -1), (-1, -1)], 300, 300, mixed_chars(16))]
    c["up_to_int32_max"] = [diagonal(path, 100, INT32_MAX - 100, INT32_MAX - 100),
                            diagonal(path, 70, INT32_MAX, INT32_MAX, (-1, -1)),
                            diagonal(path, 66, INT32_MAX - 65, 0, (1, 0))]
    c["genomepos_0"] = [diagonal(path, 10, 0, 0, (1, 0)), diagonal(path, 5, 4, 4, (-1, -1)),
                        cat(diagonal(path, 4, 10, 3, (1, -1)), records(path, [14, 15], [-1, -2]),
                            diagonal(path, 3, 16, 0))]
    return c


def char_cases(path):
    codes = [bytes((NT[a], COMP[cp], NT[b], NT[b])) for cp in range(4) for b in range(4) for a in range(4)]
    c = {"all_64_codes": [diagonal(path, 64, chars=codes), diagonal(path, 64, 9, 9, (0, 1), codes[::-1])]}
    for name, ch in (("lowercase_cdna", b"a|AA"), ("n_cdna", b"N GG"), ("n_genome", b"A NN"),
                     ("lowercase_genome", b"C cc"), ("comp_dash", b"A-AA"), ("comp_gt", b"A>AA"),
                     ("genomealt_differs", b"A|AC"), ("nul_characters", b"\0\0\0\0"),
                     ("ff_characters", b"\xff\xff\xff\xff")):
        c["escape_" + name] = [diagonal(path, 1, chars=ch),
                               diagonal(path, 9, chars=[ch if i in (0, 4, 8) else b"T|TT" for i in range(9)]),
                               diagonal(path, 70, chars=[ch if i in (62, 63, 64) else b"G GG" for i in range(70)])]
    return c


def worst_case(path):
    """One list of escaped records whose step alternates, filling the whole arena."""
    return {"worst_256": [alternating(path, 256)]}


def run_cap_cases(path):
    """Runs around the cap, one launch."""
    return {"run_cap": [diagonal(path, n, 7, 1000) for n in (65534, 65535, 65536, 65537, 131071)] +
            [diagonal(path, 70000, 3, 12345, (1, 0), b"c-CC")]}


def run_cap_cpu_cases(path):
    """The same for the host tests, and a run of exactly two caps with a tail after it."""
    c = run_cap_cases(path)
    c["run_cap_then_more"] = [cat(diagonal(path, 2 * MAX_RUN + 1, 0, 0), gapholder(path), diagonal(path, 3, 9, 9))]
    return c


@functools.lru_cache(maxsize=None)
def random_case(path, seed=20240611, nlists=2500):
    """Lists of 0-300 records from a persistent random walk over the nine steps, with a few percent each of
    RAW records, position jumps and escaped characters."""
    rng = random.Random(seed + (1 if path else 0))
    nine = [(dq, dg) for dq in (-1, 0, 1) for dg in (-1, 0, 1)]
    plain = [bytes((NT[a], COMP[cp], NT[b], NT[b])) for cp in range(4) for b in range(4) for a in range(4)]
    odd = [b"a|AA", b"N NN", b"A-AA", b"A|AC", b"c c.", b"T~TT"]
    lists = []
    for _ in range(nlists):
        n = rng.choice((0, 1, 2, 63, 64, 65)) if rng.random() < 0.1 else rng.randint(0, 300)
        q, g, jq, jg, ch = [], [], [], [], []
        cq, cg, st = rng.randint(0, 5000), rng.randint(0, 10 ** 6), rng.choice(nine)
        keep = rng.choice((0.5, 0.9, 0.98))          # how persistent this list's walk is
        for _i in range(n):
            x = rng.random()
            if x < 0.03:                             # RAW: a gap holder, or a record with a jump in place
                holder = rng.random() < 0.5
                q.append(-1 if holder else cq)
                g.append(-1 if holder else cg)
                jq.append(rng.randint(1, 300))
                jg.append(rng.randint(0, 300))
                ch.append(b" - .")
                continue
            if x < 0.06:                             # a position jump
                cq += rng.randint(-50, 50)
                cg += rng.randint(-3000, 3000)
            else:
                if rng.random() > keep:
                    st = rng.choice(nine)
                cq += st[0]
                cg += st[1]
            q.append(cq)                             # (a negative position goes RAW)
            g.append(cg)
            jq.append(0)
            jg.append(0)
            ch.append(rng.choice(odd) if rng.random() < 0.04 else rng.choice(plain))
        lists.append(records(path, q, g, ch, jump=jq, gjump=jg) if n else diagonal(path, 0))
    return lists


def small_cases(path):
    """Every tiny case, for the tests that take them all."""
    c = {}
    for f in (length_cases, boundary_cases, step_cases, char_cases, worst_case):
        c.update(f(path))
    return c


# ---- the host expander on a case ----

FILL = 0x5A


def expand(stream, offsets, lists, path, npairs=None, pair_offsets=None, capacity=None, gap=3, nthreads=1):
    """gmapdp_expand_pairs / gmapdp_expand_path_pairs over an arena pre-filled with FILL bytes, the lists
    `gap` records apart (or at pair_offsets, with npairs records each).  Returns (rc, the arena, the arena
    expected: the lists' records in place and FILL everywhere else)."""
    lib = gmapdp.load_library()
    dt = dtype_of(path)
    if npairs is None:
        npairs = [len(x) for x in lists]
    if pair_offsets is None:
        pair_offsets, at = [], gap
        for x in lists:
            pair_offsets.append(at)
            at += len(x) + gap
        if capacity is None:
            capacity = at
    arena = np.frombuffer(bytes([FILL]) * (dt.itemsize * max(capacity, 1)), dtype=dt).copy()
    want = arena.copy()
    for x, m, at in zip(lists, npairs, pair_offsets):
        if m > 0 and 0 <= at and at + m <= capacity:
            want[at:at + m] = x[:m]
    st = np.frombuffer(bytes(stream) + b"\0", dtype=np.uint8)[:len(stream)]
    of = np.ascontiguousarray(offsets, dtype=np.uint64)
    if path:
        pa = np.zeros(len(lists), dtype=gmapdp.PATH_DTYPE)
        pa["npairs"] = npairs
        pa["pair_offset"] = pair_offsets
        rc = lib.gmapdp_expand_path_pairs(st.ctypes.data, of.ctypes.data, len(pa), pa.ctypes.data, arena.ctypes.data,
                                          capacity, nthreads)
    else:
        npc = np.asarray(npairs, dtype=np.int32)
        po = np.asarray(pair_offsets, dtype=np.int64)
        rc = lib.gmapdp_expand_pairs(st.ctypes.data, of.ctypes.data, len(npc), npc.ctypes.data, po.ctypes.data,
                                     arena.ctypes.data, capacity, nthreads)
    return rc, arena, want


# ---- the shipped kernel on caller-made lists ----

GUARD = 64
GUARD_BYTE = 0xC3


class Device:
    """Device buffers for one run, freed on exit."""

    def __init__(self):
        self.hip = gmapdp._hip()
        self.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            self.hip.hipFree(b)

    def alloc(self, nbytes, fill=None):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(int(nbytes), 16)) == 0, "hipMalloc(%d)" % nbytes
        self.bufs.append(p)
        if fill is not None:
            assert self.hip.hipMemset(p, fill, max(int(nbytes), 16)) == 0
            self.sync()                 # (the kernels run on the engine's own stream)
        return p

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        if arr.nbytes:
            assert self.hip.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0   # host to device
        return p

    def down(self, p, nbytes, dtype=np.uint8):
        out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        if out.nbytes:
            assert self.hip.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0   # device to host
        return out

    def sync(self):
        assert self.hip.hipDeviceSynchronize() == 0, "hipDeviceSynchronize"


def _two_passes(dev, nlists, launch):
    """The sizing pass (d_out NULL), then the write pass into a buffer of the sizing pass's total plus GUARD
    bytes of GUARD_BYTE -- never sized from the bound under test.  Returns (stream, offsets, guard intact)."""
    d_off = dev.alloc(8 * (nlists + 1), fill=0xEE)
    launch(None, d_off)
    dev.sync()
    sized = dev.down(d_off, 8 * (nlists + 1), np.uint64)
    total = int(sized[-1])
    assert total < 2 ** 28, "the sizing pass reports %d bytes" % total
    d_out = dev.alloc(total + GUARD, fill=GUARD_BYTE)
    launch(d_out, d_off)
    dev.sync()
    offs = dev.down(d_off, 8 * (nlists + 1), np.uint64)
    assert np.array_equal(offs, sized), "the write pass's offsets differ from the sizing pass's"
    got = dev.down(d_out, total + GUARD)
    return got[:total].tobytes(), offs, bool(np.all(got[total:] == GUARD_BYTE))


def compact_pairs(eng, results, gresults, arena):
    """gmapdp_compact_pairs over uploaded gmapdp.RESULT_DTYPE / GENOME_RESULT_DTYPE records and a PAIR_DTYPE
    arena.  Returns (stream, offsets, guard intact)."""
    lib = eng.lib
    with Device() as dev:
        d_res = dev.up(results) if len(results) else None
        d_gres = dev.up(gresults) if len(gresults) else None
        d_pairs = dev.up(arena)

        def launch(d_out, d_off):
            eng._check(lib.gmapdp_compact_pairs(eng.h, d_res, len(results), d_gres, len(gresults), d_pairs, d_out,
                                                d_off, None), "gmapdp_compact_pairs")
        return _two_passes(dev, len(results) + len(gresults), launch)


def compact_path_pairs(eng, paths, npaths, arena, pair_cap=None):
    """gmapdp_compact_path_pairs over uploaded PATH_DTYPE records (all of them lists; the first npaths count)
    and a PATH_PAIR_DTYPE arena of pair_cap records (default: all of it)."""
    lib = eng.lib
    with Device() as dev:
        d_paths = dev.up(paths)
        d_np = dev.up(np.array([npaths], dtype=np.uint64))
        d_pairs = dev.up(arena)
        cap = len(arena) if pair_cap is None else pair_cap

        def launch(d_out, d_off):
            eng._check(lib.gmapdp_compact_path_pairs(eng.h, d_paths, d_np, len(paths), d_pairs, cap, d_out, d_off,
                                                     None), "gmapdp_compact_path_pairs")
        return _two_passes(dev, len(paths), launch)


def lay_out(lists, path, gap=3):
    """The lists `gap` filler records apart in one arena (gap = 0: the lists fill it).  Returns (arena, the
    lists' offsets)."""
    dt = dtype_of(path)
    filler = records(path, [77] * gap, [78] * gap, b"T|TT")     # would extend a diagonal if it were read
    parts, offs, at = [filler], [], gap
    for x in lists:
        offs.append(at)
        parts += [x, filler]
        at += len(x) + gap
    return np.concatenate(parts).astype(dt), offs


def run_kernel(eng, lists, path, gap=3, n0=None):
    """The case through the shipped kernel: DP lists as the first n0 gmapdp_result records and the others as
    gmapdp_genome_result records (default: half and half), path lists as gmapdp_path records.  Returns
    (stream, offsets, guard intact, the arena, the lists' offsets)."""
    arena, offs = lay_out(lists, path, gap)
    if path:
        paths = np.zeros(len(lists), dtype=gmapdp.PATH_DTYPE)
        paths["pair_offset"] = offs
        paths["npairs"] = [len(x) for x in lists]
        paths["pad_"] = -1
        return compact_path_pairs(eng, paths, len(lists), arena) + (arena, offs)
    n0 = (len(lists) + 1) // 2 if n0 is None else n0
    res = np.zeros(n0, dtype=gmapdp.RESULT_DTYPE)
    gres = np.zeros(len(lists) - n0, dtype=gmapdp.GENOME_RESULT_DTYPE)
    for r in (res, gres):               # every other field: values a wrong stride would show as a length
        for name in r.dtype.names:
            if r.dtype[name].kind == "i":
                r[name] = 1000003
    res["npairs"] = [len(x) for x in lists[:n0]]
    res["pair_offset"] = offs[:n0]
    gres["npairs"] = [len(x) for x in lists[n0:]]
    gres["pair_offset"] = offs[n0:]
    return compact_pairs(eng, res, gres, arena) + (arena, offs)


def first_difference(got, want, offs):
    """Where two streams differ, for an assertion's message."""
    if got == want:
        return "equal"
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    lst = int(np.searchsorted(np.asarray(offs, dtype=np.uint64), at, side="right")) - 1
    return "lengths %d / %d, first difference at byte %d (list %d, its byte %d): got %s, reference %s" % (
        len(got), len(want), at, lst, at - int(offs[max(lst, 0)]), got[at:at + 20].hex(), want[at:at + 20].hex())
