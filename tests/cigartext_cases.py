"""A case table for the CIGAR text parser (svim_asm_amd/csrc/svx_cigartext.hip: k_count, k_scan, k_rec_rank, k_rec_fin,
k_emit): operator bytes, numbers and record boundaries against the edges of a chunk (1024 bytes, one workgroup), a step
(256 bytes, one byte per lane) and a wave (64 lanes); the two ways k_emit adds up ref_len; empty and `*` records at every
place a binary search among rec_off can go wrong; the carried scan at 1023 | 1024 | 1025 chunks and records; numbers at
the limit of 2^28 and digit runs longer than a chunk; every byte value; which of two errors of one record decides.
tests/test_cigartext_cases.py holds the table to its own preconditions where there is no GPU and runs the host parser
over it, tests/test_gpu_cigartext_cases.py runs it on the device.

Cases.  A case is a list of record texts (bytes), built from a description and seeded by its name (`Layout` places a
record at a byte offset and fills the gap with good records; `good` writes a good record of an exact length).  The
builders lay the cases out with the numbers of LAID, a frozen copy of K; the classes are judged with the `k` they are
given, so a constant moved in K alone moves the classes off the cases.

Expected results come from tests/sam_text_writer.parse_batch alone (`expected`), never from the host or the device
parser.

Facts.  facts(text, rec_off, k) computes from the two arrays and the constants alone, calling no parser: the chunk
count; per chunk, step and wave the records it touches (as k_emit's two searches see them: the LAST record whose offset
is at or in front of a byte holds it) and its operator bytes; per operator byte its residues and those of the first
digit of its number; per record where it starts and ends in those units.

Classes.  CLASSES names every situation the table has to show; a case lists the classes it shows.  check_preconditions
holds every case to its list and every class to at least one case.  EXEMPT names the classes that no text can show."""
import collections
import functools
import types
import zlib

import numpy as np

from tests import sam_text_writer as stw

# The constants of svx_cigartext.hip, as literals (the one place the table can be moved from).  CHUNK: kChunk, bytes per
# workgroup of k_count and k_emit; GROUP: kThreads, bytes per step; WAVE: lanes of a wave; SCAN: kScanThreads, entries
# per tile of k_scan; RANK_PER_GROUP: record boundaries per workgroup of k_rec_rank (kWaves); FIN_PER_GROUP: records per
# workgroup of k_rec_fin (kThreads); LIMIT: the least length that is refused; EXACT_DIGITS: the digits number_before
# adds up exactly.
K = dict(CHUNK=1024, GROUP=256, WAVE=64, SCAN=1024, RANK_PER_GROUP=4, FIN_PER_GROUP=256, LIMIT=1 << 28, EXACT_DIGITS=10)
LAID = types.MappingProxyType(dict(K))
UNITS = (("chunk", "CHUNK", None), ("step", "GROUP", "CHUNK"), ("wave", "WAVE", "GROUP"))   # name, constant, the unit above
CODES = ("OK", "BAD_CHAR", "BAD_OP", "EMPTY_NUMBER", "NUMBER_TOO_BIG", "TRAILING_DIGITS")
ERRORS = CODES[1:]
DISTANCES = ("same_wave", "waves_of_one_chunk", "adjacent_chunks", "two_chunks_apart")
REF_OPS, NOREF_OPS, ALL_OPS = b"MDN=X", b"ISHP", b"MIDNSHP=X"

Case = collections.namedtuple("Case", "name family texts text rec_off shows marks")


def _ceil(a, b):
    return -(-a // b)


def batch(texts):
    """texts -> (text as uint8 array, rec_off as int64 array), both read-only."""
    text = np.frombuffer(b"".join(texts), np.uint8)
    off = np.zeros(len(texts) + 1, np.int64)
    if texts:
        np.cumsum([len(t) for t in texts], out=off[1:])
    off.setflags(write=False)
    return text, off


# --------------------------------------------------------------------------------------------------------- facts
def facts(text, rec_off, k=None):
    """Every quantity of the module docstring, from `text`, `rec_off` and the constants `k` alone."""
    k = k or K
    text, rec_off = np.asarray(text, np.uint8), np.asarray(rec_off, np.int64)
    n, n_rec = len(text), len(rec_off) - 1
    F = types.SimpleNamespace(text=text, rec_off=rec_off, n_bytes=n, n_rec=n_rec, n_chunks=_ceil(n, k["CHUNK"]) if n_rec else 0)
    digit = (text >= 48) & (text <= 57)
    F.digit = digit
    F.ops = np.nonzero(~digit & (text != 42))[0]                   # neither a digit nor '*'
    F.rec_start, F.rec_end = rec_off[:-1], rec_off[1:]
    F.rec_len = F.rec_end - F.rec_start

    def rec_of(p):                                                 # the last r with rec_off[r] <= p
        return np.searchsorted(rec_off, p, side="right") - 1
    F.rec_of = rec_of
    F.op_rec = rec_of(F.ops)
    # the first digit of the number in front of an operator byte: behind the nearest byte in front of it that is no
    # digit, not in front of the record's start
    at = np.where(~digit, np.arange(n), -1)
    last_other = np.maximum.accumulate(at) if n else at
    before = np.where(F.ops > 0, last_other[np.maximum(F.ops - 1, 0)], -1)
    F.num_start = np.maximum(before + 1, F.rec_start[F.op_rec]) if len(F.ops) else np.zeros(0, np.int64)
    F.n_digits = F.ops - F.num_start
    F.first_op_of = np.searchsorted(F.ops, rec_off)                # ops of record r: ops[first_op_of[r]:first_op_of[r + 1]]
    F.unit = {}
    for name, key, _ in UNITS:
        u = k[key]
        nu = _ceil(n, u)
        first = np.arange(nu, dtype=np.int64) * u
        last = np.minimum(first + u - 1, n - 1)
        F.unit[name] = types.SimpleNamespace(
            size=u, n=nu, first=first, last=last, full=first + u <= n, op_count=np.bincount(F.ops // u, minlength=nu),
            r_first=rec_of(first), r_last=rec_of(last), op_res=F.ops % u, num_res=F.num_start % u,
            rec_first=F.rec_start // u, rec_last=np.where(F.rec_len > 0, (F.rec_end - 1) // u, -1))
    F.empty = F.rec_len == 0
    F.star = (F.rec_len == 1) & (text[np.minimum(F.rec_start, max(n - 1, 0))] == 42) if n else np.zeros(n_rec, bool)
    F.real = ~F.empty & ~F.star
    return F


def number_text(F, i):
    """The digits in front of operator byte i, as bytes."""
    return F.text[F.num_start[i]:F.ops[i]].tobytes()


def ops_of(F, r):
    return F.text[F.ops[F.first_op_of[r]:F.first_op_of[r + 1]]]


def ref_sum(F, r):
    """What a record's M, D, N, = and X lengths add up to, unwrapped."""
    return sum(int(number_text(F, i)) for i in range(F.first_op_of[r], F.first_op_of[r + 1]) if F.text[F.ops[i]] in REF_OPS)


def expected(texts):
    """The oracle's answer as arrays: status, n_ops, cigar_off, ref_len, words."""
    e = stw.parse_batch(list(texts))
    E = types.SimpleNamespace(status=np.asarray(e["status"], np.int64), cigar_off=np.asarray(e["cigar_off"], np.int64),
                              ref_len=np.asarray(e["ref_len"], np.int64), words=np.asarray(e["words"], np.int64))
    E.n_ops = np.diff(E.cigar_off)
    E.good = E.status == 0
    for a in vars(E).values():
        a.setflags(write=False)
    return E


# ------------------------------------------------------------------------------------------------------- classes
def _proper(edge, k, above):
    """An edge of a unit that is not an edge of the unit above as well."""
    return edge % k[above] != 0 if above else np.ones(np.shape(edge), bool)


def _edge_classes(add):
    for name, key, above in UNITS:
        def op_last(F, E, k, c, key=key, above=above):
            u, p = k[key], F.ops
            return bool(((p % u == u - 1) & (p + 1 < F.n_bytes) & (F.n_digits >= 1) & (F.num_start // u == p // u)
                         & E.good[F.op_rec] & _proper(p + 1, k, above)).any())

        def op_first(F, E, k, c, key=key, above=above):
            u, p = k[key], F.ops
            return bool(((p % u == 0) & (p > 0) & (F.n_digits >= 1) & (F.num_start >= p - u) & E.good[F.op_rec] & _proper(p, k, above)).any())

        def straddles(F, E, k, c, key=key, above=above):
            u, p = k[key], F.ops
            e = (F.num_start // u + 1) * u                         # digits at e - 1 and at e
            return bool(((F.n_digits >= 2) & (e <= p - 1) & (F.n_digits < 20) & E.good[F.op_rec] & _proper(e, k, above)).any())

        def boundary(F, E, k, c, shift, key=key, above=above):
            u = k[key]
            if F.n_rec < 2:
                return False
            b = F.rec_off[1:-1]
            both = (F.real & E.good)[:-1] & (F.real & E.good)[1:]
            edge = b - shift
            return bool((both & (edge > 0) & (edge % u == 0) & _proper(edge, k, above)).any())
        add("edge.%s.operator_last_byte" % name, op_last)
        add("edge.%s.operator_first_byte" % name, op_first)
        add("edge.%s.number_straddles" % name, straddles)
        add("edge.%s.record_boundary_on" % name, lambda F, E, k, c, b=boundary: b(F, E, k, c, 0))
        add("edge.%s.record_boundary_one_before" % name, lambda F, E, k, c, b=boundary: b(F, E, k, c, -1))
        add("edge.%s.record_boundary_one_behind" % name, lambda F, E, k, c, b=boundary: b(F, E, k, c, 1))


SIZES = collections.OrderedDict([
    ("1", lambda k: 1), ("wave-1", lambda k: k["WAVE"] - 1), ("wave", lambda k: k["WAVE"]), ("wave+1", lambda k: k["WAVE"] + 1),
    ("step-1", lambda k: k["GROUP"] - 1), ("step", lambda k: k["GROUP"]), ("step+1", lambda k: k["GROUP"] + 1),
    ("chunk-1", lambda k: k["CHUNK"] - 1), ("chunk", lambda k: k["CHUNK"]), ("chunk+1", lambda k: k["CHUNK"] + 1),
    ("2chunks", lambda k: 2 * k["CHUNK"]), ("2chunks+1", lambda k: 2 * k["CHUNK"] + 1)])
ONLY_EMPTY = collections.OrderedDict([
    ("1", lambda k: 1), ("rank_group-1", lambda k: k["RANK_PER_GROUP"] - 1), ("rank_group", lambda k: k["RANK_PER_GROUP"]),
    ("rank_group+1", lambda k: k["RANK_PER_GROUP"] + 1), ("fin_group-1", lambda k: k["FIN_PER_GROUP"] - 1),
    ("fin_group", lambda k: k["FIN_PER_GROUP"]), ("fin_group+1", lambda k: k["FIN_PER_GROUP"] + 1),
    ("scan", lambda k: k["SCAN"]), ("scan+1", lambda k: k["SCAN"] + 1)])
COUNTS = collections.OrderedDict([
    ("scan-1", lambda k: k["SCAN"] - 1), ("scan", lambda k: k["SCAN"]), ("scan+1", lambda k: k["SCAN"] + 1),
    ("2scans", lambda k: 2 * k["SCAN"]), ("2scans+1", lambda k: 2 * k["SCAN"] + 1)])
VALUES = collections.OrderedDict([
    ("0", lambda k: 0), ("1", lambda k: 1), ("limit-1", lambda k: k["LIMIT"] - 1), ("limit", lambda k: k["LIMIT"]),
    ("limit+1", lambda k: k["LIMIT"] + 1), ("999999999", lambda k: 999999999), ("1000000000", lambda k: 1000000000),
    ("2^32-1", lambda k: 4294967295), ("2^32", lambda k: 4294967296), ("9999999999", lambda k: 9999999999),
    ("10000000000", lambda k: 10000000000), ("21_digits", lambda k: 123456789012345678901)])
ZEROS = (1, 2, 10, 11, 1100)


def _wave_classes(add):
    def waves(F, k):
        return F.unit["wave"]

    def inside(F, E, k, c, letters, good):
        W = waves(F, k)
        for w in np.nonzero(W.full & (W.r_first == W.r_last) & (W.op_count > 0))[0]:
            r = W.r_first[w]
            if bool(E.good[r]) != good or F.rec_start[r] > W.first[w] or F.rec_end[r] < W.first[w] + W.size:
                continue
            mine = F.text[F.ops[(F.ops >= W.first[w]) & (F.ops <= W.last[w])]]
            if good and all(x in letters for x in ops_of(F, r)):
                return True
            if not good and any(x in REF_OPS for x in mine):       # lengths that would count if the record were good
                return True
        return False
    add("wave.inside_one_good_record_of_MDN=X", lambda F, E, k, c: inside(F, E, k, c, REF_OPS, True))
    add("wave.inside_one_good_record_of_ISHP", lambda F, E, k, c: inside(F, E, k, c, NOREF_OPS, True))
    add("wave.inside_one_error_record", lambda F, E, k, c: inside(F, E, k, c, None, False))

    def spans(F, E, k, c, n_records):
        W = waves(F, k)
        for w in np.nonzero(W.full & (W.r_last - W.r_first + 1 == n_records))[0]:
            rs = slice(W.r_first[w], W.r_last[w] + 1)
            if F.real[rs].all() and E.good[rs].all():
                return True
        return False
    for m in (2, 3, 32):
        add("wave.over_%d_records" % m, lambda F, E, k, c, m=m: spans(F, E, k, c, m))

    def lone_lane(F, E, k, c, last):
        W = waves(F, k)
        for w in np.nonzero(W.full & (W.r_last == W.r_first + 1))[0]:
            a, b = W.r_first[w], W.r_last[w]
            cut = W.first[w] + (W.size - 1 if last else 1)
            if F.rec_start[b] == cut and F.rec_start[a] <= W.first[w] and F.rec_end[b] > W.last[w] - (0 if last else 1) and \
                    E.good[a] and E.good[b] and F.real[a] and F.real[b]:
                return True
        return False
    add("wave.last_lane_in_the_next_record", lambda F, E, k, c: lone_lane(F, E, k, c, True))
    add("wave.first_lane_in_the_record_before", lambda F, E, k, c: lone_lane(F, E, k, c, False))

    def error_between(F, E, k, c):
        W = waves(F, k)
        for w in np.nonzero(W.full & (W.r_last - W.r_first == 2))[0]:
            a = W.r_first[w]
            if E.good[a] and not E.good[a + 1] and E.good[a + 2] and F.real[a:a + 3].all():
                recs = F.op_rec[(F.ops >= W.first[w]) & (F.ops <= W.last[w])]
                if set(recs.tolist()) == {a, a + 1, a + 2}:
                    return True
        return False
    add("wave.error_record_between_two_good_ones", error_between)

    def empties(F, E, k, c, m):
        W = waves(F, k)
        for w in np.nonzero(W.full & (W.r_last - W.r_first - 1 == m))[0]:
            a, b = W.r_first[w], W.r_last[w]
            if F.empty[a + 1:b].all() and F.real[a] and F.real[b] and E.good[a] and E.good[b] and W.first[w] < F.rec_start[b] <= W.last[w]:
                return True
        return False
    for m in (1, 2, 65):
        add("wave.%d_empty_records_between_two_lanes" % m, lambda F, E, k, c, m=m: empties(F, E, k, c, m))

    def long_sum(F, E, k, c, lo, hi):
        W = waves(F, k)
        for r in np.nonzero(E.good & F.real & (W.rec_last - W.rec_first >= 2))[0]:
            if lo <= ref_sum(F, r) < hi:
                return True
        return False
    add("wave.ref_len_passes_2^31", lambda F, E, k, c: long_sum(F, E, k, c, 1 << 31, 1 << 32))
    add("wave.ref_len_passes_2^32", lambda F, E, k, c: long_sum(F, E, k, c, 1 << 32, 1 << 40))


def _record_classes(add):
    for kind in ("empty", "star"):
        def is_kind(F, kind=kind):
            return F.empty if kind == "empty" else F.star

        def first(F, E, k, c, is_kind=is_kind):
            return F.n_rec > 1 and bool(is_kind(F)[0] and F.real[1] and E.good[1])

        def last(F, E, k, c, multiple, is_kind=is_kind):
            return F.n_rec > 1 and F.n_bytes > 0 and bool(is_kind(F)[-1] and F.real[-2] and E.good[-2]) and \
                (F.n_bytes % k["CHUNK"] == 0) == multiple

        def run(F, E, k, c, m, is_kind=is_kind, kind=kind):
            kd = is_kind(F)
            for r0 in np.nonzero(kd[1:] & ~kd[:-1])[0] + 1:
                r1 = r0
                while r1 < F.n_rec and kd[r1]:
                    r1 += 1
                if r1 - r0 != m or r1 >= F.n_rec or not (F.real[r0 - 1] and F.real[r1] and E.good[r0 - 1] and E.good[r1]):
                    continue
                a, b = F.rec_start[r0], F.rec_end[r1 - 1]         # the run's bytes [a, b)
                if kind == "empty":
                    if a > 0 and a % k["CHUNK"] == 0:
                        return True
                else:
                    e = _ceil(a + 1, k["CHUNK"]) * k["CHUNK"]      # the first edge behind the run's first byte
                    if (m == 1 and (a % k["CHUNK"] == 0 and a > 0 or e == b)) or (m > 1 and e < b):
                        return True
            return False
        add("records.%s.first" % kind, first)
        add("records.%s.last.text_of_whole_chunks" % kind, lambda F, E, k, c, f=last: f(F, E, k, c, True))
        add("records.%s.last.text_ends_inside_a_chunk" % kind, lambda F, E, k, c, f=last: f(F, E, k, c, False))
        for m in (1, 2, 65):
            add("records.%s.run_of_%d_on_a_chunk_edge" % (kind, m), lambda F, E, k, c, f=run, m=m: f(F, E, k, c, m))
    for name, value in ONLY_EMPTY.items():
        add("records.only_empty.%s" % name, lambda F, E, k, c, v=value: F.n_bytes == 0 and F.n_rec == v(k))

    def count(F, E, k, c, value):
        s = k["SCAN"]
        if F.n_rec != value(k):
            return False
        tiles_have_errors = all((~E.good[t:t + s]).any() for t in range(0, F.n_rec, s))
        inner = range(s, F.n_rec, s)
        return tiles_have_errors and all(E.n_ops[m - 1] != E.n_ops[m] and not (E.good[m - 1] and E.good[m]) for m in inner) and \
            len(set(E.n_ops.tolist())) >= 5
    for name, value in COUNTS.items():
        add("records.count.%s" % name, lambda F, E, k, c, v=value: count(F, E, k, c, v))

    def chunks(F, E, k, c, value):
        s, C = k["SCAN"], F.unit["chunk"]
        if F.n_chunks != value(k) or (F.n_chunks % s == 0 and F.n_bytes != F.n_chunks * k["CHUNK"]):
            return False
        inner = range(s, F.n_chunks, s)
        starts = set((F.rec_start[F.real] // k["CHUNK"]).tolist())
        differ = int((C.op_count[1:] != C.op_count[:-1]).sum())
        return all(C.op_count[m - 1] != C.op_count[m] and m in starts for m in inner) and differ >= F.n_chunks // 2 and \
            len(set(C.op_count.tolist())) >= 5 and bool((~E.good).any())
    for name, value in list(COUNTS.items())[:3]:
        add("chunks.count.%s" % name, lambda F, E, k, c, v=value: chunks(F, E, k, c, v))


def _number_classes(add):
    def numbers(F):
        if not hasattr(F, "numbers"):
            F.numbers = {}
            for i in range(len(F.ops)):
                F.numbers.setdefault(number_text(F, i), []).append(i)
        return F.numbers

    def value(F, E, k, c, v):
        want = E.status[F.op_rec[numbers(F).get(b"%d" % v(k), [])]]
        return bool((want == (0 if v(k) < k["LIMIT"] else stw.NUMBER_TOO_BIG)).any())
    for name, v in VALUES.items():
        add("numbers.value.%s" % name, lambda F, E, k, c, v=v: value(F, E, k, c, v))
    for z in ZEROS:
        add("numbers.limit-1_behind_%d_zeros" % z,
            lambda F, E, k, c, z=z: bool(E.good[F.op_rec[numbers(F).get(b"0" * z + b"%d" % (k["LIMIT"] - 1), [])]].any()))

    def run(F, E, k, c, digits, edges, zero_first):
        i = np.nonzero((F.n_digits == digits) & (F.ops // k["CHUNK"] - F.num_start // k["CHUNK"] == edges))[0]
        i = i[(F.text[F.num_start[i]] == 48) == zero_first]
        return bool((E.status[F.op_rec[i]] == (0 if zero_first else stw.NUMBER_TOO_BIG)).any())
    for digits, edges in ((1100, 1), (2100, 2)):
        for zero_first in (True, False):
            add("numbers.run_of_%d_digits_over_%d_chunk_edge%s.%s" % (digits, edges, "s" if edges > 1 else "", "zeros_first" if zero_first else "nonzero_first"),
                lambda F, E, k, c, d=digits, e=edges, z=zero_first: run(F, E, k, c, d, e, z))


def byte_forms(inside):
    return [(b"1M5" + bytes([b]) + b"2M") if inside else (b"5" + bytes([b])) for b in range(256)]


# the oracle's rule over the 256 byte values.  (The nine operators hold eight letters and `=`: 52 - 8 = 44 other letters.)
BYTE_COUNTS = {False: {stw.OK: 9, stw.BAD_OP: 44, stw.BAD_CHAR: 193, stw.TRAILING_DIGITS: 10},
               True: {stw.OK: 19, stw.BAD_OP: 44, stw.BAD_CHAR: 193}}


def _byte_classes(add):
    def every(F, E, k, c, inside):
        where = {t: r for r, t in enumerate(c.texts)}
        forms = byte_forms(inside)
        if not all(t in where for t in forms):
            return False
        st = [int(E.status[where[t]]) for t in forms]
        letters = [b for b in range(256) if chr(b).isascii() and chr(b).isalpha() and b not in ALL_OPS]
        return collections.Counter(st) == BYTE_COUNTS[inside] and all(st[b] == stw.BAD_OP for b in letters) and \
            all(st[b] == stw.OK for b in ALL_OPS) and st[42] == stw.BAD_CHAR and \
            all(st[b] == (stw.OK if inside else stw.TRAILING_DIGITS) for b in range(48, 58))
    add("bytes.every_value_as_the_operator", lambda F, E, k, c: every(F, E, k, c, False))
    add("bytes.every_value_inside_a_record", lambda F, E, k, c: every(F, E, k, c, True))


def sites_hold(text, sites):
    """A record's planted errors [(index of the byte the error is noted at, code)], by the oracle: every piece (the number
    in front of the byte and the byte) has its code on its own, everything between the pieces is good text, and the
    record has the first one's code."""
    cur, ok = 0, stw.parse_cigar(text)[0] == sites[0][1]
    for q, code in sites:
        s = q + 1 if code == stw.TRAILING_DIGITS else q
        while s > cur and text[s - 1:s].isdigit():
            s -= 1
        ok = ok and stw.parse_cigar(text[s:q + 1])[0] == code and (s == cur or stw.parse_cigar(text[cur:s])[0] == stw.OK)
        cur = q + 1
    return ok and (cur == len(text) or stw.parse_cigar(text[cur:])[0] == stw.OK) and [q for q, _ in sites] == sorted({q for q, _ in sites})


def distance_of(p, q, k):
    if p // k["WAVE"] == q // k["WAVE"] and p // k["CHUNK"] == q // k["CHUNK"]:
        return "same_wave"
    d = q // k["CHUNK"] - p // k["CHUNK"]
    return {0: "waves_of_one_chunk", 1: "adjacent_chunks", 2: "two_chunks_apart"}.get(d)


def _order_classes(add):
    def pair(F, E, k, c, a, b, dist):
        for r, sites in c.marks.items():
            if len(sites) == 2 and (sites[0][1], sites[1][1]) == (a, b) and sites_hold(c.texts[r], sites) and \
                    distance_of(F.rec_start[r] + sites[0][0], F.rec_start[r] + sites[1][0], k) == dist and E.status[r] == a:
                return True
        return False
    for a in range(1, 6):
        for b in range(1, 6):
            if a != b:
                for dist in DISTANCES:
                    add("order.%s_then_%s.%s" % (CODES[a], CODES[b], dist), lambda F, E, k, c, a=a, b=b, d=dist: pair(F, E, k, c, a, b, d))

    def early_with_trailing(F, E, k, c):
        return any(len(s) >= 2 and s[-1][1] == stw.TRAILING_DIGITS and sites_hold(c.texts[r], s) and s[0][0] < k["WAVE"] and
                   (F.rec_start[r] + s[-1][0]) // k["CHUNK"] > (F.rec_start[r] + s[0][0]) // k["CHUNK"] for r, s in c.marks.items())
    add("order.early_error_and_a_trailing_digit", early_with_trailing)
    # two errors noted at ONE byte: the smaller code decides (a bad byte behind no number or behind a number too big)
    add("order.two_errors_at_one_byte", lambda F, E, k, c: all(
        t in c.texts and E.status[c.texts.index(t)] == st and E.good[c.texts.index(t) - 1] and E.good[c.texts.index(t) + 1]
        for t, st in ((b"Q", stw.BAD_OP), (b"!", stw.BAD_CHAR), (b"3MQ", stw.BAD_OP), (b"%dq" % k["LIMIT"], stw.BAD_OP),
                      (b"%d!" % k["LIMIT"], stw.BAD_CHAR), (b"3M12345678901{", stw.BAD_CHAR))))
    add("order.three_errors_in_one_record",lambda F, E, k, c: any(len(s) == 3 and len({x for _, x in s}) == 3 and sites_hold(c.texts[r], s)
                                                                   for r, s in c.marks.items()))


def _classes():
    c = collections.OrderedDict()

    def add(cid, pred):
        assert cid not in c
        c[cid] = (cid.split(".")[0], pred)
    _edge_classes(add)
    for name, value in SIZES.items():
        add("size.%s" % name, lambda F, E, k, c, v=value: F.n_bytes == v(k) and (F.n_bytes == 1 or (len(F.ops) > 0 and F.n_rec >= 2)))
    for m, name in ((1, "chunk"), (2, "2chunks")):
        add("size.%s.ends_in_a_digit" % name, lambda F, E, k, c, m=m: F.n_bytes == m * k["CHUNK"] and bool(F.digit[-1]) and F.rec_len[-1] > 0
            and E.status[-1] == stw.TRAILING_DIGITS)
        add("size.%s.ends_in_an_operator" % name, lambda F, E, k, c, m=m: F.n_bytes == m * k["CHUNK"] and len(F.ops) and F.ops[-1] == F.n_bytes - 1
            and bool(E.good[-1]))
    _wave_classes(add)
    _record_classes(add)
    _number_classes(add)
    _byte_classes(add)
    _order_classes(add)
    full = lambda F, E, k, c, v: F.n_bytes == v and len(F.ops) * 2 == F.n_bytes and int(E.cigar_off[-1]) == F.n_bytes // 2
    add("capacity.every_slot.2_bytes", lambda F, E, k, c: full(F, E, k, c, 2))
    add("capacity.every_slot.chunk", lambda F, E, k, c: full(F, E, k, c, k["CHUNK"]))
    add("capacity.every_slot.2chunks+2", lambda F, E, k, c: full(F, E, k, c, 2 * k["CHUNK"] + 2))
    return c


CLASSES = _classes()
FAMILIES = ("edge", "size", "wave", "records", "chunks", "numbers", "bytes", "order", "capacity")
# Classes no text can show.  TRAILING_DIGITS is noted at the record's last byte and nowhere else, so no error of the same
# record stands behind it: it is never the first of two.
EXEMPT = {cid: "a trailing digit is the record's last byte: no error stands behind it"
          for cid in CLASSES if cid.startswith("order.TRAILING_DIGITS_then_")}


# ------------------------------------------------------------------------------------------------------- builder
def _rng(name):
    return np.random.default_rng([zlib.crc32(name.encode())])


def good(n, rng=None, ops=ALL_OPS, lead=b"1"):
    """A good record of exactly n >= 2 bytes: lengths of one digit (the first of two where n is odd)."""
    assert n >= 2
    pick = (lambda: ops[int(rng.integers(len(ops)))]) if rng is not None else (lambda: ops[0])
    dig = (lambda: 49 + int(rng.integers(9))) if rng is not None else (lambda: 49)
    out = bytearray(lead if n % 2 else b"")
    while len(out) < n:
        out += bytes([dig(), pick()])
    return bytes(out)


def record_of_ops(lengths, ops):
    return b"".join(b"%d%c" % (l, o) for l, o in zip(lengths, ops))


class Layout:
    """Records placed at byte offsets; gaps are filled with good records (`1M`, one `12M` where the gap is odd, `*` for a
    gap of one byte)."""

    def __init__(self):
        self.texts, self.size, self.marks = [], 0, {}

    def add(self, *records, sites=None):
        for t in records:
            if sites:
                self.marks[len(self.texts)] = list(sites)
            self.texts.append(bytes(t))
            self.size += len(t)
        return self

    def fill(self, upto, one=False, rng=None, ops=ALL_OPS):
        gap = upto - self.size
        assert gap >= 0, (upto, self.size)
        if gap == 1:
            return self.add(b"*")
        if one and gap:
            return self.add(good(gap, rng, ops))
        if gap % 2:
            self.add(b"12M")
        return self.add(*[b"1M"] * ((upto - self.size) // 2))

    def at(self, offset, *records, **kw):
        return self.fill(offset, **{a: kw.pop(a) for a in ("one", "rng", "ops") if a in kw}).add(*records, **kw)


def _case(name, family, texts, shows, marks=None):
    texts = tuple(bytes(t) for t in (texts.texts if isinstance(texts, Layout) else texts))
    marks = marks or {}
    text, off = batch(texts)
    return Case(name, family, texts, text, off, tuple(shows), marks)


def mixed(name, n_bytes, end="operator", errors=True):
    """Random records of 2 .. 40 bytes, about one in eight with an error, n_bytes in all."""
    rng, L = _rng(name), Layout()
    while L.size < n_bytes:
        left = n_bytes - L.size
        g = min(int(rng.integers(2, 41)), left)
        if left - g == 1:
            g += 1
        if g == 1:
            L.add(b"*")
            continue
        t = bytearray(good(g, rng))
        last = L.size + g == n_bytes
        if last and end == "digit":
            t = bytearray(good(g - 1, rng) + b"7") if g > 2 else bytearray(b"77")
        elif errors and not last and L.texts and rng.integers(8) == 0:
            t[1 + 2 * int(rng.integers(g // 2)) - (0 if g % 2 == 0 else -1)] = ord("Q")
        L.add(t)
    assert L.size == n_bytes
    return L


PIECES = {stw.BAD_CHAR: (b"5!", b"5*"), stw.BAD_OP: (b"5Q", b"5m"), stw.EMPTY_NUMBER: (b"M", b"D"),
          stw.NUMBER_TOO_BIG: (b"268435456M", b"0999999999X"), stw.TRAILING_DIGITS: (b"7", b"40")}


def record_with_errors(start, sites, tail, variant=0):
    """A record that begins at byte `start` of its text and holds an error at each absolute byte of `sites`
    [(byte, code)]; good text between them and `tail` bytes of it behind the last.  -> (text, [(index, code)])."""
    out, marks = bytearray(), []
    for q, code in sites:
        piece = PIECES[code][variant % 2]
        gap = q + 1 - len(piece) - (start + len(out))
        assert gap == 0 or gap >= 2, (q, code, gap)
        if gap:
            out += good(gap)
        out += piece
        marks.append((len(out) - 1, code))
    if tail and sites[-1][1] != stw.TRAILING_DIGITS:
        out += good(tail)
    return bytes(out), marks


# --------------------------------------------------------------------------------------------------------- table
def _edge_case(name, key, above):
    """All six edge classes of one unit, at edges of that unit that are no edges of the unit above."""
    u = LAID[key]
    top = LAID[above] if above else 1 << 30
    edges = [e for e in range(u, 40 * u, u) if e % top != 0][:6]
    L = Layout()
    e = edges[0]
    L.at(e - 4, b"123M", b"45D6M")                      # M is the last byte, its number inside; a boundary on the edge
    e = edges[1]
    L.at(e - 3, b"789" b"=7I")                          # = is the first byte, its number wholly in front of the edge
    e = edges[2]
    L.at(e - 7, b"2M12345" b"678X9S")                   # 12345 | 678 lies across the edge
    e = edges[3]
    L.at(e - 3, b"3N", b"5H6P")                         # a boundary one byte in front of the edge
    e = edges[4]
    L.at(e - 3, b"3D1M", b"1M")                         # ... and one byte behind it
    e = edges[5]
    L.at(e - 1, b"*", b"8M").fill(e + u + 7)
    return _case(name, "edge", L, ["edge.%s.%s" % (name.split("-")[1], c) for c in (
        "operator_last_byte", "operator_first_byte", "number_straddles", "record_boundary_on", "record_boundary_one_before",
        "record_boundary_one_behind")])


def _order_case(dist, number):
    """The sixteen ordered pairs of codes, one record each, the two errors `dist` apart."""
    L = Layout()
    delta = {"same_wave": 30, "waves_of_one_chunk": 30 + 2 * LAID["WAVE"], "adjacent_chunks": LAID["CHUNK"], "two_chunks_apart": 2 * LAID["CHUNK"]}[dist]
    shows, j = [], 0
    for a in range(1, 5):
        for b in range(1, 6):
            if a == b:
                continue
            start = _ceil(L.size + 2, LAID["CHUNK"]) * LAID["CHUNK"] + LAID["WAVE"]
            L.fill(start)
            q1 = start + 20
            text, marks = record_with_errors(start, [(q1, a), (q1 + delta, b)], 6, variant=j + number)
            L.add(text, sites=marks)
            shows.append("order.%s_then_%s.%s" % (CODES[a], CODES[b], dist))
            j += 1
    L.fill(L.size + 4)
    return _case("order-%s" % dist.replace("_", "-"), "order", L, shows, L.marks)


def _count_case(n_rec):
    """n_rec records of 1 .. 5 operations; error records (no operations) next to every multiple of 1024 and elsewhere."""
    rng, texts = _rng("records-%d" % n_rec), []
    for r in range(n_rec):
        n_ops = 1 + (r * 7) % 5
        t = record_of_ops(rng.integers(1, 3000, n_ops).tolist(), [ALL_OPS[int(x)] for x in rng.integers(0, 9, n_ops)])
        if r % 1024 == 0 and r or r % 97 == 50:
            t = (b"12Q3M", b"3M4", b"", b"268435456M", b"1M*")[(r // 97 + r // 1024) % 5]
        texts.append(t)
    return _case("records-%d" % n_rec, "records", texts, ["records.count.%s" % name for name, v in COUNTS.items() if v(LAID) == n_rec])


def _chunks_case(n_chunks):
    """n_chunks chunks of text whose operator density changes from chunk to chunk (lengths of 1 .. 9 digits), records of
    about eight operations, one in a hundred with an error; 1024 chunks are exactly 1 MiB."""
    rng = _rng("chunks-%d" % n_chunks)
    n_bytes = n_chunks * 1024 - (0 if n_chunks % 1024 == 0 else 371)
    texts, cur, size, j = [], bytearray(b"12M"), 3, 0
    breaks, draw = rng.integers(0, 8, 1 << 18).tolist(), rng.random(1 << 18).tolist()
    while n_bytes - size >= 24:
        d = 1 + ((size // 1024) * 5) % 9
        lo, hi = (10 ** (d - 1) if d > 1 else 1), min(10 ** d, 1 << 28)
        if breaks[j % len(breaks)] == 0:
            texts.append(bytes(cur))
            cur = bytearray()
        op = ord("Q") if not cur and len(texts) % 100 == 50 else ALL_OPS[j % 9]   # (an error record: its first operator)
        cur += b"%d%c" % (lo + int(draw[j % len(draw)] * (hi - lo)), op)
        size += d + 1
        j += 1
    cur += b"0" * (n_bytes - size - 2) + b"7M"
    texts.append(bytes(cur))
    assert sum(len(t) for t in texts) == n_bytes
    name = [nm for nm, v in COUNTS.items() if v(LAID) == n_chunks][0]
    return _case("chunks-%d" % n_chunks, "chunks", texts, ["chunks.count.%s" % name])


def _table():
    out = []
    W, C = LAID["WAVE"], LAID["CHUNK"]
    A = lambda *a, **kw: out.append(_case(*a, **kw))
    # ---- edges
    for name, key, above in UNITS:
        out.append(_edge_case("edge-%s" % name, key, above))
    # ---- sizes
    for name, value in SIZES.items():
        n = value(LAID)
        if n == 1:
            A("size-1", "size", [b"M"], ["size.1"])
            continue
        shows = ["size.%s" % name] + (["size.%s.ends_in_an_operator" % name] if name in ("chunk", "2chunks") else [])
        A("size-%d" % n, "size", mixed("size-%d" % n, n), shows)
        if name in ("chunk", "2chunks"):
            A("size-%d-ends-in-a-digit" % n, "size", mixed("size-%d-digit" % n, n, end="digit"), ["size.%s" % name, "size.%s.ends_in_a_digit" % name])
    # ---- waves: every special wave begins at a multiple of 64 with a good record directly in front and behind
    rng = _rng("waves")
    L = Layout().add(b"5M")
    L.at(3 * W - 10, good(2 * W + 20, rng, REF_OPS), b"9M")
    L.at(8 * W - 10, good(2 * W + 21, rng, NOREF_OPS), b"9M")
    bad = bytearray(good(3 * W, rng, REF_OPS))
    bad[1] = ord("Q")                                      # the error stands in the record's first wave, two good waves behind it
    L.at(13 * W, bad, b"9M")
    A("wave-inside-one-record", "wave", L.fill(L.size + 6), ["wave.inside_one_good_record_of_MDN=X", "wave.inside_one_good_record_of_ISHP",
                                                            "wave.inside_one_error_record"])
    L = Layout().add(b"5M")
    L.at(2 * W, good(32, rng, REF_OPS), good(32, rng, REF_OPS))
    L.at(4 * W, good(20, rng, REF_OPS), good(24, rng), good(20, rng, REF_OPS))
    L.at(6 * W - 6, b"7M7D7N")                             # 32 records of `1M` in the wave behind it
    L.fill(7 * W).add(b"8=", b"3X")
    A("wave-over-2-3-32-records", "wave", L, ["wave.over_2_records", "wave.over_3_records", "wave.over_32_records"])
    L = Layout().add(b"5M")
    L.at(2 * W - 8, good(8 + W - 1, rng, REF_OPS), good(41, rng, REF_OPS))                 # lane 63 is the next record's first digit
    L.at(6 * W - 9, good(10, rng, REF_OPS), good(W - 1 + 30, rng, REF_OPS), b"2M")         # lane 0 is the last operator of the record before
    L.at(10 * W, good(20, rng, REF_OPS), b"4M5Q6D7M", good(36, rng, REF_OPS), b"3M")
    A("wave-lone-lanes-and-an-error-between", "wave", L, ["wave.last_lane_in_the_next_record", "wave.first_lane_in_the_record_before",
                                                           "wave.error_record_between_two_good_ones"])
    L = Layout().add(b"5M")
    for i, m in enumerate((1, 2, 65)):
        L.at((2 + 3 * i) * W - 4, good(4 + 30, rng, REF_OPS), *[b""] * m)
        L.add(good(50, rng, REF_OPS), b"3M")
    A("wave-empty-records-between-lanes", "wave", L, ["wave.%d_empty_records_between_two_lanes" % m for m in (1, 2, 65)])
    L = Layout().add(b"5M")
    L.at(2 * W - 14, b"268435455M" * 9, b"6M")             # 9 * (2^28 - 1) = 2^31 + 2^28 - 9, over three waves
    L.at(5 * W + 5, b"268435455D1I" * 17, b"6M")           # 17 * (2^28 - 1) = 2^32 + 2^28 - 17
    A("wave-ref-len-past-2^31-and-2^32", "wave", L, ["wave.ref_len_passes_2^31", "wave.ref_len_passes_2^32"])
    # ---- records: empty and `*` records
    for kind, t in (("empty", b""), ("star", b"*")):
        A("records-%s-first" % kind, "records", [t, b"12M", b"3D"], ["records.%s.first" % kind])
        A("records-%s-last-inside-a-chunk" % kind, "records", [b"12M", b"3D", t], ["records.%s.last.text_ends_inside_a_chunk" % kind])
        A("records-%s-last-whole-chunks" % kind, "records", _whole_chunk_last(kind), ["records.%s.last.text_of_whole_chunks" % kind])
        for m in (1, 2, 65):
            L = Layout().add(b"5M")
            if kind == "empty":
                L.at(2 * C - 6, b"11M22D", *[t] * m).add(b"33N4M", b"2M")
            else:                                           # the run's first `*` is a chunk's last byte
                L.at(2 * C - 4, b"11M", *[t] * m).add(b"33N4M", b"2M")
                if m == 1:                                  # ... and the single `*` as a chunk's first byte
                    L.at(3 * C - 3, b"11M", t, b"33N4M", b"2M")
            A("records-%s-run-of-%d" % (kind, m), "records", L, ["records.%s.run_of_%d_on_a_chunk_edge" % (kind, m)])
    for name, value in ONLY_EMPTY.items():
        A("records-only-empty-%d" % value(LAID), "records", [b""] * value(LAID), ["records.only_empty.%s" % name])
    for name, value in COUNTS.items():
        out.append(_count_case(value(LAID)))
    for name, value in list(COUNTS.items())[:3]:
        out.append(_chunks_case(value(LAID)))
    # ---- numbers
    texts = [b"3M"]
    for name, value in VALUES.items():
        texts += [b"%d%c" % (value(LAID), b"MDN=X"[len(texts) % 5]), b"3M"]
    for z in ZEROS:
        texts += [b"2I" + b"0" * z + b"268435455D", b"3M"]
    A("numbers-values", "numbers", texts, ["numbers.value.%s" % n for n in VALUES] + ["numbers.limit-1_behind_%d_zeros" % z for z in ZEROS])
    for digits, edges in ((1100, 1), (2100, 2)):
        for zero_first in (True, False):
            run = (b"0" * (digits - 9) + b"268435455") if zero_first else (b"1" + b"0" * (digits - 1))
            L = Layout().add(b"5M").at(498, b"3M" + run + b"N4M", b"6D")       # the run begins at byte 500
            L.fill(L.size + 12)
            A("numbers-run-of-%d-%s" % (digits, "zeros-first" if zero_first else "nonzero-first"), "numbers", L,
              ["numbers.run_of_%d_digits_over_%d_chunk_edge%s.%s" % (digits, edges, "s" if edges > 1 else "", "zeros_first" if zero_first else "nonzero_first")])
    # ---- bytes
    for inside in (False, True):
        texts = [b"3M"]
        for t in byte_forms(inside):
            texts += [t, b"3M"]
        A("bytes-%s" % ("inside-a-record" if inside else "as-the-operator"), "bytes", texts,
          ["bytes.every_value_%s" % ("inside_a_record" if inside else "as_the_operator")])
    # ---- order of errors
    for number, dist in enumerate(DISTANCES):
        out.append(_order_case(dist, number))
    L = Layout().add(b"5M")
    t, m = record_with_errors(L.size, [(L.size + 9, stw.BAD_OP), (L.size + 9 + 2 * C + 100, stw.TRAILING_DIGITS)], 0)
    L.add(t, sites=m).add(b"6M")
    start = _ceil(L.size, C) * C + W
    t, m = record_with_errors(start, [(start + 20, stw.NUMBER_TOO_BIG), (start + 20 + C, stw.BAD_CHAR), (start + 50 + C + W, stw.EMPTY_NUMBER)], 8, variant=1)
    L.at(start, t, sites=m).add(b"6M")
    for t in (b"Q", b"!", b"3MQ", b"268435456q", b"268435456!", b"3M12345678901{"):
        L.add(t, b"6M")
    A("order-trailing-digit-and-three-errors", "order", L, ["order.early_error_and_a_trailing_digit", "order.three_errors_in_one_record",
                                                             "order.two_errors_at_one_byte"], L.marks)
    # ---- capacity: `1M` over and over, one record
    for n, name in ((2, "2_bytes"), (C, "chunk"), (2 * C + 2, "2chunks+2")):
        A("capacity-%d" % n, "capacity", [b"1M" * (n // 2)], ["capacity.every_slot.%s" % name])
    return collections.OrderedDict((c.name, c) for c in out)


def _whole_chunk_last(kind):
    """A text of exactly one chunk whose last record is empty (rec_off == n_bytes) or a `*` (the chunk's last byte)."""
    L = Layout().add(b"12M")
    if kind == "empty":
        return L.fill(LAID["CHUNK"] - 4).add(b"4D5M", b"")
    return L.fill(LAID["CHUNK"] - 5).add(b"4D5M", b"*")


CASES = _table()
MEGABYTE_CASES = ("chunks-1023", "chunks-1024", "chunks-1025")


def family(name):
    return [c for c in CASES.values() if c.family == name]


@functools.lru_cache(maxsize=None)
def case_expected(name):
    return expected(combined().texts if name == "combined" else CASES[name].texts)


@functools.lru_cache(maxsize=None)
def case_facts(name):
    c = combined() if name == "combined" else CASES[name]
    return facts(c.text, c.rec_off)


@functools.lru_cache(maxsize=1)
def combined():
    """Every case in ONE batch, each starting at a multiple of 1024 bytes (records of `1M` between them), so that every
    byte keeps its place in its chunk, step and wave.  -> Case; marks: {case name: (first byte, first record)}."""
    L, at = Layout(), {}
    for c in CASES.values():
        L.fill(_ceil(L.size, LAID["CHUNK"]) * LAID["CHUNK"])
        at[c.name] = (L.size, len(L.texts))
        L.add(*c.texts)
    L.fill(L.size + 2)
    return _case("combined", "combined", L, [], at)


def check_preconditions(k=None, cases=None):
    """Every case shows the classes it lists; every class of CLASSES but those of EXEMPT is shown by a case.  `k`: the
    constants the classes are judged with (default K; the cases stay as they were laid out)."""
    k = k or K
    default = cases is None
    shown = set()
    for c in (cases or CASES).values():
        own = CASES.get(c.name) is c
        F = case_facts(c.name) if own and k == K else facts(c.text, c.rec_off, k)
        E = case_expected(c.name) if own else expected(c.texts)
        assert c.shows, c.name
        for cid in c.shows:
            assert cid not in EXEMPT, (c.name, cid)
            assert CLASSES[cid][1](F, E, k, c), "%s does not show %s" % (c.name, cid)
            shown.add(cid)
    if default:
        missing = [cid for cid in CLASSES if cid not in shown and cid not in EXEMPT]
        assert not missing, missing
        assert all(cid.startswith("order.TRAILING_DIGITS_then_") for cid in EXEMPT) and len(EXEMPT) == 16
    return shown
