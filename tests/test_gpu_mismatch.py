"""svx_cigar_mismatch on the device (svim_asm_amd/csrc/svx_mismatch.hip) against the loop of tests/mismatch_restatement.py,
element for element: one M op at the tile's edges with mismatches in every tile's first and last column, a whole tile of
mismatches, one op per column over more than a tile, pools of 1 to 4097 ops over several alignments, every op code,
letter case and letters outside ACGT, every residue of both pool offsets modulo 16, lengths shorter than the CIGAR's use
with a canary behind each range, empty alignments, prefixes beyond 2^32, the capacity contract, the _dev form, the
refusals, poisoned scratch and 200 random small cases."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import mismatch_restatement as MM

pytestmark = pytest.mark.gpu

M, I, D, N, S, H, P, EQ, X = range(9)
T = _lib.MISMATCH_TILE
COLS = ("aln", "ref_pos", "qry_pos", "ref_base", "qry_base")
OTHER = {65: 67, 67: 71, 71: 84, 84: 65}  # another base than the given one


def columns(ops):
    """(reference offset, query offset) of every aligned column of `ops`, and both totals."""
    pairs, r, q = [], 0, 0
    for op, n in ops:
        if op in (M, EQ, X):
            pairs += [(r + j, q + j) for j in range(n)] if n < (1 << 20) else []
        if op in (M, D, N, EQ, X):
            r += n
        if op in (M, I, S, EQ, X):
            q += n
    return pairs, r, q


def sequences(rng, ops, rate=0.02, alphabet=b"ACGT"):
    """A reference window and a SEQ that fit `ops`: aligned columns equal but for `rate` of them."""
    pairs, r, q = columns(ops)
    ref = bytearray(rng.choice(alphabet) for _ in range(r))
    qry = bytearray(rng.choice(alphabet) for _ in range(q))
    for i, j in pairs:
        qry[j] = ref[i] if rng.random() >= rate else rng.choice(alphabet)
    return ref, qry


class Aln(object):
    def __init__(self, start, ops, ref, qry, ref_len=None, qry_len=None, ref_res=None, qry_res=None):
        self.start, self.ops, self.ref, self.qry = start, ops, bytearray(ref), bytearray(qry)
        self.ref_len = len(ref) if ref_len is None else ref_len
        self.qry_len = len(qry) if qry_len is None else qry_len
        self.ref_res, self.qry_res = ref_res, qry_res


def canary(aln, side):
    """The byte behind a range that an overrun would meet: a base that DIFFERS from the one the next column holds on the
    other side, so that comparing it would give an event."""
    pairs, _, _ = columns(aln.ops)
    if side == "ref":
        other = [aln.qry[q] for r, q in pairs if r == aln.ref_len and q < len(aln.qry)]
    else:
        other = [aln.ref[r] for r, q in pairs if q == aln.qry_len and r < len(aln.ref)]
    return OTHER.get((other[0] & 0xDF) if other else 65, 65)


def pack(alns, rng=None):
    """The entry point's arguments: every range at its residue modulo 16 (random without one), a canary behind it."""
    rng = rng or random.Random(len(alns))
    pool, ref_off, qry_off = bytearray(), [], []

    def place(data, res, mark):
        res = rng.randrange(16) if res is None else res
        pool.extend(b"T" * ((res - len(pool)) % 16))
        at = len(pool)
        pool.extend(data)
        pool.append(mark)
        return at
    for a in alns:
        ref_off.append(place(a.ref[:a.ref_len], a.ref_res, canary(a, "ref")))
        qry_off.append(place(a.qry[:a.qry_len], a.qry_res, canary(a, "qry")))
    words = np.array([(n << 4) | op for a in alns for op, n in a.ops], dtype=np.uint32)
    off = np.zeros(len(alns) + 1, np.uint64)
    np.cumsum([len(a.ops) for a in alns], out=off[1:])
    return (words, off, np.array([a.start for a in alns], dtype=np.int32), np.frombuffer(bytes(pool), dtype=np.uint8),
            np.array(ref_off, dtype=np.uint64), np.array([a.ref_len for a in alns], dtype=np.uint32),
            np.array(qry_off, dtype=np.uint64), np.array([a.qry_len for a in alns], dtype=np.uint32))


def one_m(n):
    """One M op of n columns, equal but for the first and last column of every tile."""
    rng = random.Random(n)
    ref, qry = sequences(rng, [(M, n)], rate=0.0)
    for c in range(n):
        if c % T in (0, T - 1) or c == n - 1:
            qry[c] = OTHER[ref[c]]
    return pack([Aln(77, [(M, n)], ref, qry)], rng)


def whole_tile():
    n = 3 * T + 5
    rng = random.Random(31)
    ref, qry = sequences(rng, [(S, 3), (EQ, n)], rate=0.0)
    for c in range(T, 2 * T):
        qry[3 + c] = OTHER[ref[c]]
    return pack([Aln(5, [(S, 3), (EQ, n)], ref, qry)], rng)


def op_per_column(second, pairs):
    rng = random.Random(pairs + second)
    ops = [(M, 1), (second, 1)] * pairs + [(M, 1)]
    ref, qry = sequences(rng, ops, rate=0.3)
    return pack([Aln(1000, ops, ref, qry)], rng)


def random_ops(rng, n):
    ops = []
    for k in range(n):
        r = rng.random()
        if k in (0, n - 1) and n > 2 and r < 0.6:
            op = rng.choice((S, H))
        elif r < 0.5:
            op = rng.choice((M, EQ, X))
        elif r < 0.65:
            op = I
        elif r < 0.8:
            op = D
        elif r < 0.88:
            op = N
        elif r < 0.94:
            op = P
        else:
            op = rng.choice((9, 12, 15))
        ops.append((op, rng.randrange(1, 40)))
    if not any(op in (M, EQ, X) for op, _ in ops):
        ops[n // 2] = (M, 13)
    return ops


def pool_of(sizes, seed):
    rng = random.Random(seed)
    alns = []
    for n in sizes:
        ops = random_ops(rng, n)
        ref, qry = sequences(rng, ops, rate=0.05, alphabet=b"ACGTacgtN")
        alns.append(Aln(rng.randrange(0, 1 << 24), ops, ref, qry))
    return pack(alns, rng)


def every_code():
    rng = random.Random(16)
    ops = [(H, 4), (S, 6), (M, 9), (N, 7), (EQ, 5), (I, 3), (X, 4), (D, 2), (P, 8), (M, 3)] + [(c, 5) for c in range(9, 16)] + [(M, 6), (S, 5), (H, 2)]
    ref, qry = sequences(rng, ops, rate=0.5)
    return pack([Aln(42, ops, ref, qry)], rng)


def letters():
    ref = b"AaAaCGTNRY=ACGTacgtn*"
    qry = b"aAcCcgtAAAAN=RYTgcaAC"
    return pack([Aln(10, [(M, len(ref))], ref, qry)])


# a / A: none; A / c and a / C: A, C; N, R, Y, = and * on either side: none; lower case on the reference side: upper case out
LETTERS_EXPECTED = [(12, 2, "A", "C"), (13, 3, "A", "C"), (25, 15, "A", "T"), (26, 16, "C", "G"), (27, 17, "G", "C"), (28, 18, "T", "A")]


def residues():
    rng = random.Random(256)
    alns = []
    for k in range(256):
        ops = [(S, rng.randrange(0, 4)), (M, rng.randrange(1, 40)), (I, 2), (M, rng.randrange(1, 40))]
        ref, qry = sequences(rng, ops, rate=0.3)
        alns.append(Aln(k, ops, ref, qry, ref_res=k % 16, qry_res=k // 16))
    return pack(alns, rng)


def short_lengths():
    rng = random.Random(9)
    alns = []
    for ref_cut, qry_cut in ((0, None), (None, 0), (0, 0), (1, None), (None, 1), (17, None), (None, 17), (T + 3, None), (None, T - 2), (40, 33), (16, 16)):
        ops = [(S, 5), (M, 30), (D, 3), (M, T + 40), (I, 4), (M, 50), (S, 2)]
        ref, qry = sequences(rng, ops, rate=0.1)
        alns.append(Aln(rng.randrange(1000), ops, ref, qry, ref_len=ref_cut, qry_len=qry_cut))
    return pack(alns, rng)


def empties():
    rng = random.Random(3)
    ops = [(M, 20), (I, 1), (M, 20)]
    ref, qry = sequences(rng, ops, rate=0.3)
    return pack([Aln(0, [], b"", b""), Aln(9, ops, ref, qry), Aln(1, [], b"ACGT", b"TTTT"), Aln(2, [(S, 4), (I, 2)], b"", b"ACGTAC"),
                 Aln(3, [(D, 4)], b"ACGT", b""), Aln(11, ops, ref, qry), Aln(0, [], b"", b"")], rng)


def wide():
    """40 alignments of one 2^27M op with 300 bases each: the reference prefix passes 2^32, the pool stays small."""
    rng = random.Random(40)
    alns = []
    for a in range(40):
        ref, qry = sequences(rng, [(M, 300)], rate=0.05)
        alns.append(Aln(a * 1000, [(M, 1 << 27)], ref, qry))
    return pack(alns, rng)


CASES = {"one_m_%d" % n: functools.partial(one_m, n) for n in (1, T - 1, T, T + 1, 2 * T + 1)}
CASES.update(whole_tile=whole_tile, md_4097=functools.partial(op_per_column, D, 2048), mi_4097=functools.partial(op_per_column, I, 2048),
             md_tile=functools.partial(op_per_column, D, T + 3), mi_tile=functools.partial(op_per_column, I, T + 3),
             every_code=every_code, letters=letters, residues=residues, short_lengths=short_lengths, empties=empties, wide=wide,
             pool_small=functools.partial(pool_of, (1, 2, 3, 63, 64, 65, 255, 256, 257), 1),
             pool_chunk=functools.partial(pool_of, (1023, 1, 1024, 2, 1025), 2), pool_4097=functools.partial(pool_of, (4097, 5), 3),
             pool_2049=functools.partial(pool_of, (700, 2049, 300, 1), 4))


@functools.lru_cache(maxsize=None)
def case(name):
    inputs = CASES[name]()
    return inputs, MM.mismatch_batch(*inputs)


def check(name, got):
    expected = case(name)[1]
    for k in COLS:
        assert got[k].dtype == (np.uint8 if k.endswith("base") else np.uint32)
        assert got[k].tolist() == expected[k], (name, k)


def raw(ctx, inputs, cap):
    """The C entry as it is: (status, n_out, the `cap` rows' buffers)."""
    cigar, off, start, bases, ref_off, ref_len, qry_off, qry_len = inputs
    out = {k: np.full(cap + 1, 0xEE, np.uint8 if k.endswith("base") else np.uint32) for k in COLS}
    soa = _lib.MismatchSoa(*(out[k].ctypes.data for k in COLS))
    n = C.c_uint64(12345)
    rc = ctx.lib.svx_cigar_mismatch(ctx.h, cigar.ctypes.data, off.ctypes.data, start.ctypes.data, len(start), bases.ctypes.data, len(bases),
                                    ref_off.ctypes.data, ref_len.ctypes.data, qry_off.ctypes.data, qry_len.ctypes.data, soa, cap, C.byref(n))
    return rc, int(n.value), out


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_hold_events(name):
    inputs, expected = case(name)
    assert len(expected["aln"]) > 0
    keys = list(zip(expected["aln"], expected["ref_pos"]))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    if name.startswith("one_m_"):
        n = int(name[6:])
        assert [p - 77 for p in expected["ref_pos"]] == sorted({c for c in range(n) if c % T in (0, T - 1) or c == n - 1})
    if name == "whole_tile":
        assert [p - 5 for p in expected["ref_pos"]] == list(range(T, 2 * T))
    if name in ("md_4097", "mi_4097"):
        assert len(inputs[0]) == 4097 > _lib.LIFT_CHUNK
    if name == "letters":
        got = list(zip(expected["ref_pos"], expected["qry_pos"], map(chr, expected["ref_base"]), map(chr, expected["qry_base"])))
        assert got == LETTERS_EXPECTED
    if name == "wide":
        assert 40 * (1 << 27) > 1 << 32 and len(set(expected["aln"])) == 40


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_equals_the_restatement(svx_ctx, name):
    check(name, svx_ctx.cigar_mismatch(*case(name)[0]))


def test_canaries_would_show_an_overrun():
    """With the lengths one byte longer the restatement finds more events in short_lengths: the canaries are live."""
    cigar, off, start, bases, ref_off, ref_len, qry_off, qry_len = case("short_lengths")[0]
    n = len(case("short_lengths")[1]["aln"])
    assert len(MM.mismatch_batch(cigar, off, start, bases, ref_off, ref_len + 1, qry_off, qry_len)["aln"]) > n
    assert len(MM.mismatch_batch(cigar, off, start, bases, ref_off, ref_len, qry_off, qry_len + 1)["aln"]) > n


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_answers_do_not_depend_on_what_scratch_held(svx_ctx, byte):
    svx_ctx.cigar_mismatch(*case("pool_4097")[0])  # (the regions exist from here on)
    for name in sorted(CASES):
        svx_ctx.scratch_fill(byte)
        check(name, svx_ctx.cigar_mismatch(*case(name)[0]))


@pytest.mark.parametrize("name", ["pool_chunk", "md_4097", "wide", "residues"])
def test_the_dev_form(svx_ctx, name):
    inputs = case(name)[0]
    pool = svx_ctx.dev_array(np.concatenate((inputs[0], np.full(7, (9 << 4) | M, np.uint32))))
    try:
        check(name, svx_ctx.cigar_mismatch(pool.ptr, *inputs[1:], n_ops=len(inputs[0]) + 7))
    finally:
        pool.free()


def test_capacity(svx_ctx):
    inputs, expected = case("pool_chunk")
    count = len(expected["aln"])
    assert count > 2
    for cap in (0, count - 1, count):
        rc, n, out = raw(svx_ctx, inputs, cap)
        assert n == count and rc == (_lib.SVX_OK if cap >= count else _lib.SVX_E_CAPACITY)
        for k in COLS:
            assert out[k][:cap].tolist() == expected[k][:cap]
            assert out[k][cap] == 0xEE  # nothing behind cap is written
    # and the binding repeats the call with the exact count
    check("pool_chunk", svx_ctx.cigar_mismatch(*inputs, cap=1))


def test_no_alignments(svx_ctx):
    z = np.zeros
    got = svx_ctx.cigar_mismatch(z(0, np.uint32), z(1, np.uint64), z(0, np.int32), z(0, np.uint8), z(0, np.uint64), z(0, np.uint32), z(0, np.uint64),
                                 z(0, np.uint32))
    assert all(len(got[k]) == 0 for k in COLS)
    rc, n, _ = raw(svx_ctx, (z(0, np.uint32), z(1, np.uint64), z(0, np.int32), z(0, np.uint8), z(0, np.uint64), z(0, np.uint32), z(0, np.uint64),
                             z(0, np.uint32)), 4)
    assert (rc, n) == (_lib.SVX_OK, 0)


REFUSALS = ["aln_off[0] != 0", "decreasing offsets", "negative ref_start", "window behind the pool", "SEQ behind the pool",
            "window behind 2^32 - 1", "pool shorter than the offsets"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_leave_the_context_usable(svx_ctx, what):
    cigar, off, start, bases, ref_off, ref_len, qry_off, qry_len = [a.copy() for a in case("pool_small")[0]]
    kw, names = {}, "alignment 4"
    if what == "aln_off[0] != 0":
        off[0], names = 1, "aln_off[0]"
    elif what == "decreasing offsets":
        off[5] = off[4] - 1
    elif what == "negative ref_start":
        start[4] = -1
    elif what == "window behind the pool":
        ref_len[4] = len(bases) - int(ref_off[4]) + 1
    elif what == "SEQ behind the pool":
        qry_off[4], qry_len[4] = len(bases) + 1, 0
    elif what == "window behind 2^32 - 1":
        start[4], ref_len[4] = (1 << 31) - 1, (1 << 31) + 1
    else:
        pool = svx_ctx.dev_array(cigar)
        cigar, kw, names = pool.ptr, {"n_ops": len(case("pool_small")[0][0]) - 1}, "behind the pool"
    try:
        with pytest.raises(_lib.SvxError) as e:
            svx_ctx.cigar_mismatch(cigar, off, start, bases, ref_off, ref_len, qry_off, qry_len, **kw)
    finally:
        if kw:
            pool.free()
    assert e.value.status == _lib.SVX_E_INVALID and names in str(e.value)
    if what == "window behind 2^32 - 1":
        assert "2^32" in str(e.value)
    check("pool_small", svx_ctx.cigar_mismatch(*case("pool_small")[0]))


def test_200_random_small_cases(svx_ctx):
    rng = random.Random(200)
    for k in range(200):
        alns = []
        for _ in range(rng.randrange(1, 5)):
            ops = random_ops(rng, rng.randrange(1, 12))
            ref, qry = sequences(rng, ops, rate=rng.choice((0.0, 0.05, 0.5, 1.0)), alphabet=rng.choice((b"ACGT", b"ACGTacgtNn", b"AC")))
            cut = rng.random()
            alns.append(Aln(rng.randrange(0, 1 << 30), ops, ref, qry,
                            ref_len=rng.randrange(len(ref) + 1) if cut < 0.15 else None, qry_len=rng.randrange(len(qry) + 1) if cut > 0.85 else None))
        inputs = pack(alns, rng)
        expected = MM.mismatch_batch(*inputs)
        got = svx_ctx.cigar_mismatch(*inputs)
        for key in COLS:
            assert got[key].tolist() == expected[key], (k, key)
