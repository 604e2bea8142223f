"""svx_cigar_lift on the device (svim_asm_amd/csrc/svx_lift.hip) against the loop of tests/lift_restatement.py, element
for element: one-alignment pools at the wave, workgroup and chunk edges of the scan, a pool of many alignments whose
borders straddle chunk edges (an alignment without ops, alignments of clips and insertions only, every op code), one op
of 2^28 - 1 bases, a pool whose reference sum passes 2^32, a pool whose chunk sums take two passes of the second level;
every case again on poisoned scratch, behind a svx_cover_query of another size and through the _dev form; the refusals.

Every case holds all four states, between a tenth and nine tenths of its queries ALIGNED — but the one-op pool, whose
single M op leaves no place for DELETED."""
import functools
import random

import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import cover_cases as K, lift_restatement as LR

pytestmark = pytest.mark.gpu

M, I, D, N, S, H, P, EQ, X = range(9)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)
QUERY_COUNTS = (0, 1, 63, 64, 65, 1000)


def random_ops(rng, n):
    """n ops: clips at the ends only, every code 0..8 and codes above 8 (which consume nothing) inside."""
    if n == 1:
        return [(M, 17)]
    if n == 2:
        return [(M, 9), (D, 4)]
    ops = []
    for k in range(n):
        r = rng.random()
        if k == 0 and r < 0.7:
            op = rng.choice((S, H))
        elif k == n - 1 and r < 0.7:
            op = rng.choice((S, H))
        elif r < 0.45:
            op = rng.choice((M, EQ, X))
        elif r < 0.62:
            op = I
        elif r < 0.82:
            op = D
        elif r < 0.90:
            op = N
        elif r < 0.96:
            op = P
        else:
            op = rng.choice((9, 12, 15))
        ops.append((op, rng.randrange(1, 30)))
    if not any(op in (M, EQ, X) for op, _ in ops):
        ops[n // 2] = (M, 11)
    return ops


def positions(rng, ops, ref_start, at_most=48):
    """Reference positions worth asking of one alignment: one in front of it, its first base, the first and last base
    of (at most `at_most` of) its reference-consuming ops — inside D and N, directly behind an I —, its last base, its
    end and one behind."""
    spans, ref = [], ref_start
    for op, n in ops:
        if op in (M, D, N, EQ, X):
            spans.append((ref, ref + n))
            ref += n
    if len(spans) > at_most:
        spans = [spans[0], spans[-1]] + rng.sample(spans[1:-1], at_most - 2)
    out = [ref_start - 1, ref_start, ref - 1, ref, ref + 1]
    for a, b in spans:
        out += [a, b - 1, (a + b) // 2]
    return out


def pack(alignments):
    """[(ref_start, ops)] -> (cigar words, aln_off, ref_start) as numpy arrays."""
    words = np.array([(n << 4) | op for _, ops in alignments for op, n in ops], dtype=np.uint32)
    off = np.zeros(len(alignments) + 1, np.uint64)
    np.cumsum([len(ops) for _, ops in alignments], out=off[1:])
    return words, off, np.array([s for s, _ in alignments], dtype=np.int32)


def with_queries(rng, alignments, ask=None):
    q_aln, q_ref = [], []
    for a in (range(len(alignments)) if ask is None else ask):
        for r in positions(rng, alignments[a][1], alignments[a][0]):
            q_aln.append(a)
            q_ref.append(r)
    order = list(range(len(q_aln)))
    rng.shuffle(order)
    return pack(alignments) + (np.array(q_aln, dtype=np.uint32)[order], np.array(q_ref, dtype=np.int64)[order])


def single(n):
    rng = random.Random(1000 + n)
    return with_queries(rng, [(rng.randrange(0, 5000), random_ops(rng, n))])


def mixed():
    """Alignments of 1 to 700 ops back to back, their borders all over the chunks of 1024; between them an alignment
    without ops, alignments of S / I / H ops only, one with leading and trailing H and S, one with every code."""
    rng = random.Random(77)
    alns = [(rng.randrange(0, 1 << 20), random_ops(rng, rng.choice((1, 2, 3, 40, 300, 700, 1023)))) for _ in range(24)]
    alns.insert(5, (123, []))
    alns.insert(9, (500, [(S, 5), (I, 7), (H, 2)]))
    alns.insert(10, (600, [(H, 3), (S, 4), (M, 10), (I, 2), (M, 1), (D, 3), (M, 6), (S, 8), (H, 1)]))
    alns.insert(11, (-5, [(EQ, 3), (X, 2), (I, 4), (D, 2), (N, 6), (P, 3), (M, 5), (11, 9), (S, 2)]))  # (starts in front of 0)
    alns.insert(20, (7, [(I, 3), (S, 2)]))
    return with_queries(rng, alns)


def long_op():
    rng = random.Random(5)
    return with_queries(rng, [(1000, [(S, 10), (M, (1 << 28) - 1), (D, 5), (M, 3)])])


def wide():
    """40 alignments of one 2^27M op each — the pool's reference prefix passes 2^32 —, and a short one behind them."""
    rng = random.Random(6)
    return with_queries(rng, [(a * 1000, [(M, 1 << 27)]) for a in range(40)] + [(50, [(M, 5), (D, 3), (I, 2), (M, 5)])])


def two_pass():
    """About 1.1 M ops: more than 1024 chunks of 1024, so the scan of the chunk sums takes a second pass with a carry;
    queries on alignments of the first pass, around its edge and at the pool's end."""
    rng = random.Random(8)
    distinct = [random_ops(rng, 997) for _ in range(24)]  # (the queried ones are among the first and the last of them)
    alns = [(rng.randrange(0, 1 << 24), distinct[a % len(distinct)]) for a in range(1105)]
    assert sum(len(ops) for _, ops in alns) > _lib.LIFT_CHUNK * _lib.LIFT_CHUNK + 4 * _lib.LIFT_CHUNK
    return with_queries(rng, alns, ask=[0, 1, 500, 1050, 1051, 1052, 1053, 1054, 1103, 1104])


CASES = {"ops_%d" % n: functools.partial(single, n) for n in SIZES}
CASES.update(mixed=mixed, long_op=long_op, wide=wide, two_pass=two_pass)


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, expected query offsets, expected states): the restatement runs once per case."""
    inputs = CASES[name]()
    cigar, off, start, q_aln, q_ref = inputs
    only = sorted(set(q_aln.tolist()))  # (the loop decodes the alignments that are asked about)
    again = {a: k for k, a in enumerate(only)}
    sub = [cigar[int(off[a]):int(off[a + 1])] for a in only]
    sub_off = np.concatenate(([0], np.cumsum([len(w) for w in sub])))
    query, state = LR.lift_batch(np.concatenate(sub) if sub else cigar[:0], sub_off, start[only], [again[a] for a in q_aln.tolist()], q_ref)
    return inputs, query, state


def check(name, got):
    _, query, state = case(name)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint8
    assert got[1].tolist() == state and got[0].tolist() == query


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_hold_every_state(name):
    _, _, state = case(name)
    aligned = state.count(LR.ALIGNED)
    assert 10 * aligned >= len(state) and 10 * aligned <= 9 * len(state)
    assert {LR.OUTSIDE, LR.ALIGNED, LR.END} <= set(state) and (LR.DELETED in state or name == "ops_1")


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_equals_the_restatement(svx_ctx, name):
    check(name, svx_ctx.cigar_lift(*case(name)[0]))


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_answers_do_not_depend_on_what_scratch_held(svx_ctx, byte):
    svx_ctx.cigar_lift(*case("two_pass")[0])  # (the regions exist from here on)
    for name in sorted(CASES):
        svx_ctx.scratch_fill(byte)
        check(name, svx_ctx.cigar_lift(*case(name)[0]))


def test_every_case_behind_a_cover_query_of_another_size(svx_ctx):
    from tests.test_gpu_cover import arrays
    for k, name in enumerate(sorted(CASES)):
        lists, queries = K.CASES[sorted(K.CASES)[k % len(K.CASES)]]()
        assert svx_ctx.cover_query(*arrays(lists, queries)).tolist() == K.answers(sorted(K.CASES)[k % len(K.CASES)])
        check(name, svx_ctx.cigar_lift(*case(name)[0]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_dev_form(svx_ctx, name):
    cigar, off, start, q_aln, q_ref = case(name)[0]
    # the pool in HBM with words behind the alignments' last one: n_ops says how long it is
    pool = svx_ctx.dev_array(np.concatenate((cigar, np.full(7, (9 << 4) | M, np.uint32))))
    try:
        check(name, svx_ctx.cigar_lift(pool.ptr, off, start, q_aln, q_ref, n_ops=len(cigar) + 7))
    finally:
        pool.free()


@pytest.mark.parametrize("n_q", QUERY_COUNTS)
def test_query_counts(svx_ctx, n_q):
    (cigar, off, start, q_aln, q_ref), query, state = case("mixed")
    assert len(q_aln) >= max(QUERY_COUNTS)
    got = svx_ctx.cigar_lift(cigar, off, start, q_aln[:n_q], q_ref[:n_q])
    assert got[0].tolist() == query[:n_q] and got[1].tolist() == state[:n_q]


def test_no_alignments_and_alignments_without_ops(svx_ctx):
    none = svx_ctx.cigar_lift(np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.uint32), np.zeros(0, np.int64))
    assert len(none[0]) == len(none[1]) == 0
    got = svx_ctx.cigar_lift(np.zeros(0, np.uint32), np.zeros(4, np.uint64), np.array([5, 6, 7], np.int32), np.array([0, 2, 1], np.uint32),
                             np.array([5, 7, 0], np.int64))
    assert got[0].tolist() == [0, 0, 0] and got[1].tolist() == [LR.OUTSIDE] * 3


@pytest.mark.parametrize("what", ["aln_off[0] != 0", "decreasing offsets", "q_aln >= n_aln", "pool shorter than the offsets"])
def test_refusals_leave_the_context_usable(svx_ctx, what):
    cigar, off, start, q_aln, q_ref = [a.copy() for a in case("mixed")[0]]
    kw = {}
    if what == "aln_off[0] != 0":
        off[0] = 1
    elif what == "decreasing offsets":
        off[7] = off[6] - 1
    elif what == "q_aln >= n_aln":
        q_aln[11] = len(start)
    else:
        pool = svx_ctx.dev_array(cigar)
        cigar, kw = pool.ptr, {"n_ops": len(case("mixed")[0][0]) - 1}
    with pytest.raises(_lib.SvxError) as e:
        svx_ctx.cigar_lift(cigar, off, start, q_aln, q_ref, **kw)
    assert e.value.status == _lib.SVX_E_INVALID
    check("mixed", svx_ctx.cigar_lift(*case("mixed")[0]))
