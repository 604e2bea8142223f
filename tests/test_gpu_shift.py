"""svx_indel_shift on the device (svim_asm_amd/csrc/svx_shift.hip) against the loop of tests/shift_restatement.py, element
for element, under the default hand-over, the wave form alone (0) and the lane form alone (INT32_MAX): homopolymer gaps
whose true shift sits at the hand-over and at the edges of the wave form's iteration, each with the limit far away, at the
shift and one below it; period-2 and period-3 repeats longer than two iterations; a tandem insertion whose walk crosses from
the inserted bases to the bases in front; a stop by every rule at step 1, at the hand-over and behind one iteration; events
at the front of their ranges and of the pool with live canaries around every range; all residues of both offsets modulo
16 in mixed case; event counts around the wave and workgroup sizes with every 7th, every and no event undecided; empty
batches; the refusals; poisoned scratch; and 200 random alignments.

The range conditions of the loop (r - i < ref_len, q - i < qry_len, q + L - i < qry_len, r + L - i < ref_len) can only bind
at step 1 — their left sides fall with i —, so the cases that stop on them stop there; i > r and i > q stop at any step."""
import random

import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import shift_restatement as SH

pytestmark = pytest.mark.gpu

INS, DEL = SH.INS, SH.DEL
W = _lib.SHIFT_WAVE_COLS
LS = _lib.SHIFT_LANE_STEPS
FAR = 1 << 30
FORMS = (-1, 0, _lib.SHIFT_LANES_ONLY)


class Aln(object):
    def __init__(self, ref, qry, start=1000, ref_res=None, qry_res=None):
        self.ref, self.qry, self.start, self.ref_res, self.qry_res = bytes(ref), bytes(qry), start, ref_res, qry_res


def pack(alns, events, rng=None, first_at_zero=False):
    """The entry point's arguments.  Every range lies at its residue modulo 16 (random without one) between LIVE canaries:
    the bytes in front repeat the range's first byte and the byte behind its last one, so that a walk that read them would go
    on where the range has ended.  `events`: (alignment, r, q, length, kind, limit)."""
    rng = rng or random.Random(len(alns) * 7 + len(events))
    pool, ref_off, qry_off = bytearray(), [], []

    def place(data, res):
        res = rng.randrange(16) if res is None else res
        pad = (res - len(pool)) % 16
        if pad == 0 and not (first_at_zero and not pool):
            pad = 16
        pool.extend((data[:1] or b"A") * pad)
        at = len(pool)
        pool.extend(data)
        pool.extend(data[-1:] or b"A")
        return at
    for a in alns:
        ref_off.append(place(a.ref, 0 if first_at_zero and not pool else a.ref_res))
        qry_off.append(place(a.qry, a.qry_res))
    ev = list(zip(*events)) if events else [[]] * 6
    return (np.frombuffer(bytes(pool), dtype=np.uint8), np.array(ref_off, dtype=np.uint64), np.array([len(a.ref) for a in alns], dtype=np.uint32),
            np.array(qry_off, dtype=np.uint64), np.array([len(a.qry) for a in alns], dtype=np.uint32),
            np.array([a.start for a in alns], dtype=np.int32), np.array(ev[0], dtype=np.uint32),
            np.array([alns[a].start + r for a, r in zip(ev[0], ev[1])], dtype=np.uint32), np.array(ev[2], dtype=np.uint32),
            np.array(ev[3], dtype=np.uint32), np.array(ev[4], dtype=np.uint8), np.array(ev[5], dtype=np.uint32))


def check(ctx, args, forms=FORMS, expect=None):
    exp = SH.shift_batch(*args)
    if expect is not None:
        assert exp == list(expect)
    try:
        for form in forms:
            ctx.set_shift_lane_steps(form)
            got = ctx.indel_shift(*args)
            assert got.dtype == np.uint32 and got.tolist() == exp, (form, [(e, g, x) for e, (g, x) in enumerate(zip(got.tolist(), exp)) if g != x][:10])
    finally:
        ctx.set_shift_lane_steps(-1)
    return exp


def homopolymer(shift, kind, base=b"A", front=b"G", back=b"T"):
    """(alignment, r, q): a gap of one base at the right end of a run in which it can move `shift` columns."""
    if kind == DEL:
        return Aln(front + base * (shift + 1) + back, front + base * shift + back), len(front) + shift, len(front) + shift
    return Aln(front + base * shift + back, front + base * (shift + 1) + back), len(front) + shift, len(front) + shift


SHIFTS = (0, 1, LS - 1, LS, LS + 1, W - 1, W, W + 1, 2 * W + 1)


def test_homopolymers_at_the_hand_over_and_the_iteration_edges(svx_ctx):
    alns, events, expect = [], [], []
    for kind in (DEL, INS):
        for s in SHIFTS:
            for limit in (FAR, s, s - 1):
                if limit < 0:
                    continue
                a, r, q = homopolymer(s, kind)
                events.append((len(alns), r, q, 1, kind, limit))
                alns.append(a)
                expect.append(min(s, limit))
    check(svx_ctx, pack(alns, events), expect=expect)


def test_repeats_of_period_two_and_three(svx_ctx):
    alns, events = [], []
    for unit in (b"AC", b"ACG"):
        for length in (2, 3, 5):
            n = (2 * W + 40) // len(unit)
            run = unit * n
            for kind in (DEL, INS):
                # the gap at the right end of the run: `length` bases of the repeat deleted, or `length` more of it inserted
                longer = (unit * (n + length))[:len(run) + length]
                ref, qry = (b"GG" + longer + b"TT", b"GG" + run + b"TT") if kind == DEL else (b"GG" + run + b"TT", b"GG" + longer + b"TT")
                events.append((len(alns), 2 + len(run), 2 + len(run), length, kind, FAR))
                alns.append(Aln(ref, qry))
    exp = check(svx_ctx, pack(alns, events))
    assert max(exp) > 2 * W and min(exp) == 0  # (a gap of a whole unit runs the repeat down; another length does not move)


def test_an_insertion_whose_walk_crosses_into_the_bases_in_front(svx_ctx):
    """A tandem copy of the `length` bases in front: steps 1..length compare inserted bases with the bases in front of
    them, the steps behind compare bases in front with bases in front.  A C column on both sides (a stop by X != R) is put
    at steps length - 1, length, length + 1 and far behind."""
    rng = random.Random(5)
    alns, events = [], []
    for length in (2, 3, 5):
        for stop in (length - 1, length, length + 1, 3 * length + 1, None):
            unit = bytes(rng.choice(b"AG") for _ in range(length))
            front = bytearray(b"T" + unit * 8)
            if stop is not None:
                front[len(front) - stop] = ord("C")
            ref, qry = bytes(front) + b"TT", bytes(front) + unit + b"TT"
            events.append((len(alns), len(front), len(front), length, INS, FAR))
            alns.append(Aln(ref, qry))
    check(svx_ctx, pack(alns, events))


def stopped(rule, step, kind):
    """A homopolymer gap of one base that would move far, stopped by `rule` AT `step` (shift = step - 1)."""
    run = W + 60
    a, r, q = homopolymer(run, kind)
    ref, qry = bytearray(a.ref), bytearray(a.qry)
    if rule == "column":
        qry[q - step] = ord("C")
    elif rule == "n_ref":
        ref[r - step] = ord("N")
    elif rule == "n_seq":
        qry[q - step] = ord("n")
    elif rule == "x":  # the column of step `step` holds C on both sides: it matches, and X is still the run's base
        ref[r - step] = qry[q - step] = ord("C")
    elif rule == "i>r":  # the window starts step - 1 bases in front of the gap; SEQ goes on (a live canary in front of the window)
        ref, r = ref[r - (step - 1):], step - 1
    elif rule == "i>q":
        qry, q = qry[q - (step - 1):], step - 1
    return Aln(ref, qry), r, q


def test_a_stop_by_every_rule_at_three_steps(svx_ctx):
    alns, events, expect = [], [], []
    for rule in ("column", "n_ref", "n_seq", "x", "i>r", "i>q"):
        for step in (1, LS, W + 1):
            for kind in (DEL, INS):
                a, r, q = stopped(rule, step, kind)
                events.append((len(alns), r, q, 1, kind, FAR))
                alns.append(a)
                expect.append(step - 1)
    check(svx_ctx, pack(alns, events), expect=expect)


def test_steps_outside_the_lengths_stop_at_once(svx_ctx):
    """Ranges that end in front of what the event needs: the byte behind each range is a live canary."""
    alns, events = [], []
    for kind in (DEL, INS):
        a, r, q = homopolymer(20, kind, back=b"")
        for ref_cut, qry_cut in ((0, 0), (1, 0), (0, 1), (2, 0), (0, 2), (1, 1)):  # (the first one moves: nothing is cut)
            ref, qry = a.ref[:len(a.ref) - ref_cut], a.qry[:len(a.qry) - qry_cut]
            events.append((len(alns), r, q, 1, kind, FAR))
            alns.append(Aln(ref, qry))
        events.append((len(alns), r + 5, q, 1, kind, FAR))   # r behind ref_len
        alns.append(a)
        events.append((len(alns), r, q + 5, 1, kind, FAR))   # q behind qry_len
        alns.append(a)
        events.append((len(alns), r, q, 3, kind, FAR))       # the gap's right end behind its range
        alns.append(a)
    exp = check(svx_ctx, pack(alns, events))
    assert exp.count(20) == 2 and exp.count(0) == len(exp) - 2


def test_the_front_of_a_range_and_of_the_pool(svx_ctx):
    alns, events = [], []
    for kind in (DEL, INS):
        for run in (1, 2, LS + 3, W + 5):  # a run from the range's first byte on: the walk ends by i > r and i > q together
            a, r, q = homopolymer(run, kind, front=b"")
            for r_ev in (1, r):
                events.append((len(alns), r_ev, r_ev, 1, kind, FAR))
                alns.append(a)
            events.append((len(alns), 0, 0, 1, kind, FAR))
            alns.append(a)
    for first_at_zero in (True, False):
        exp = check(svx_ctx, pack(alns, events, first_at_zero=first_at_zero))
        assert exp[0] == 1 and max(exp) == W + 5


def test_every_residue_of_both_offsets_in_mixed_case(svx_ctx):
    rng = random.Random(16)
    alns, events = [], []
    for i in range(16):
        for j in range(16):
            length = 1 + (i + j) % 5
            kind = (DEL, INS)[(i ^ j) & 1]
            unit = bytes(rng.choice(b"ACGT") for _ in range(length))
            n = rng.choice((2, 5, 12, (W + 30) // length))
            less, more = b"GC" + unit * n + b"TA", b"GC" + unit * (n + 1) + b"TA"
            ref, qry = (more, less) if kind == DEL else (less, more)
            case = rng.choice((bytes.lower, bytes.upper, lambda b: bytes(c | 0x20 if rng.random() < 0.5 else c for c in b)))
            events.append((len(alns), 2 + len(unit) * n, 2 + len(unit) * n, length, kind, FAR))
            alns.append(Aln(case(ref), case(qry), ref_res=i, qry_res=j))
    exp = check(svx_ctx, pack(alns, events))
    assert sum(1 for k in exp if k > W) > 20 and sum(1 for k in exp if 0 < k < LS) > 20


@pytest.mark.parametrize("n_ev", (1, 63, 64, 65, 257, 4097))
def test_event_counts_with_every_seventh_event_undecided(svx_ctx, n_ev):
    """Under the default hand-over every 7th event goes to the wave form (the compacted list crosses workgroups from 1793
    events on); under 0 every event does, under INT32_MAX none."""
    kinds = (DEL, INS)
    long_ones = [homopolymer(W + 3, k) for k in kinds] + [homopolymer(LS + 1, k) for k in kinds]
    short_ones = [homopolymer(s, k) for k in kinds for s in (0, 1, 2, LS)]
    alns = [a for a, _, _ in long_ones + short_ones]
    events = []
    for e in range(n_ev):
        if e % 7 == 0:
            j = (e // 7) % len(long_ones)
            events.append((j, long_ones[j][1], long_ones[j][2], 1, kinds[j % 2], FAR))
        else:
            j = e % len(short_ones)
            events.append((len(long_ones) + j, short_ones[j][1], short_ones[j][2], 1, kinds[j // 4], FAR if e % 3 else 1))
    exp = check(svx_ctx, pack(alns, events))
    assert all(k > LS for k in exp[::7]) and all(k <= LS for e, k in enumerate(exp) if e % 7)


def test_empty_batches_and_any_event_order(svx_ctx):
    a, r, q = homopolymer(5, DEL)
    b, rb, qb = homopolymer(W + 9, INS)
    assert len(svx_ctx.indel_shift(*pack([a, b], []))) == 0
    assert len(svx_ctx.indel_shift(*pack([], []))) == 0
    events = [(1, rb, qb, 1, INS, FAR), (0, r, q, 1, DEL, FAR), (1, rb, qb, 1, INS, 7), (0, r, q, 1, DEL, 0), (1, rb - 1, qb - 1, 1, INS, FAR)]
    check(svx_ctx, pack([a, b], events), expect=[W + 9, 5, 7, 0, W + 8])


def test_refusals_leave_the_context_usable(svx_ctx):
    a, r, q = homopolymer(5, DEL)
    good = pack([a], [(0, r, q, 1, DEL, FAR)])
    names = ("bases", "ref_off", "ref_len", "qry_off", "qry_len", "ref_start", "aln", "ref_pos", "qry_pos", "length", "type", "limit")

    def refused(word, **change):
        args = [np.array(x) for x in good]
        for name, value in change.items():
            args[names.index(name)][0] = value
        with pytest.raises(_lib.SvxError) as ei:
            svx_ctx.indel_shift(*args)
        assert ei.value.status == _lib.SVX_E_INVALID and word in str(ei.value), str(ei.value)
        assert svx_ctx.indel_shift(*good).tolist() == [5]
    refused("event 0", aln=1)
    refused("event 0", ref_pos=a.start - 1)
    refused("event 0", type=2)
    refused("event 0", length=0)
    refused("alignment 0", ref_start=-1)
    refused("alignment 0", ref_len=len(good[0]))
    refused("alignment 0", qry_off=len(good[0]) + 1)
    refused("alignment 0", qry_len=len(good[0]))
    with pytest.raises(_lib.SvxError):  # events without alignments
        svx_ctx.indel_shift(good[0], *[x[:0] for x in good[1:6]], *good[6:])
    assert svx_ctx.indel_shift(*good).tolist() == [5]


@pytest.mark.parametrize("fill", (0x00, 0xFF, 0xA5))
def test_poisoned_scratch(svx_ctx, fill):
    made = [homopolymer(s, (DEL, INS)[j & 1]) for j, s in enumerate((0, 3, LS + 2, W + 1, 2 * W + 7))]
    events = [(e % 5, made[e % 5][1], made[e % 5][2], 1, (DEL, INS)[(e % 5) & 1], FAR) for e in range(600)]
    args = pack([a for a, _, _ in made], events)
    svx_ctx.indel_shift(*args)  # (the regions exist and have their size)
    exp = SH.shift_batch(*args)
    try:
        for form in FORMS:
            svx_ctx.set_shift_lane_steps(form)
            svx_ctx.scratch_fill(fill)
            assert svx_ctx.indel_shift(*args).tolist() == exp, form
    finally:
        svx_ctx.set_shift_lane_steps(-1)


def test_random_cases(svx_ctx):
    """200 alignments of random two- to five-letter strings with repeats, three events each with ANY r, q, length and limit
    — inside the ranges or not."""
    rng = random.Random(2024)
    for call in range(10):
        alns, events = [], []
        for _ in range(20):
            alphabet = rng.choice((b"AC", b"AC", b"ACGT", b"ACgtN", b"aC"))
            unit = bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, 4)))
            n = rng.choice((3, 10, 40, 300))
            ref = bytearray(bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 6))) + unit * n)
            length = rng.randrange(1, 7)
            kind = rng.choice((DEL, INS))
            if kind == DEL:
                qry = ref[:len(ref) - min(length, len(ref))]
                r, q = len(qry), len(qry)
            else:
                qry = ref + (unit * 8)[:length]
                r, q = len(ref), len(ref)
            for _ in range(rng.randrange(0, 3)):  # a few injuries
                s = rng.choice((ref, qry))
                if s:
                    s[rng.randrange(len(s))] = rng.choice(b"ACGTN")
            ref, qry = ref + b"TG", qry + b"TG"
            events.append((len(alns), r, q, length, kind, rng.choice((FAR, FAR, rng.randrange(0, 400)))))
            events.append((len(alns), max(0, r - rng.randrange(0, 4)), max(0, q - rng.randrange(0, 4)), rng.randrange(1, 7), kind, FAR))
            events.append((len(alns), rng.randrange(0, len(ref) + 3), rng.randrange(0, len(qry) + 3), rng.randrange(1, 7), rng.choice((DEL, INS)), rng.randrange(0, 1000)))
            alns.append(Aln(ref, qry, start=rng.randrange(0, 1 << 20)))
        check(svx_ctx, pack(alns, events, rng=rng))
