"""The lift-over's definition where there is no GPU: the loop of tests/lift_restatement.py on hand-written alignments —
the consequences include/svx.h spells out —, the host baseline of tools/lift_probe.py against it, and the argument checks
of Context.cigar_lift / cover_locate that need no device."""
import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import lift_restatement as LR

M, I, D, N, S, H, P, EQ, X = range(9)


def test_the_states_by_hand():
    ops = [(H, 4), (S, 3), (M, 10), (I, 2), (D, 3), (EQ, 5), (N, 7), (X, 1), (I, 6), (S, 9)]  # from 100: M 100-109, D 110-112, = 113-117, N 118-124, X 125
    assert LR.lift(ops, 100, 99) == (0, LR.OUTSIDE)
    assert LR.lift(ops, 100, 100) == (3, LR.ALIGNED)       # the soft clip counts, the hard clip does not
    assert LR.lift(ops, 100, 109) == (12, LR.ALIGNED)
    assert LR.lift(ops, 100, 110) == (15, LR.DELETED)      # the bases inserted in front of the D lie to the left
    assert LR.lift(ops, 100, 112) == (15, LR.DELETED)
    assert LR.lift(ops, 100, 113) == (15, LR.ALIGNED)
    assert LR.lift(ops, 100, 124) == (20, LR.DELETED)      # N as D
    assert LR.lift(ops, 100, 125) == (20, LR.ALIGNED)
    assert LR.lift(ops, 100, 126) == (21, LR.END)          # behind the last reference-consuming op: trailing I and S not counted
    assert LR.lift(ops, 100, 127) == (0, LR.OUTSIDE)


def test_ops_that_consume_nothing_and_alignments_without_reference_bases():
    assert LR.lift([(M, 5), (P, 9), (11, 7), (M, 5)], 0, 5) == (5, LR.ALIGNED)   # P and a code above 8
    assert LR.lift([(M, 5), (D, 2)], 10, 17) == (5, LR.END)
    for ops in ([], [(S, 5), (I, 7), (H, 2)]):
        for r in (9, 10, 11):
            assert LR.lift(ops, 10, r) == (0, LR.OUTSIDE)


def test_locate_takes_the_longest_reach_and_the_first_among_equals():
    ivs = [(10, 90), (20, 95), (20, 95), (50, 60)]
    assert LR.locate([ivs, []], [(25, 95), (55, 96), (5, 6), (10, 90), (19, 91)]) == [[1, LR.NONE, LR.NONE, 0, LR.NONE], [LR.NONE] * 5]


def test_the_probes_host_baseline_equals_the_loop():
    from tools import lift_probe
    batch = lift_probe.synthetic_batch(30000, 4000, per_alignment=100)
    cigar, aln_off, ref_start, q_aln, q_ref = batch
    assert len(cigar) == 30000 and aln_off.tolist() == list(range(0, 30001, 100)) and len(q_aln) == len(q_ref) == 4000
    # some queries exactly at an alignment's end and first base
    ref_len = np.array([sum(int(w) >> 4 for w in cigar[a * 100:(a + 1) * 100] if int(w) & 15 in (M, D)) for a in range(300)])
    q_ref[:50] = ref_start[q_aln[:50]].astype(np.int64) + ref_len[q_aln[:50]]
    q_ref[50:60] = ref_start[q_aln[50:60]]
    query, state = lift_probe.on_host(*batch)
    exp_query, exp_state = LR.lift_batch(*batch)
    assert state.tolist() == exp_state and query.tolist() == exp_query
    assert {LR.OUTSIDE, LR.ALIGNED, LR.DELETED, LR.END} == set(exp_state)


def test_the_bindings_refuse_mismatched_arrays_before_any_device_call():
    ctx = _lib.Context.__new__(_lib.Context)  # (no device: the checks below come first)
    with pytest.raises(_lib.SvxError):
        ctx.cigar_lift(np.zeros(3, np.uint32), [0, 3], [5, 6], [0], [7])          # two starts for one alignment
    with pytest.raises(_lib.SvxError):
        ctx.cigar_lift(np.zeros(3, np.uint32), [0, 3], [5], [0, 0], [7])          # a position without its alignment
    with pytest.raises(_lib.SvxError):
        ctx.cigar_lift(np.zeros(2, np.uint32), [0, 3], [5], [0], [7])             # fewer words than the offsets say
    with pytest.raises(_lib.SvxError):
        ctx.cover_locate([1, 2], [3], [0, 2], [1], [2])
    empty = ctx.cigar_lift(np.zeros(0, np.uint32), [0], np.zeros(0, np.int32), [], [])
    assert len(empty[0]) == len(empty[1]) == 0
    assert ctx.cover_locate([], [], [0], [1, 2], [3, 4]).shape == (0, 2)
