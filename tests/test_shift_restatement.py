"""tests/shift_restatement.py against brute force and on the fixture (no GPU): the loop of include/svx.h gives, for an
isolated gap, exactly the placements that leave the haplotype unchanged; it is idempotent; every stop rule stops where it
should; and tests/golden/config1 moves as DESIGN.md §3.19 says."""
import os
import random

from tests import merge_restatement as MR, shift_restatement as SH, small_restatement as SR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config1")
INS, DEL = SH.INS, SH.DEL


def isolated(rng, kind, length, alphabet="AC"):
    """(ref, qry, p): one gap of `length` at reference offset p > 0 of a random string; r = q = p."""
    n = rng.randrange(length + 2, 24)
    ref = "".join(rng.choice(alphabet) for _ in range(n))
    if kind == DEL:
        p = rng.randrange(1, n - length + 1)
        return ref, ref[:p] + ref[p + length:], p
    p = rng.randrange(1, n + 1)
    return ref, ref[:p] + "".join(rng.choice(alphabet) for _ in range(length)) + ref[p:], p


def reproduces(ref, qry, p, s, kind, length):
    """Does the gap placed s columns to the left (its bases read from SEQ there) give the same query?"""
    at = p - s
    if kind == DEL:
        return ref[:at] + ref[at + length:] == qry
    return ref[:at] + qry[at:at + length] + ref[at:] == qry


def test_isolated_gaps_against_brute_force():
    rng = random.Random(1951)
    moved = 0
    for case in range(4000):
        kind, length = rng.choice((INS, DEL)), rng.randrange(1, 5)
        ref, qry, p = isolated(rng, kind, length)
        limit = p - 1 if case % 3 else rng.randrange(0, p)
        k = SH.shift_of(ref.encode(), qry.encode(), p, p, length, kind, limit)
        assert 0 <= k <= limit
        # every placement 0..k reproduces the query, and none beyond k (inside the limit, and one past it where there is room)
        for s in range(0, p):
            if s <= k:
                assert reproduces(ref, qry, p, s, kind, length), (ref, qry, p, kind, length, k, s)
            elif s <= limit:
                assert not reproduces(ref, qry, p, s, kind, length), (ref, qry, p, kind, length, k, s)
        # a second walk from the new position does not move
        if k < limit:  # (the bases stopped it, not the limit)
            again = SH.shift_of(ref.encode(), qry.encode(), p - k, p - k, length, kind, p - k - 1)
            assert again == 0, (ref, qry, p, kind, length, k, again)
        moved += k > 0
    assert moved > 500


def test_every_stop_rule():
    #       0123456789
    ref = b"GTAAAAAAAC"
    qry = b"GTAAAAAC"  # two A deleted, placed at the right end of the run ref[2:9]: r = q = 7
    assert SH.shift_of(ref, qry, 7, 7, 2, DEL, 100) == 5           # down to the T in front of the run
    assert SH.shift_of(ref, qry, 7, 7, 2, DEL, 3) == 3             # a binding limit
    assert SH.shift_of(ref, qry, 7, 7, 2, DEL, 0) == 0
    assert SH.shift_of(b"GTAACAAAAC", b"GTAACAAC", 7, 7, 2, DEL, 100) == 2                    # X != R at the C
    assert SH.shift_of(b"GTAAAAAAAC", b"GTAAGAAC", 7, 7, 2, DEL, 100) == 2                    # a mismatching column (q = 4)
    assert SH.shift_of(b"GTAANAAAAC", b"GTAANAAC", 7, 7, 2, DEL, 100) == 2                    # N in both: outside ACGT
    assert SH.shift_of(b"GTAAAAAANC", b"GTAAAAAC", 7, 7, 2, DEL, 100) == 0                    # X of step 1 is the N at ref[7 + 2 - 1]
    assert SH.shift_of(b"GTAAAAANAC", b"GTAAAAAC", 7, 7, 2, DEL, 100) == 1                    # X of step 2
    assert SH.shift_of(b"gtaaaaaaac", b"GTAAAAAC", 7, 7, 2, DEL, 100) == 5                    # lower case equals upper case
    assert SH.shift_of(b"GTaAaAAAAC", b"gtAaAaAc", 7, 7, 2, DEL, 100) == 5
    # an insertion of one unit of a period-2 repeat: the walk crosses from the inserted bases to the bases in front
    ref, qry = b"GGCACACAT", b"GGCACACACAT"
    assert SH.shift_of(ref, qry, 8, 8, 2, INS, 100) == 6
    assert SH.shift_of(ref, qry, 8, 8, 2, INS, 100) == max(s for s in range(8) if reproduces(ref.decode(), qry.decode(), 8, s, INS, 2))
    # indices: i > r, i > q, and ranges shorter than the event says
    assert SH.shift_of(b"AAAA", b"TAAAA", 3, 4, 1, DEL, 100) == 3  # i <= r binds (SEQ has one base more in front)
    assert SH.shift_of(b"TTAAAA", b"AAA", 5, 2, 1, DEL, 100) == 2  # i <= q binds
    assert SH.shift_of(b"AAAA"[:3], b"AAA", 3, 3, 1, DEL, 100) == 0  # r + L - i outside ref_len
    assert SH.shift_of(b"AAAA", b"AAAAA"[:4], 4, 4, 1, INS, 100) == 0  # q + L - i outside qry_len
    assert SH.shift_of(b"AAA", b"AAAAAA", 5, 5, 1, INS, 100) == 0  # r - i outside ref_len at step 1


def test_rewrite_moves_the_cigar_and_nothing_else():
    seqs = {"c": "GTAAAAAAACGG"}
    aln = ("c", 0, [(0, 7), (2, 2), (0, 3)], "GTAAAAACGG")
    (out,), moved = SH.rewrite([aln], seqs, 40)
    assert out == ("c", 0, [(0, 2), (2, 2), (0, 8)], "GTAAAAACGG") and moved == [5]
    # a second gap one aligned column behind the first does not move; a gap of min_sv_size stays and bounds its neighbour
    aln = ("c", 0, [(0, 4), (2, 1), (0, 1), (2, 1), (0, 5)], "GTAAAAACGG")
    assert [k for _, k in SH.shifts_of(aln, seqs, 40)] == [2, 0]
    aln = ("c", 0, [(0, 4), (2, 2), (0, 2), (2, 1), (0, 3)], "GTAAAACGG")
    assert SH.shifts_of(aln, seqs, 2) == [(3, 1)]
    assert SH.rewrite([("c", 0, [(0, 12)], "")], seqs, 40) == ([("c", 0, [(0, 12)], "")], [])


def test_the_binding_states_the_header_constants():
    import re
    from svim_asm_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLD), "..", "..", "include", "svx.h")).read()
    value = lambda name: int(re.search(r"^#define %s (\d+)$" % name, header, flags=re.M).group(1))
    assert _lib.SHIFT_WAVE_COLS == value("SVX_SHIFT_WAVE_COLS") and _lib.SHIFT_WAVE_COLS % 64 == 0
    assert _lib.SHIFT_LANE_STEPS == value("SVX_SHIFT_LANE_STEPS") >= 2
    assert _lib.SHIFT_LANES_ONLY == 2 ** 31 - 1 and (SH.INS, SH.DEL) == (value("SVX_SIG_INS"), value("SVX_SIG_DEL"))


def fixture_figures(path, seqs):
    shifts = [k for a in SR.alignments_of(path) for _, k in SH.shifts_of(a, seqs, 40)]
    return len([k for k in shifts if k]), len(shifts), sum(shifts), max(shifts)


def test_config1_figures():
    seqs = MR.read_fasta(os.path.join(GOLD, "ref.fa"))
    assert fixture_figures(os.path.join(GOLD, "hap1.bam"), seqs) == (52, 192, 66, 3)
    assert fixture_figures(os.path.join(GOLD, "hap2.bam"), seqs) == (44, 202, 61, 5)
