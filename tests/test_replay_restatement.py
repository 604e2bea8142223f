"""The loop of svx_variant_replay as tests/replay_restatement.py states it, where there is no GPU: against brute-force
splicing on every list of up to 3 edits over a window of 6 letters; every status rule at its edge; a homopolymer
deletion written at each of its positions; an MNP against its two SNVs."""
import itertools

from tests import replay_restatement as RR

WIN = b"ACGTCA"


def all_edits(n):
    """Every edit over a window of n letters with a reference length of 0 .. 2 and one of three alleles, some of them not
    inside."""
    return [(s, r, alt) for s in range(n + 1) for r in range(3) for alt in (b"", b"T", b"GG") if r or alt]


def expected_status(win, edits):
    order = all(b[0] >= a[0] + a[1] and b[0] > a[0] for a, b in zip(edits, edits[1:]))
    inside = all(s + r <= len(win) for s, r, _ in edits)
    return 0 if order and inside else 1 if not order else 2


def test_the_loop_against_brute_force_on_every_short_edit_list():
    single = all_edits(len(WIN))
    n = {0: 0, 1: 0, 2: 0}
    for k in range(4):
        for edits in itertools.product(single, repeat=k):
            st, s = RR.replay_job(WIN, edits)
            assert st == expected_status(WIN, edits), edits
            n[st] += 1
            if st == 0:
                assert s == RR.splice_brute(WIN, edits), edits
            else:
                assert s is None
    assert min(n.values()) > 1000


def test_every_status_rule_at_its_edge():
    A = (2, 2, b"T")
    assert RR.replay_job(WIN, [A, (4, 1, b"G")]) == (0, b"ACTGA")        # begins where the one in front ends
    assert RR.replay_job(WIN, [A, (3, 1, b"G")])[0] == 1                   # one byte earlier
    assert RR.replay_job(WIN, [A, (2, 0, b"G")])[0] == 1                   # equal starts
    assert RR.replay_job(WIN, [(2, 0, b"T"), (2, 1, b"G")])[0] == 1        # equal starts behind an insertion
    assert RR.replay_job(WIN, [(2, 0, b"T"), (3, 1, b"G")]) == (0, b"ACTGGCA")
    assert RR.replay_job(WIN, [(4, 2, b"")]) == (0, b"ACGT")               # ends at win_len
    assert RR.replay_job(WIN, [(4, 3, b"")])[0] == 2                       # one byte behind it
    assert RR.replay_job(WIN, [(6, 0, b"T")]) == (0, b"ACGTCAT")           # an insertion at win_len
    assert RR.replay_job(WIN, [(7, 0, b"T")])[0] == 2
    assert RR.replay_job(WIN, [(0, 0, b"T")]) == (0, b"TACGTCA")           # and at 0
    assert RR.replay_job(WIN, [(0, 6, b"")]) == (0, b"")
    assert RR.replay_job(WIN, [A, (3, 9, b"G")])[0] == 1                   # both: 1 wins
    assert RR.replay_job(b"", []) == (0, b"") and RR.replay_job(b"", [(0, 0, b"AC")]) == (0, b"AC")


def test_a_homopolymer_deletion_gives_one_string_at_each_of_its_positions():
    win = b"GCAAAAAATC"
    strings = {RR.replay_job(win, [(at, 2, b"")]) for at in range(2, 7)}
    assert strings == {(0, b"GCAAAATC")}
    assert RR.replay_job(win, [(1, 2, b"")])[1] != b"GCAAAATC" and RR.replay_job(win, [(7, 2, b"")])[1] != b"GCAAAATC"
    # and the same for an insertion into the run, and for the VCF's anchored spelling against the bare one
    assert {RR.replay_job(win, [(at, 0, b"A")])[1] for at in range(2, 9)} == {b"GCAAAAAAATC"}
    assert RR.replay_job(win, [(1, 3, b"C")]) == RR.replay_job(win, [(2, 2, b"")])


def test_an_mnp_equals_its_two_snvs():
    win = b"GATTACA"
    mnp = RR.replay_job(win, [(2, 2, b"CG")])
    assert mnp == RR.replay_job(win, [(2, 1, b"C"), (3, 1, b"G")]) == (0, b"GACGACA")
    pool = win + b"CG"
    res = RR.replay_batch(pool, [0, 0, 0], [7, 7, 7], [0, 1, 3, 4], [2, 2, 3, 2], [2, 1, 1, 1], [7, 7, 8, 7], [2, 1, 1, 1], [0, 0, 1], [1, 2, 2])
    assert res["equal"] == [1, 0, 0] and res["out_len"] == [7, 7, 7] and res["out_off"] == [0, 7, 14, 21]


def test_the_fixture_pair_replays_equal_where_a_key_join_does_not():
    """tests/golden/config1: small.vcf by tests/small_restatement.py against the same alignments after
    tests/shift_restatement.rewrite.  A join of keys leaves 83 records on either side without a partner; every one of the
    825 clusters replays equal, haplotype by haplotype, in straight orientation."""
    import collections
    from tests import smallcmp_cases as S
    rows = []
    for side, text in enumerate(S.fixture_texts()):
        n = 0
        for line in text.splitlines():
            if line.startswith("#"):
                continue
            contig, pos, _, ref, alt, _, _, _, _, gt = line.split("\t")
            p = 0
            while p < min(len(ref), len(alt)) and ref[p] == alt[p]:
                p += 1
            s = 0
            while s < min(len(ref), len(alt)) - p and ref[-1 - s] == alt[-1 - s]:
                s += 1
            assert "|" in gt and S.SEQS[contig][int(pos) - 1:int(pos) - 1 + len(ref)].upper() == ref
            rows.append({"side": side, "c": S.NAMES.index(contig), "start": int(pos) - 1 + p, "ref_len": len(ref) - p - s,
                         "alt": alt[p:len(alt) - s], "haps": [h for h, a in enumerate(gt.split("|")) if a == "1"], "line": line})
            n += 1
        assert n == 929
    lines = [set(r["line"] for r in rows if r["side"] == s) for s in (0, 1)]
    assert len(lines[0] - lines[1]) == len(lines[1] - lines[0]) == 83
    keys = [set((r["c"], r["start"], r["ref_len"], r["alt"]) for r in rows if r["side"] == s) for s in (0, 1)]
    assert len(keys[0] - keys[1]) == len(keys[1] - keys[0]) == 83
    clusters = RR.clusters_of(sorted(rows, key=lambda r: (r["c"], r["start"])), 50)
    assert collections.Counter(len(c) for c in clusters) == {2: 733, 4: 81, 6: 10, 8: 1} and len(clusters) == 825
    widest = 0
    for cl in clusters:
        lo, hi = min(r["start"] for r in cl), max(r["start"] + r["ref_len"] for r in cl)
        widest = max(widest, hi - lo)
        win = S.SEQS[S.NAMES[cl[0]["c"]]][lo:hi].upper().encode()
        for h in (0, 1):
            strings = [RR.replay_job(win, [(r["start"] - lo, r["ref_len"], r["alt"].encode()) for r in cl if r["side"] == s and h in r["haps"]])
                       for s in (0, 1)]
            assert strings[0][0] == strings[1][0] == 0 and strings[0][1] == strings[1][1]   # no conflict, equal straight
    assert widest == 87
