"""The case table of the edit distance (tests/editdist_cases.py) where there is no GPU: with the oracle's full-matrix
distance and the restated plan (tests/editdist_restatement.py) alone, the table holds every state it claims — a
construction that misses its intended distance fails here, not on the device —; a table without one of its cap cases
fails; the layouts put the sequences where they say; the recipes' expected strings equal what Python's own
bytes.upper() / translate() make of the slices; the restated constants are those of the kernel source."""
import os
import re

import numpy as np
import pytest

from tests import editdist_cases as E
from tests import editdist_restatement as R

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svim_asm_amd", "csrc", "svx_editdist.hip")
EXACT = R.EXACT
# which term can decide the first-stage cap under each setting, for sequences of at most MAX_LEN bytes: (la + lb) / 32
# stays below 1024 (it needs 32 768 bytes), and 48 lies below the floor of 64
CAN_BIND = {1024: ("floor", "length"), 48: ("wfa_cap",), 100: ("floor", "length", "wfa_cap")}
FAMILY_SIZES = {"cap_length": 15, "cap_wfa": 9, "cap_lendiff": 8, "batches": 9, "clipped": 11, "runs": 3 * len(E.RUNS) + 1,
                "alphabets": 18, "bands": 15, "strips": 20}


@pytest.fixture(scope="module")
def ref():
    return E.reference()


def sigma_of_pattern(a, b):
    return len(set(a if len(a) >= len(b) else b))


def check_table(cases, ref):
    """Every state the table claims, from (a, b), the reference distance and the restated plan."""
    rows = [(n, len(a), len(b), ref[n], a, b) for n, (a, b) in cases.items()]

    def some(what, pred):
        assert any(pred(*row) for row in rows), what

    # the first-stage cap's edges, for each term that can decide it, on pairs of equal lengths (substitutions alone)
    for wfa_cap, bounds in CAN_BIND.items():
        for bound in bounds:
            for delta in (-1, 0, 1):
                some("wfa_cap %d, %s decides, d = cap%+d" % (wfa_cap, bound, delta),
                     lambda n, la, lb, d, a, b: la == lb and R.binding(la, lb, EXACT, wfa_cap) == bound
                     and d == R.first_stage_cap(la, lb, EXACT, wfa_cap) + delta)
    for k in E.K_BINDING:
        assert k in E.FIXED_KS
        for delta in (-1, 0, 1):
            some("threshold %d decides, d = k%+d" % (k, delta),
                 lambda n, la, lb, d, a, b: k < R.first_stage_cap(la, lb, EXACT, 1024)
                 and R.binding(la, lb, k, 1024) == "k" and d == k + delta)
    # ... on each number of strips when the lengths decide
    for n_strips in (1, 2, 3):
        for delta in (-1, 0, 1):
            some("%d strips, d = cap%+d" % (n_strips, delta),
                 lambda n, la, lb, d, a, b: la == lb and R.strips(la, lb) == n_strips
                 and R.binding(la, lb, EXACT, 1024) == "length" and d == R.first_stage_cap(la, lb, EXACT, 1024) + delta)
    # the lengths differ by cap and cap + 1 (the wavefront kernel's early exit), on one strip and on two
    for n_strips in (1, 2):
        for delta in (0, 1):
            some("%d strips, |n - m| = cap%+d" % (n_strips, delta),
                 lambda n, la, lb, d, a, b: R.strips(la, lb) == n_strips
                 and abs(la - lb) == R.first_stage_cap(la, lb, EXACT, 1024) + delta)
    some("indels and substitutions add up to the cap",
         lambda n, la, lb, d, a, b: 0 < abs(la - lb) < d == R.first_stage_cap(la, lb, EXACT, 1024))
    # more than 64, 128 and 192 diagonals within the first stage: 2 d + 1 of them at distance d
    for edge in (32, 64, 96):
        for d_want in (edge - 1, edge, edge + 1):
            some("d = %d resolved by the first stage, with indels" % d_want,
                 lambda n, la, lb, d, a, b: d == d_want and la != lb and d <= R.first_stage_cap(la, lb, EXACT, 1024))
    some("diagonals clipped: a side shorter than the distance",
         lambda n, la, lb, d, a, b: min(la, lb) < d <= R.first_stage_cap(la, lb, EXACT, 1024))
    some("... on a's side", lambda n, la, lb, d, a, b: la < d <= 64 and la < lb)
    some("... on b's side", lambda n, la, lb, d, a, b: lb < d <= 64 and lb < la)
    # alphabets of the pattern (the longer side, or a at a tie)
    for sigma in (16, 17, 255, 256):
        for n_strips in (1, 2):
            some("sigma %d on %d strips" % (sigma, n_strips),
                 lambda n, la, lb, d, a, b: sigma_of_pattern(a, b) == sigma and R.strips(la, lb) == n_strips and d > 0)
    for lo in (16, 255):
        some("%d symbols in a, %d in b, equal lengths" % (lo, lo + 1),
             lambda n, la, lb, d, a, b: la == lb and len(set(a)) == lo and len(set(b)) == lo + 1 and d > 0)
        some("%d symbols in a, %d in b, b one byte longer" % (lo, lo + 1),
             lambda n, la, lb, d, a, b: la + 1 == lb and len(set(a)) == lo and len(set(b)) == lo + 1)
    some("a 16-symbol pattern meets text bytes it lacks",
         lambda n, la, lb, d, a, b: la > lb and len(set(a)) == 16 and set(b) - set(a))
    for sigma in (17, 255):
        some("a %d-symbol pattern whose lowest byte meets only a byte it lacks" % sigma,
             lambda n, la, lb, d, a, b: la == lb and len(set(a)) == sigma and d >= 200
             and all(y not in set(a) for x, y in zip(a, b) if x == min(a)) and all(x == y or x == min(a) for x, y in zip(a, b)))
    for n_strips in (1, 2, 3):
        some("%d strips" % n_strips, lambda n, la, lb, d, a, b: R.strips(la, lb) == n_strips and d > 0)
    # the exact request's band rounds on multi-strip pairs, plain DNA and rich
    for n_strips in (2, 3):
        for d_want in (R.FIRST_BAND, R.FIRST_BAND + 1, R.FIRST_BAND * R.WIDEN, R.FIRST_BAND * R.WIDEN + 1):
            some("%d strips, d = %d" % (n_strips, d_want),
                 lambda n, la, lb, d, a, b: R.strips(la, lb) == n_strips and d == d_want and sigma_of_pattern(a, b) <= 16)
        for band in (R.FIRST_BAND, R.FIRST_BAND * R.WIDEN):
            some("%d strips, lengths differ by more than %d" % (n_strips, band),
                 lambda n, la, lb, d, a, b: R.strips(la, lb) == n_strips and band < abs(la - lb) <= band * R.WIDEN)
    for band in (R.FIRST_BAND, R.FIRST_BAND * R.WIDEN):
        some("rich alphabet, multi-strip, d > %d" % band,
             lambda n, la, lb, d, a, b: R.strips(la, lb) > 1 and sigma_of_pattern(a, b) > 16 and band < d <= band * R.WIDEN)
    some("unrelated multi-strip sequences", lambda n, la, lb, d, a, b: R.strips(la, lb) > 1 and 2 * d > min(la, lb))
    # strip geometry: the pattern on the strip edge and one past it, the text on the stream's 32-column words
    for m in (R.STRIP, R.STRIP + 1, 2 * R.STRIP, 2 * R.STRIP + 1):
        for short in (0, 1, 31, 32, 33):
            some("m = %d, n = m - %d" % (m, short), lambda n, la, lb, d, a, b: max(la, lb) == m and min(la, lb) == m - short)
    # runs of exactly r matching bytes: at the sequences' ends, inside, as the common prefix
    for r in E.RUNS:
        for where in ("end", "mid", "head"):
            a, b = cases["runs/r%d_%s" % (r, where)]
            diff = np.nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))[0].tolist()
            x = len(a) - r if where == "end" else 5
            assert len(a) == len(b) and diff == {"end": [x - 1], "mid": [x - 1, x + r], "head": [r]}[where], (r, where)
    a, b = cases["runs/chain"]
    diff = np.nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))[0]
    assert np.diff(np.concatenate(([-1], diff, [len(a)]))).tolist() == [r + 1 for r in E.RUNS]
    for name, (a, b) in cases.items():
        assert max(len(a), len(b)) <= E.MAX_LEN, name


def test_constructions_give_their_intended_distance(ref):
    assert len(E.INTENDED) > 100
    for name, d in E.INTENDED.items():
        assert ref[name] == d, name


def test_the_table_holds_every_state(ref):
    check_table(E.CASES, ref)
    assert {f: sum(1 for n in E.NAMES if E.FAMILY[n] == f) for f in E.FAMILIES} == FAMILY_SIZES


@pytest.mark.parametrize("name", ["cap_length/L1000_subs64", "cap_wfa/L4200_subs100", "cap_lendiff/L4200_cut255",
                                  "bands/L8300_subs257", "alphabets/sigma255_against_256_L600_b_longer"])
def test_a_table_without_one_of_its_cases_fails(ref, name):
    """(cap_length/L1000_subs64 is the d == cap case of the floor of 64.)"""
    less = {n: c for n, c in E.CASES.items() if n != name}
    assert len(less) == len(E.CASES) - 1
    with pytest.raises(AssertionError):
        check_table(less, ref)


def test_thresholds_split_the_table(ref):
    """Every threshold the device module asks with, below the largest distance, has pairs on both sides."""
    d = np.array([ref[n] for n in E.NAMES])
    ks = E.thresholds(ref)
    assert set(E.FIXED_KS) <= set(ks) and all(x in ks for v in set(d.tolist()) for x in (v - 1, v, v + 1) if x >= 0)
    for k in ks:
        if k < d.max():
            assert (d <= k).any() and (d > k).any(), k


def test_layouts():
    names = E.NAMES
    pairs = [E.CASES[n] for n in names]
    for adversarial in (True, False):
        pool, ao, al, bo, bl = E.layout({n: E.CASES[n] for n in names}, adversarial=adversarial)
        pool = pool.tobytes()
        assert {(x % 8, y % 8) for x, y in zip(ao, bo)} == {(x, y) for x in range(8) for y in range(8)}
        spans = sorted([(o, l) for o, l in zip(ao, al)] + [(o, l) for o, l in zip(bo, bl)])
        assert all(o + l + E.TAIL <= o2 for (o, l), (o2, _) in zip(spans, spans[1:]))
        assert len(pool) >= spans[-1][0] + spans[-1][1] + 2 * E.TAIL
        for (a, b), xo, xl, yo, yl in zip(pairs, ao, al, bo, bl):
            assert pool[xo:xo + xl] == a and pool[yo:yo + yl] == b
            ta, tb = pool[xo + xl:xo + xl + E.TAIL], pool[yo + yl:yo + yl + E.TAIL]
            if not adversarial:
                assert ta == tb == bytes(E.TAIL)
                continue
            # the bytes behind the shorter side continue its match with the longer one; equal ends have equal tails
            if xl < yl:
                assert ta[:yl - xl] == b[xl:xl + E.TAIL]
            if yl < xl:
                assert tb[:xl - yl] == a[yl:yl + E.TAIL]
            if xl == yl >= E.TAIL and a[-E.TAIL:] == b[-E.TAIL:]:
                assert ta == tb == a[-E.TAIL:]
    pool, ao, al, bo, bl = E.layout(pairs, residues="packed")
    assert pool.tobytes() == b"".join(a + b for a, b in pairs) + bytes(pool[-E.TAIL:]) and ao[0] == 0
    assert all(x + l == y for x, l, y in zip(ao, al, bo)) and all(y + l == x for y, l, x in zip(bo, bl, ao[1:]))
    rn, rp, rr = E.runs_at_every_residue()
    pool, ao, al, bo, bl = E.layout(rp, residues=rr)
    assert len(rp) == 64 * FAMILY_SIZES["runs"] and [(x % 8, y % 8) for x, y in zip(ao, bo)] == rr
    assert sorted(set(rr)) == [(x, y) for x in range(8) for y in range(8)]


def plain_python(pool, pieces):
    """assemble() once more with bytes.upper() and bytes.translate()."""
    out = b""
    for off, ln, rep, flags in pieces:
        s = pool[off:off + ln]
        if flags & R.UPPER:
            s = s.upper()
        if flags & R.REVCOMP:
            s = s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
        out += s * rep
    return out


def test_recipes_hold_every_form():
    pool = E.HAP_POOL.tobytes()
    assert pool[:256] == bytes(range(256)) and len(pool) == 256 + 4096
    iupac = pool[256:]
    assert any(c in iupac for c in b"acgt") and any(c in iupac for c in b"ACGT") and any(c in iupac for c in b"nryNRY")
    H = E.HAP_CASES
    for name, pieces in H.items():
        assert all(off + ln <= len(pool) for off, ln, _, _ in pieces), name
        assert E.hap_expected(name) == plain_python(pool, pieces), name
    forms = {tuple((ln > 0, min(rep, 2)) for _, ln, rep, _ in pieces) for pieces in H.values()}
    for pos in range(3):   # len > 0, repeat = 0 in each position, its neighbours present
        assert tuple((True, 0 if q == pos else 1) for q in range(3)) in forms
    assert any(p[1][1] == 0 and p[1][2] == 3 and p[0][1] and p[2][1] for p in H.values())
    assert all(any(p[1][2] == 3 and p[1][3] == f and p[1][1] > 1 for p in H.values()) for f in (R.REVCOMP, R.REVCOMP | R.UPPER))
    assert any(p[1][1:3] == (1, 65535) for p in H.values()) and any(p[1][1:3] == (700, 4) and p[0][1] and p[2][1] for p in H.values())
    assert any(all(pc == (0, 0, 0, 0) for pc in p) for p in H.values())
    assert any(sum(1 for pc in p if pc[1] and pc[2]) == 3 for p in H.values())
    assert {p[0][1] for p in H.values()} >= {255, 256, 257}
    for name in E.HAP_LENGTH_FORMS:
        assert len(E.hap_expected(name)) == {"len1_repeat65535": 65535, "len700_repeat4": 90 + 2800 + 110}[name]
    # all 256 bytes under each flag combination differ from the plain slice exactly where they should
    raw = bytes(range(256))
    got = {f: E.hap_expected("all_bytes_flags%d" % f) for f in (0, 1, 2, 3)}
    assert got[0] == raw
    assert [i for i in range(256) if got[1][i] != raw[i]] == list(range(ord("a"), ord("z") + 1))
    assert all(got[1][c] == c - 32 for c in range(ord("a"), ord("z") + 1)) and got[1][ord("`")] == ord("`") and got[1][ord("{")] == ord("{")
    back = {f: got[f][::-1] for f in (2, 3)}
    assert {c for c in range(256) if back[2][c] != raw[c]} == set(b"ACGT")
    assert {c for c in range(256) if back[3][c] != raw[c]} == set(range(ord("a"), ord("z") + 1)) | set(b"ACGT")
    assert [back[3][c] for c in b"acgtACGTn"] == list(b"TGCATGCAN") and [back[2][c] for c in b"acgtACGTn"] == list(b"acgtTGCAn")
    # a repeated reverse complement repeats the reversed slice, it does not reverse the repeats
    off, ln, rep, _ = H["revcomp_repeat3"][1]
    assert pool[off:off + ln] != pool[off:off + ln][::-1]
    assert E.hap_expected("revcomp_repeat3")[90:90 + 3 * ln] == 3 * plain_python(pool, [(off, ln, 1, R.REVCOMP)])


def test_restated_plan():
    assert R.first_stage_cap(1000, 1000, EXACT, 1024) == 64 and R.first_stage_cap(4200, 4200, EXACT, 1024) == 262
    assert R.first_stage_cap(4200, 4200, 200, 1024) == 200 and R.first_stage_cap(4200, 4200, 300, 1024) == 262
    assert R.first_stage_cap(4200, 4200, 0xFFFFFFFE, 48) == 48 and R.first_stage_cap(40000, 40000, EXACT, 1024) == 1024
    assert R.first_band(4200, 4200, EXACT, 1024, True) is None and R.first_band(4200, 4200, EXACT, 1024, False) == 524
    assert R.first_band(1000, 1000, EXACT, 1024, False) == 256 and R.first_band(4200, 4200, EXACT, 0, False) == 256
    assert R.first_band(4200, 4200, 300, 1024, False) == 300 and R.first_band(4200, 4200, 200, 1024, False) is None
    assert (R.strips(4096, 1), R.strips(1, 4097), R.strips(8193, 8193)) == (1, 2, 3)


def test_constants_are_those_of_the_kernel_source():
    """A retune of the hand-over point or the band schedule has to move the table in the same change."""
    text = open(SOURCE).read()
    assert re.findall(r"constexpr uint32_t kStripRows = (\d+) \* (\d+);", text) == [(str(R.BLOCK), str(R.STRIP // R.BLOCK))]
    assert re.findall(r"std::max<uint64_t>\((\d+), \(\(uint64_t\)a_len\[i\] \+ b_len\[i\]\) / (\d+)\)", text) == \
        [(str(R.FLOOR), str(R.LENGTH_SHARE))]
    assert re.findall(r"exact_of\(i\) \? (\d+)u : kmax_of\(i\)", text) == [str(R.FIRST_BAND)]
    assert re.findall(r"std::max<uint32_t>\((\d+)u, (\d+) \* lst_band\[w\]\)", text) == [(str(R.FIRST_BAND), "2")]
    assert re.findall(r"band_of\[i\] \* (\d+);", text) == [str(R.WIDEN)]
