"""The case table of the edit distance (svim_asm_amd/csrc/svx_editdist.hip): pairs placed on the values where the host
plan ed_run and the kernels k_edit_wfa / k_edit_myers<16|256> change their mind, and haplotype recipes for every form
k_hap_build reads.  Built deterministically from one seeded generator; tests/test_editdist_cases.py shows (with the
oracle's full-matrix distance and tests/editdist_restatement.py alone) that every state the families name is in the
table, tests/test_gpu_editdist_cases.py holds the device to it.

CASES: name -> (a, b); FAMILY: name -> family; INTENDED: name -> the distance the construction aims at (only where it
aims at one; the CPU module holds the oracle to it).  No sequence is longer than 8400 bytes (three strips), so the
oracle's full matrix stays affordable."""
import functools

import numpy as np

from tests import editdist_restatement as R

SEED = 0xED17
MAX_LEN = 8400
TAIL = 16                      # bytes behind a sequence that the layout chooses, and behind the pool's last one
WFA_CAPS = (1024, 48, 100)     # svx_ctx_set_edit_wavefront_cap settings the cap edges are built for
K_BINDING = (48, 64, 100)      # thresholds the cap edges are also built for (k binds the first-stage cap)
FIXED_KS = (0, 1, 47, 48, 49, 63, 64, 65, 99, 100, 101, 127, 128, 129, 255, 256, 257, 261, 262, 263, 517, 518, 519,
            1023, 1024, 1025, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE)
RUNS = (0, 1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 519, 520, 521, 1023, 1024, 1025)
FAMILIES = ("cap_length", "cap_wfa", "cap_lendiff", "batches", "clipped", "runs", "alphabets", "bands", "strips")

_DNA = np.frombuffer(b"ACGT", np.uint8)
_NEXT = np.arange(1, 257, dtype=np.uint16).astype(np.uint8)        # any byte -> the next value ...
for _x, _y in zip(b"ACGT", b"CGTA"):
    _NEXT[_x] = _y                                                 # ... a base -> the next base


def nxt(s):
    """Every byte of s replaced by the next one."""
    return _NEXT[np.frombuffer(s, np.uint8)].tobytes() if s else b""


def dna(rng, n):
    return _DNA[rng.integers(0, 4, n)].tobytes()


def spread(length, d):
    """d distinct, evenly spaced positions of a sequence of `length`."""
    assert 0 <= d <= length
    return [(2 * i + 1) * length // (2 * d) for i in range(d)]


def subs(a, d):
    """a with exactly d substitutions at evenly spaced positions, each to the next base."""
    s = np.frombuffer(a, np.uint8).copy()
    at = spread(len(a), d)
    s[at] = _NEXT[s[at]]
    return s.tobytes()


def dels(a, d):
    """a without d single bases at evenly spaced positions."""
    keep = np.ones(len(a), bool)
    keep[spread(len(a), d)] = False
    return np.frombuffer(a, np.uint8)[keep].tobytes()


def cut(a, at, n):
    """a without the block a[at : at + n]."""
    assert at + n <= len(a)
    return a[:at] + a[at + n:]


def mixed(a, n_dels, n_subs):
    """a with n_dels single-base deletions in its first half and n_subs substitutions in its second (apart, so that no
    substitution is absorbed by a deletion next to it)."""
    h = len(a) // 2
    return dels(a[:h], n_dels) + subs(a[h:], n_subs)


def _with_alphabet(rng, sigma, n, alphabet=None):
    """n bytes over exactly sigma distinct values (each occurs), and the values."""
    alphabet = rng.permutation(256)[:sigma].astype(np.uint8) if alphabet is None else alphabet
    assert len(alphabet) == sigma <= n
    s = np.concatenate((alphabet, alphabet[rng.integers(0, sigma, n - sigma)]))
    return rng.permutation(s).tobytes(), alphabet


def _build():
    rng = np.random.default_rng(SEED)
    cases, family, intended = {}, {}, {}

    def add(fam, name, a, b, d=None):
        name = fam + "/" + name
        assert name not in cases and max(len(a), len(b)) <= MAX_LEN
        cases[name], family[name] = (bytes(a), bytes(b)), fam
        if d is not None:
            intended[name] = d

    base = {L: dna(rng, L) for L in (1000, 1500, 2048, 4200, 8300)}

    # 1. first-stage cap decided by the lengths (or their floor of 64): d = cap - 1, cap, cap + 1 on one, two and three
    #    strips.  (L = 1500: the lengths' share, 93, is also what decides under a dedicated cap of 100.)
    for L in (2048, 4200, 8300, 1000, 1500):
        cap = R.length_bound(L, L)
        assert cap == {2048: 128, 4200: 262, 8300: 518, 1000: 64, 1500: 93}[L]
        for d in (cap - 1, cap, cap + 1):
            add("cap_length", "L%d_subs%d" % (L, d), base[L], subs(base[L], d), d)
    # 2. ... decided by svx_ctx_set_edit_wavefront_cap (48, 100), or by a threshold of 48 / 100
    for L, ds in ((1000, (47, 48, 49)), (4200, (47, 48, 49)), (4200, (99, 100, 101))):
        for d in ds:
            add("cap_wfa", "L%d_subs%d" % (L, d), base[L], subs(base[L], d), d)
    # 3. the lengths alone differ by cap and cap + 1 (k_edit_wfa's early exit); the shorter side moves the cap itself:
    #    (4200 + 4200 - 254) / 32 = 254, so blocks of 254 / 255 sit on it and 262 / 263 (the cap of two full lengths) above
    for L, blocks in ((1000, (63, 64, 65)), (4200, (254, 255, 262, 263))):
        for n in blocks:
            add("cap_lendiff", "L%d_cut%d" % (L, n), base[L], cut(base[L], L // 2, n), n)
    add("cap_lendiff", "L1000_dels30_subs34", base[1000], mixed(base[1000], 30, 34), 64)
    # 4. more than 64, 128 and 192 diagonals (d >= 32, 64, 96), from deletions and substitutions in equal parts
    for d in (31, 32, 33, 63, 64, 65, 95, 96, 97):
        add("batches", "L2048_dels%d_subs%d" % (d // 2, d - d // 2), base[2048], mixed(base[2048], d // 2, d - d // 2), d)
    # 5. a sequence shorter than the edit count: diagonals clipped at -m or +n
    for la, lb in ((1, 1), (1, 2), (1, 64), (1, 65), (1, 66), (2, 40), (40, 2), (3, 60), (5, 5)):
        a = dna(rng, la)
        b = dna(rng, lb)
        if (la, lb) == (1, 1):
            b = nxt(a)
        add("clipped", "unrelated_%d_%d" % (la, lb), a, b)
    add("clipped", "equal_1_1", b"G", b"G", 0)
    add("clipped", "A_against_64A", b"A", b"A" * 64, 63)
    # 6. match runs of exactly r bytes: the byte in front differs (x / x2), the byte behind differs (y / y2) or the run
    #    ends at both sequences' ends ("end"); "head": the run is the common prefix
    runs = []
    for r in RUNS:
        x, y, run = dna(rng, 5), dna(rng, 6), dna(rng, r)
        x2, y2 = x[:-1] + nxt(x[-1:]), nxt(y[:1]) + y[1:]
        add("runs", "r%d_end" % r, x + run, x2 + run, 1)
        add("runs", "r%d_mid" % r, x + run + y, x2 + run + y2, 2)
        add("runs", "r%d_head" % r, run + y, run + y2, 1)
        runs.append(run)
    sep = dna(rng, len(RUNS) - 1)
    chain_a = b"".join(run + sep[i:i + 1] for i, run in enumerate(runs))
    chain_b = b"".join(run + nxt(sep[i:i + 1]) for i, run in enumerate(runs))
    add("runs", "chain", chain_a, chain_b, len(RUNS) - 1)
    # 7. patterns of exactly 16 / 17 (fast / rich instantiation) and 255 / 256 symbols on one and two strips: the copy
    #    carries ~2 % substitutions — every fourth to a byte the pattern lacks — and one 7-byte deletion, so `a` is the pattern
    for sigma in (16, 17, 255, 256):
        for L in (300, 4200):
            a, alphabet = _with_alphabet(rng, sigma, L)
            foreign = np.setdiff1d(np.arange(256, dtype=np.uint8), alphabet)
            b = np.frombuffer(a, np.uint8).copy()
            for j, at in enumerate(spread(L, L // 50)):
                b[at] = foreign[j % len(foreign)] if (j % 4 == 0 and len(foreign)) else _NEXT[b[at]]
            add("alphabets", "sigma%d_L%d" % (sigma, L), a, cut(b.tobytes(), L // 3, 7))
    #    a 16-symbol `a` against a 17-symbol `b` (and 255 against 256): at equal lengths `a` is the pattern, one byte more
    #    on `b` and `b` is — two kernels, one answer
    for lo, L in ((16, 300), (16, 4200), (255, 600)):
        full = rng.permutation(256)[:lo + 1].astype(np.uint8)
        a, _ = _with_alphabet(rng, lo, L, full[:lo])
        b = np.frombuffer(a, np.uint8).copy()
        # the extra symbol goes where `a` repeats a byte, so that `b` keeps all of a's symbols
        seen, spare = set(), []
        for at, c in enumerate(a):
            if c in seen:
                spare.append(at)
            seen.add(c)
        b[spare[::max(1, len(spare) // 5)][:5]] = full[lo]
        b = b.tobytes()
        assert len(set(a)) == lo and len(set(b)) == lo + 1
        add("alphabets", "sigma%d_against_%d_L%d_same_length" % (lo, lo + 1, L), a, b, 5)
        add("alphabets", "sigma%d_against_%d_L%d_b_longer" % (lo, lo + 1, L), a, b + bytes(full[lo:lo + 1]), 6)
    #    the text holds a byte the rich pattern lacks wherever the pattern holds its lowest byte (its symbol 0): the
    #    marker for "absent" must not be taken for a symbol
    for sigma in (17, 255):
        alphabet = np.sort(rng.permutation(256)[:sigma]).astype(np.uint8)
        foreign = np.setdiff1d(np.arange(256, dtype=np.uint8), alphabet)[-1]
        a = np.full(600, alphabet[0], np.uint8)     # every third byte is the lowest one, the others hold the rest
        rest, _ = _with_alphabet(rng, sigma - 1, 400, alphabet[1:])
        a[np.arange(600) % 3 != 0] = np.frombuffer(rest, np.uint8)
        b = np.where(a == alphabet[0], foreign, a).astype(np.uint8)
        add("alphabets", "sigma%d_foreign_where_symbol0" % sigma, a.tobytes(), b.tobytes(), int((a == alphabet[0]).sum()))
    #    rich pairs for the band rounds: both instantiations in every round
    rich, _ = _with_alphabet(rng, 256, 4200)
    add("alphabets", "sigma256_L4200_subs300", rich, subs(rich, 300), 300)
    add("alphabets", "sigma256_L4200_subs1100", rich, subs(rich, 1100), 1100)
    # 8. the exact request's band rounds on two and three strips: 256 | 257 (first band), 1024 | 1025 (second), a length
    #    difference above the first and above the second band, a bad start, unrelated sequences
    for L in (4200, 8300):
        for d in (256, 257, 1024, 1025):
            add("bands", "L%d_subs%d" % (L, d), base[L], subs(base[L], d), d)
        for n in (300, 1100):
            add("bands", "L%d_cut%d" % (L, n), base[L], cut(base[L], L // 2, n), n)
        add("bands", "L%d_unrelated_start" % L, dna(rng, 1500) + base[L][1500:], base[L])
    add("bands", "unrelated_4200_4100", dna(rng, 4200), dna(rng, 4100))
    # 9. pattern lengths around one and two strips, text lengths around the boundary stream's 32-column words
    for m in (4096, 4097, 8192, 8193):
        a = dna(rng, m)
        for d in (0, 1, 31, 32, 33):
            add("strips", "m%d_n%d" % (m, m - d), a, subs(cut(a, m // 2, d), 4), d + 4)   # (no substitution at the cut)
    assert set(family.values()) == set(FAMILIES)
    return cases, family, intended


CASES, FAMILY, INTENDED = _build()
NAMES = sorted(CASES)


@functools.lru_cache(maxsize=None)
def reference():
    """name -> the oracle's full-matrix distance, computed once per process."""
    from oracle import orc
    return {name: orc.edit_distance(*CASES[name]) for name in NAMES}


def thresholds(ref):
    """The thresholds the whole table is asked with: FIXED_KS and every distinct reference distance, one below, one above."""
    return sorted(set(FIXED_KS) | {k for d in set(ref.values()) for k in (d - 1, d, d + 1) if k >= 0})


def _tail(own, partner):
    """What follows `own` in an adversarial pool: the partner's next bytes on the main diagonal — they would continue a
    match that runs into own's end — and, where the partner has none, its last bytes (equal ends: both tails match)."""
    t = partner[len(own):len(own) + TAIL]
    t += (partner[-TAIL:] if partner else b"")[:TAIL - len(t)]
    return t + b"ACGTTGCAACGTTGCA"[:TAIL - len(t)]


def layout(cases, residues=None, adversarial=True):
    """(pool u8, a_off, a_len, b_off, b_len) for `cases`: a dict name -> (a, b) (in its own order) or a list of (a, b).

    residues: None — pair i starts its a at an address = i mod 8 and its b at (i div 8) mod 8 (mod 8), so every 64 pairs
    walk all 64 combinations; a list of (ra, rb) per pair; or "packed" — no padding at all, every sequence starts
    where the one before ends (no tails either).  adversarial: the TAIL bytes behind each sequence continue its match
    with the partner (see _tail) and the padding is bases; otherwise tails and padding are zero bytes.  The pool ends
    with TAIL filler bytes."""
    pairs = list(cases.values()) if isinstance(cases, dict) else list(cases)
    out, at = [], 0
    a_off, a_len, b_off, b_len = [], [], [], []

    def put(s):
        nonlocal at
        out.append(s)
        at += len(s)

    def pad_to(residue):
        n = (residue - at) % 8
        put((b"TGCATGCA" if adversarial else bytes(8))[:n])

    for i, (a, b) in enumerate(pairs):
        packed = isinstance(residues, str)
        if packed:
            assert residues == "packed"
        else:
            ra, rb = (i % 8, (i // 8) % 8) if residues is None else residues[i]
        for own, partner, offs, lens, res in ((a, b, a_off, a_len, None if packed else ra),
                                              (b, a, b_off, b_len, None if packed else rb)):
            if not packed:
                pad_to(res)
            offs.append(at)
            lens.append(len(own))
            put(own)
            if not packed:
                put(_tail(own, partner) if adversarial else bytes(TAIL))
    put(b"N" * TAIL if adversarial else bytes(TAIL))
    return np.frombuffer(b"".join(out), np.uint8), a_off, a_len, b_off, b_len


def runs_at_every_residue():
    """Family 6 once per combination of the two start addresses mod 8: (names, pairs, residues), 64 x the family."""
    fam = [n for n in NAMES if FAMILY[n] == "runs"]
    names, pairs, residues = [], [], []
    for ra in range(8):
        for rb in range(8):
            names += fam
            pairs += [CASES[n] for n in fam]
            residues += [(ra, rb)] * len(fam)
    return names, pairs, residues


# ---- haplotype recipes ------------------------------------------------------------------------------------------
IUPAC_AT, IUPAC_LEN = 256, 4096


def _hap_pool():
    rng = np.random.default_rng(SEED + 1)
    letters = np.frombuffer(b"ACGTNRYKMSWBDHVacgtnrykmswbdhv", np.uint8)
    return np.concatenate((np.arange(256, dtype=np.uint8), letters[rng.integers(0, len(letters), IUPAC_LEN)]))


HAP_POOL = _hap_pool()          # every byte value in order, then 4 KiB of mixed-case IUPAC


def _hap_build():
    U, RC = R.UPPER, R.REVCOMP
    absent = (0, 0, 0, 0)
    I = IUPAC_AT
    left, right = (I + 10, 90, 1, U), (I + 2000, 110, 1, U)
    cases = {}
    for f in (0, U, RC, U | RC):
        cases["all_bytes_flags%d" % f] = (absent, (0, 256, 1, f), absent)
    for n in (255, 256, 257):       # one pass of the kernel's 256 lanes, one lane less, one more
        for f in (0, U | RC):
            cases["len%d_flags%d" % (n, f)] = ((I + 300, n, 1, f), absent, absent)
    cases["three_pieces"] = ((I + 5, 100, 1, U), (I + 700, 50, 2, U | RC), (I + 1500, 77, 1, 0))
    for pos in range(3):            # len > 0, repeat = 0: the piece is absent
        pcs = [left, (I + 500, 60, 1, 0), right]
        pcs[pos] = pcs[pos][:2] + (0,) + pcs[pos][3:]
        cases["repeat0_piece%d" % pos] = tuple(pcs)
    cases["len0_repeat3"] = (left, (I + 500, 0, 3, U | RC), right)
    cases["revcomp_repeat3"] = (left, (I + 900, 41, 3, RC), right)
    cases["revcomp_upper_repeat3"] = (left, (I + 900, 41, 3, U | RC), right)
    cases["len1_repeat65535"] = (absent, (I + 7, 1, 65535, U), absent)
    cases["len700_repeat4"] = (left, (I + 1000, 700, 4, U), right)
    cases["all_absent"] = (absent, absent, absent)
    cases["all_repeat0"] = ((I, 10, 0, U), (I + 20, 30, 0, RC), (I + 50, 5, 0, 0))
    return cases


HAP_CASES = _hap_build()        # name -> three (off, len, repeat, flags) over HAP_POOL
HAP_LENGTH_FORMS = ("len1_repeat65535", "len700_repeat4")


def hap_expected(name):
    return R.assemble(HAP_POOL, HAP_CASES[name])
