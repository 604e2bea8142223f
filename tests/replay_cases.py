"""A case table for svx_variant_replay (svim_asm_amd/csrc/svx_replay.hip): jobs, edits and pairs against the edges of a
tile of output bytes (TILE, one workgroup of k_replay_emit and k_replay_compare), a lane's 16 bytes, a chunk of edits
(CHUNK, one workgroup of the edit scan) and a workgroup of jobs or pairs (GROUP).  tests/test_replay_cases.py holds the
table to its own preconditions where there is no GPU; tests/test_gpu_replay.py runs it on the device.

A case is a `Call`: jobs (window, edits), pairs, and the pool they are laid out in.  Every range of the pool lies at a
chosen residue modulo 16 between LIVE canaries — '!' in front, '?' behind, bytes that no window or allele holds — so a
byte fetched from outside a range and not masked shows in a string.  Expected results come from
tests/replay_restatement.py alone.  `facts` computes, from a call and the constants, where every job and every edit
begins in the output; `SHOWS` names what each case has to show and `check_preconditions` holds every case to it."""
import functools
import random

import numpy as np

from tests import replay_restatement as RR

# The constants of the kernels, as literals (the one place the table can be moved from): TILE = SVX_REPLAY_TILE, LANE the
# bytes of one lane, CHUNK = kScanChunk, GROUP = kScanThreads.
K = dict(TILE=4096, LANE=16, CHUNK=1024, GROUP=256)
T, C, G = K["TILE"], K["CHUNK"], K["GROUP"]
EDIT_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1)
OUT_LENGTHS = (0, 1, T - 1, T, T + 1, 2 * T + 1)
JOB_COUNTS = (1, 2, G - 1, G, G + 1, 4 * G + 1, 4097)


def dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


class Call(object):
    def __init__(self, seed=0, pool_at_zero=False):
        self.rng = random.Random(seed)
        self.pool = bytearray()
        self.pool_at_zero = pool_at_zero
        self.win_off, self.win_len, self.ed_first = [], [], [0]
        self.ed = []  # (start, ref_len, alt_off, alt_len)
        self.pair_a, self.pair_b = [], []

    def place(self, data, res=None):
        """`data` into the pool at residue `res` modulo 16 (random without one), canaries around it; its offset."""
        if self.pool_at_zero and not self.pool:
            self.pool.extend(data)
            self.pool.extend(b"?")
            return 0
        res = self.rng.randrange(16) if res is None else res
        pad = (res - len(self.pool)) % 16 or 16
        self.pool.extend(b"!" * pad)
        at = len(self.pool)
        self.pool.extend(data)
        self.pool.extend(b"?")
        return at

    def job(self, win, edits=(), win_res=None, alt_res=None):
        """A job; `edits`: (start, ref_len, alt bytes).  Returns its index."""
        self.win_off.append(self.place(win, win_res))
        self.win_len.append(len(win))
        for start, ref_len, alt in edits:
            self.ed.append((start, ref_len, self.place(alt, alt_res), len(alt)))
        self.ed_first.append(len(self.ed))
        return len(self.win_off) - 1

    def job_like(self, j):
        """A second job on job j's window and alleles: the same ranges of the pool."""
        self.win_off.append(self.win_off[j])
        self.win_len.append(self.win_len[j])
        self.ed.extend(self.ed[self.ed_first[j]:self.ed_first[j + 1]])
        self.ed_first.append(len(self.ed))
        return len(self.win_off) - 1

    def pair(self, a, b):
        self.pair_a.append(a)
        self.pair_b.append(b)

    def args(self):
        ed = list(zip(*self.ed)) if self.ed else [[]] * 4
        return (np.frombuffer(bytes(self.pool), np.uint8), np.array(self.win_off, np.uint64), np.array(self.win_len, np.uint32),
                np.array(self.ed_first, np.uint32), np.array(ed[0], np.uint32), np.array(ed[1], np.uint32), np.array(ed[2], np.uint64),
                np.array(ed[3], np.uint32), np.array(self.pair_a, np.uint32), np.array(self.pair_b, np.uint32))


def good_edits(rng, n, gap=2, alt_most=3):
    """(window, n edits in order and inside): edit i starts at gap * i + 1 and replaces 0 .. gap - 1 bytes by 0 .. alt_most."""
    win = dna(rng, gap * n + 5)
    edits = []
    for i in range(n):
        ref_len = rng.randrange(0, gap)
        alt = dna(rng, rng.randrange(0 if ref_len else 1, alt_most + 1))
        edits.append((gap * i + 1, ref_len, alt))
    return win, edits


def job_of_length(rng, n, with_edits):
    """(window, edits) whose string has exactly n bytes: no edit, or a deletion of 2, an insertion of 3 and an SNV."""
    if not with_edits or n < 4:
        return dna(rng, n), []
    win = dna(rng, n - 1)  # - 2 + 3
    third = max(1, len(win) // 3)
    return win, [(0, 2, b""), (third + 2, 0, dna(rng, 3)), (len(win) - 1, 1, b"G")]


# ------------------------------------------------------------------------------------------------------------ the cases
def case_edit_counts():
    c = Call(1)
    for n in EDIT_COUNTS:
        c.job(*good_edits(c.rng, n))
    for j in range(len(EDIT_COUNTS)):
        c.pair(j, j)
    return c


def case_out_length(n, with_edits):
    c = Call(2 + n)
    c.job(*job_of_length(c.rng, n, with_edits))
    c.pair(0, 0)
    return c


def case_out_lengths_in_a_row():
    c = Call(3)
    for n in OUT_LENGTHS + OUT_LENGTHS[::-1]:
        c.job(*job_of_length(c.rng, n, n % 2 == 1))
    return c


def case_job_boundary(d):
    """Job 1 begins at output byte TILE + d, job 3 at 2 * TILE + d (an empty job 2 in front of it)."""
    c = Call(10 + d)
    c.job(*job_of_length(c.rng, T + d, True))
    c.job(*job_of_length(c.rng, T, False))
    c.job(b"ACGT", [(0, 4, b"")])
    c.job(*job_of_length(c.rng, 7 + 40, True))
    return c


def case_edit_boundary(d):
    """An insertion whose bytes begin at output byte TILE + d, one whose bytes end there, a deletion at that byte."""
    c = Call(20 + d)
    win = dna(c.rng, T + 60)
    c.job(win, [(T + d, 0, b"TTTTT")])
    c.job(win, [(T + d - 5, 0, b"GGGGG")])   # (job 1 begins at T + 65: its edit begins at 2T + 60 + d, in any case off the edge)
    c2 = len(c.win_off)
    # job c2 begins at 2 * (T + 65): a window whose front brings it to a tile edge, then the edit at TILE + d behind it
    front = (-2 * (T + 65)) % T
    win2 = dna(c.rng, front + T + 60)
    c.job(win2, [(front + T + d - 5, 0, b"GGGGG")])
    c.job(win2, [(front + T + d, 3, b"")])
    c.job(win2, [(3, 1, b"A"), (front + T + d, 1, b"CC"), (front + T + d + 1, 0, b"T")])
    assert c2 == 2
    return c


def case_insertions_at_both_ends():
    c = Call(30)
    win = dna(c.rng, 40)
    c.job(win, [(0, 0, b"TT")])
    c.job(win, [(40, 0, b"GGG")])
    c.job(win, [(0, 0, b"T"), (40, 0, b"G")])
    c.job(win, [(0, 0, b"T"), (0, 0, b"G")])          # two edits at one start
    c.job(b"", [(0, 0, b"ACGT")])
    c.pair(0, 1)
    return c


def case_whole_window_deleted():
    c = Call(31)
    win = dna(c.rng, 33)
    a = c.job(win, [(0, 33, b"")])
    b = c.job(dna(c.rng, 5), [(0, 2, b""), (2, 3, b"")])
    e = c.job(b"")
    c.job(win, [(0, 33, b"ACG")])
    c.job(win, [(0, 34, b"")])                          # not inside
    for x, y in ((a, b), (a, e), (e, e), (a, a), (a, 3), (4, 4)):
        c.pair(x, y)
    return c


def case_alt_lengths():
    c = Call(32)
    win = dna(c.rng, 50)
    for n in (0, 1, T + 1):
        c.job(win, [(10, 3, dna(c.rng, n))])
        c.job(win, [(10, 3, dna(c.rng, n)), (13, 0, dna(c.rng, n)), (20, 1, dna(c.rng, n))])
    return c


def case_empty_windows():
    c = Call(33)
    c.job(b"")
    c.job(b"", [(0, 0, b"A")])
    c.job(b"", [(0, 1, b"A")])                          # not inside
    c.job(b"", [(1, 0, b"A")])                          # not inside: begins behind the window
    c.job(b"")
    for a in range(5):
        for b in range(5):
            c.pair(a, b)
    return c


def case_residues():
    """All 256 pairs of residues of win_off and ed_alt_off modulo 16; the first window at offset 0 of the pool."""
    c = Call(34, pool_at_zero=True)
    for i in range(16):
        for k in range(16):
            n = 20 + (i * 16 + k) % 23
            win = dna(c.rng, n)
            c.job(win, [(3, 2, dna(c.rng, 1 + (i + k) % 19)), (n - 4, 1, dna(c.rng, 17 + k))], win_res=i, alt_res=k)
    return c


def with_status(rng, n, where, status):
    """n good edits with edit `where` spoilt: out of order (1: it begins inside the edit in front, or at its start) or not
    inside (2)."""
    win, edits = good_edits(rng, n, gap=4)
    start, ref_len, alt = edits[where]
    if status == 1:
        prev = edits[where - 1]
        edits[where - 1] = (prev[0], 3, prev[2])
        edits[where] = (prev[0] + rng.choice((0, 2)), ref_len, alt)
    else:
        edits[where] = (start, len(win) - start + 1, alt)
    return win, edits


def case_status():
    """Every status at a job's first (2 only: a first edit is always in order), second, middle and last edit, each between
    two good jobs; both at once (1 wins)."""
    c = Call(35)
    for status in (1, 2):
        for where in (0, 1, 5, 10):
            if status == 1 and where == 0:
                continue
            c.job(*good_edits(c.rng, 11, gap=4))
            c.job(*with_status(c.rng, 11, where, status))
    c.job(*good_edits(c.rng, 11, gap=4))
    win, edits = with_status(c.rng, 11, 5, 1)
    edits[9] = (edits[9][0], len(win), edits[9][2])
    c.job(win, edits)
    c.job(dna(c.rng, 9), [(4, 2, b"A"), (6, 0, b"C")])  # begins where the one in front ends: in order
    c.job(dna(c.rng, 9), [(4, 2, b"A"), (5, 0, b"C")])  # one byte earlier
    c.job(dna(c.rng, 9), [(4, 2, b"A"), (4, 0, b"C")])  # equal starts
    c.job(dna(c.rng, 9), [(4, 0, b"A"), (4, 2, b"C")])  # equal starts behind an insertion
    c.job(dna(c.rng, 9), [(6, 1, b"A"), (2, 1, b"C")])  # descending
    c.job(*good_edits(c.rng, 3))
    n = len(c.win_off)
    for j in range(n - 1):
        c.pair(j, j + 1)
        c.pair(j, j)
    return c


def case_pairs():
    c = Call(36)
    base = dna(c.rng, 2 * T + 50)

    def changed(at):
        b = bytearray(base)
        b[at] = ord("A") if b[at] != ord("A") else ord("C")
        return bytes(b)
    j0 = c.job(base)
    same = c.job(base[:100], [(100, 0, base[100:])])                           # the same string by another route
    variants = [c.job(changed(at)) for at in (0, len(base) - 1, T - 1, T, 2 * T - 1, 2 * T, 15, 16)]
    shorter = c.job(base[:-1])
    longer = c.job(base, [(7, 0, b"A")])
    bad = c.job(base, [(5, 2, b"A"), (6, 1, b"C")])
    bad2 = c.job_like(bad)
    e1, e2 = c.job(b""), c.job(b"AC", [(0, 2, b"")])
    c.pair(j0, same)
    for v in variants:
        c.pair(j0, v)
        c.pair(v, same)
    for x, y in ((j0, shorter), (j0, longer), (shorter, longer), (j0, bad), (bad, j0), (bad, bad2), (bad, bad), (j0, j0), (e1, e2), (e2, e2),
                 (e1, j0)):
        c.pair(x, y)
    for k in range(1000):                                                       # the same job in 1000 pairs
        c.pair(same, (j0, variants[k % len(variants)])[k % 2])
    return c


def case_job_count(n):
    c = Call(40 + n)
    wins = [dna(c.rng, 9 + k) for k in range(7)]
    placed = {}
    for j in range(n):
        k = j % 7
        if k not in placed or j % 5 == 0:
            placed[k] = c.job(wins[k], [(1 + j % 6, j % 3, b"ACGTA"[:j % 4 + (j % 3 == 0)])])
        else:
            c.job_like(placed[k])
    for j in range(0, n - 1, 3):
        c.pair(j, j + 1)
    return c


def case_random(seed):
    rng = random.Random(seed)
    c = Call(seed)
    c.rng = rng
    for _ in range(rng.randrange(0, 7)):
        n = rng.choice((0, 1, 2, 3, 8, 30))
        win = bytes(rng.choice(b"AC") for _ in range(rng.choice((0, 1, 5, 17, 40, 300))))
        edits, at = [], 0
        for _ in range(n):
            at += rng.randrange(0, 4) if not edits or rng.random() < 0.1 else rng.randrange(1, 4)
            ref_len = rng.randrange(0, 3)
            edits.append((at, ref_len, bytes(rng.choice(b"AC") for _ in range(rng.randrange(0, 4)))))
            at += ref_len
        if edits and rng.random() < 0.15:
            k = rng.randrange(len(edits))
            edits[k] = (rng.randrange(0, len(win) + 3), rng.randrange(0, 5), edits[k][2])
        c.job(win, edits)
    n = len(c.win_off)
    if n:
        for _ in range(rng.randrange(0, 12)):
            c.pair(rng.randrange(n), rng.randrange(n))
    return c


CASES = {"edit-counts": case_edit_counts, "out-lengths-in-a-row": case_out_lengths_in_a_row,
         "insertions-at-both-ends": case_insertions_at_both_ends, "whole-window-deleted": case_whole_window_deleted,
         "alt-lengths": case_alt_lengths, "empty-windows": case_empty_windows, "residues": case_residues, "status": case_status,
         "pairs": case_pairs}
for _n in OUT_LENGTHS:
    for _w in (False, True):
        CASES["out-length-%d-%s" % (_n, "edited" if _w else "plain")] = functools.partial(case_out_length, _n, _w)
for _d in (-1, 0, 1):
    CASES["job-boundary%+d" % _d] = functools.partial(case_job_boundary, _d)
    CASES["edit-boundary%+d" % _d] = functools.partial(case_edit_boundary, _d)
for _n in JOB_COUNTS:
    CASES["jobs-%d" % _n] = functools.partial(case_job_count, _n)


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    return c.args()


@functools.lru_cache(maxsize=None)
def expected(name):
    return RR.replay_batch(*case(name))


# ------------------------------------------------------------------------------------------------------------ facts
def facts(args, exp):
    """From the arguments and the restatement's strings: per job its offset among the output bytes and its edits, per edit
    of a good job the output byte its alternative bytes begin at (the restatement's cursor, not the kernels' sums)."""
    bases, win_off, win_len, ed_first, ed_start, ed_ref_len, ed_alt_off, ed_alt_len, pair_a, pair_b = args
    F = {"job_off": exp["out_off"], "n_edits": [int(ed_first[j + 1]) - int(ed_first[j]) for j in range(len(win_off))], "alt_at": [],
         "alt_end": [], "total": exp["total"]}
    for j in range(len(win_off)):
        if exp["status"][j]:
            continue
        at, p = exp["out_off"][j], 0
        for e in range(int(ed_first[j]), int(ed_first[j + 1])):
            at += int(ed_start[e]) - p
            F["alt_at"].append(at)
            if int(ed_alt_len[e]):
                F["alt_end"].append(at + int(ed_alt_len[e]))
            at += int(ed_alt_len[e])
            p = int(ed_start[e]) + int(ed_ref_len[e])
    return F


def edge(values, k_tile, d):
    """Does any of `values` lie d bytes behind a positive multiple of the tile?"""
    return any(v - d > 0 and (v - d) % k_tile == 0 for v in values)


def check_preconditions(k=None, cases=None):
    """Every case shows what its name promises under the constants `k`; raises AssertionError("<case> does not show
    <what>") otherwise.  Returns the number of facts checked."""
    k = k or K
    t, ch, g = k["TILE"], k["CHUNK"], k["GROUP"]
    names = cases or list(CASES)
    n = 0

    def show(name, what, ok):
        nonlocal n
        assert ok, "%s does not show %s" % (name, what)
        n += 1
    for name in names:
        args, exp = case(name), expected(name)
        F = facts(args, exp)
        ed_first = [int(x) for x in args[3]]
        if name == "edit-counts":
            for want in (0, 1, 63, 64, 65, 255, 256, 257, ch - 1, ch, ch + 1, 2 * ch + 1):
                show(name, "a job of %d edits" % want, want in F["n_edits"])
            show(name, "good jobs only", not any(exp["status"]))
            show(name, "a job over three chunks of edits", any(b // ch - a // ch >= 2 for a, b in zip(ed_first, ed_first[1:]) if b > a))
        elif name.startswith("out-length-"):
            want = int(name.split("-")[2])
            show(name, "a total of %d bytes, an edge of the tile" % want, exp["total"] == want and want in (0, 1, t - 1, t, t + 1, 2 * t + 1))
            show(name, "edits or none", (len(args[4]) > 0) == (name.endswith("edited") and want >= 4))
        elif name == "out-lengths-in-a-row":
            for want in (0, 1, t - 1, t, t + 1, 2 * t + 1):
                show(name, "a string of %d bytes" % want, want in exp["out_len"])
        elif name.startswith("job-boundary"):
            d = int(name[len("job-boundary"):])
            show(name, "a job that begins %+d from a tile" % d, edge(F["job_off"][1:-1], t, d))
            show(name, "an empty job in front of such a job", exp["out_len"][2] == 0 and (F["job_off"][3] - d) % t == 0)
        elif name.startswith("edit-boundary"):
            d = int(name[len("edit-boundary"):])
            show(name, "alternative bytes that begin %+d from a tile" % d, edge(F["alt_at"], t, d))
            show(name, "alternative bytes that end %+d from a tile" % d, edge(F["alt_end"], t, d))
        elif name == "alt-lengths":
            for want in (0, 1, t + 1):
                show(name, "an allele of %d bytes" % want, want in [int(x) for x in args[7]])
        elif name == "residues":
            seen = set()
            for j in range(len(args[1])):
                for e in range(ed_first[j], ed_first[j + 1]):
                    seen.add((int(args[1][j]) % 16, int(args[6][e]) % 16))
            show(name, "all 256 residue pairs", len(seen) == 256)
            show(name, "a window at the pool's first byte", int(args[1][0]) == 0)
        elif name == "status":
            show(name, "every status", set(exp["status"]) == {0, 1, 2})
            show(name, "a bad job between two good ones", any(a == 0 and b and c == 0 for a, b, c in zip(exp["status"], exp["status"][1:], exp["status"][2:])))
            show(name, "the three edge rules", exp["status"][-6:-3] == [0, 1, 1])
        elif name == "pairs":
            show(name, "equal and unequal pairs", set(exp["equal"]) == {0, 1})
            show(name, "a string over two tiles", max(exp["out_len"]) > 2 * t)
            show(name, "one job in 1000 pairs", max(np.bincount(args[8])) >= 1000)
            s = exp["strings"]
            diffs = set()
            for a, b in zip(args[8][:20], args[9][:20]):
                if a == 0 and len(s[b]) == len(s[0]):
                    diffs.update(i for i in range(len(s[0])) if s[0][i] != s[b][i])
            for at, what in ((0, "the first byte"), (len(s[0]) - 1, "the last byte"), (t - 1, "the last byte of a tile"), (t, "the first byte of a tile"),
                             (2 * t - 1, "the last byte of the second tile"), (2 * t, "the first byte of the third tile"),
                             (k["LANE"] - 1, "the last byte of a lane"), (k["LANE"], "the first byte of the next lane")):
                show(name, "a pair that differs in %s alone" % what, at in diffs)
            show(name, "one difference per pair", len(diffs) == 8)
        elif name.startswith("jobs-"):
            want = int(name.split("-")[1])
            show(name, "its job count", len(args[1]) == want and want in (1, 2, g - 1, g, g + 1, 4 * g + 1, 4097))
            show(name, "one edit per job", F["n_edits"] == [1] * want)
        elif name == "whole-window-deleted":
            show(name, "a good job without bytes", exp["status"][0] == 0 and exp["out_len"][0] == 0 and exp["equal"][:4] == [1, 1, 1, 1])
        elif name == "insertions-at-both-ends":
            show(name, "insertions at 0 and at win_len", exp["status"][:3] == [0, 0, 0] and exp["out_len"][:3] == [42, 43, 42] and exp["status"][3] == 1)
        elif name == "empty-windows":
            show(name, "windows of length 0", exp["status"] == [0, 0, 2, 2, 0] and exp["out_len"] == [0, 1, 0, 0, 0])
        else:
            raise AssertionError("no precondition for " + name)
    return n
