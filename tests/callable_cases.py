"""Inputs of the svx_cover_single tests (tests/test_gpu_callable.py, tests/test_callable_host.py) with their answers by
the plain loops of tests/callable_restatement.py, computed once per case and shared.  A case is a list of lists of
(start_key, end_key), each sorted by start key.  The MIXED cases are random and have to be balanced: by the restatement
alone, between a tenth and nine tenths of their slots (entries) give a segment — a kernel that flags every slot or none
cannot pass them; the targeted cases pin one behaviour each and are all-or-nothing on purpose."""
import functools
import random

from svim_asm_amd import _lib
from tests import callable_restatement as R, cover_cases as C

CHUNK = _lib.COVER_SCAN_CHUNK  # slots per pass of the scan kernel: one workgroup of 256 lanes, four per lane
# wave (64), workgroup (256) and pass (CHUNK) edges, the carry across two and four passes, an empty, a one- and a two-entry list
MIXED_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 4 * CHUNK + 1)
CONTIG_LEN = C.CONTIG_LEN


@functools.lru_cache(maxsize=None)
def mixed():
    rng = random.Random(20261019)
    lists = [C.random_list(rng, n, reach=6.0 if n < 100 else 3.0) for n in MIXED_SIZES]
    lists[1] = [(R.key(1, 500), R.key(1, CONTIG_LEN - 500))]
    return lists


@functools.lru_cache(maxsize=None)
def empty_between():
    rng = random.Random(19)
    return [C.random_list(rng, 300, reach=3.0), [], C.random_list(rng, 700, reach=2.5)]


@functools.lru_cache(maxsize=None)
def disjoint():
    """Every slot gives a segment, over two passes: an element folded in twice would read as depth 2 somewhere."""
    rng = random.Random(3)
    out, at = [], 10
    for _ in range(CHUNK + 500):
        length = 1 + rng.randrange(90)
        out.append((R.key(at // CONTIG_LEN, at % CONTIG_LEN), R.key(at // CONTIG_LEN, min(CONTIG_LEN, at % CONTIG_LEN + length))))
        at += length + 1 + rng.randrange(40)
    return [out, out[:64], out[:65]]


@functools.lru_cache(maxsize=None)
def duplicated():
    """Every entry twice: no segment at all, seg_off stays flat."""
    twice = lambda ivs: sorted(ivs + ivs)
    return [twice(disjoint()[0][:CHUNK + 77]), twice(C.random_list(random.Random(5), 150)), twice(disjoint()[0][:32])]


@functools.lru_cache(maxsize=None)
def abutting():
    """Alignments that end where the next begins: a segment each, never joined."""
    return [[(R.key(0, 100 * k), R.key(0, 100 * (k + 1))) for k in range(300)],
            [(R.key(0, 0), R.key(0, 50)), (R.key(0, 50), R.key(0, 51)), (R.key(0, 51), R.key(0, 700))]]


@functools.lru_cache(maxsize=None)
def equal_starts():
    """Groups with one start and different ends, the longest first, last or in the middle: single between the two longest."""
    rng = random.Random(23)
    out = []
    for k in range(200):
        ends = rng.sample(range(20, 150), 1 + k % 4)
        out += [(R.key(k % 2, 1000 * (k // 2)), R.key(k % 2, 1000 * (k // 2) + e)) for e in ends]
    out.sort(key=lambda t: t[0])  # (stable: the ends of a group stay in their drawn order)
    return [out]


@functools.lru_cache(maxsize=None)
def nested():
    """A short entry inside a long one: a segment in front of it and one behind it."""
    rng = random.Random(7)
    short = sorted((R.key(0, 2000 + 100 * k + rng.randrange(30)), R.key(0, 2000 + 100 * k + 60 + rng.randrange(30))) for k in range(300))
    return [[(R.key(0, 0), R.key(0, 100)), (R.key(0, 10), R.key(0, 20))], [(R.key(0, 1000), R.key(0, 40000))] + short]


def _short_run(n, first=100):
    """n short disjoint entries on contig 0 from `first` on."""
    rng = random.Random(29)
    out, at = [], first
    for _ in range(n):
        out.append((R.key(0, at), R.key(0, at + 5 + rng.randrange(20))))
        at += 30 + rng.randrange(10)
    return out


@functools.lru_cache(maxsize=None)
def carry_two_long():
    """Two long entries in pass 0 that end behind every later entry of a list of three passes: m1 and m2 both come from
    the carry in every later pass.  Single only in front of the second one and between the two ends (the open last slot)."""
    far_end = 10000000
    return [[(R.key(0, 0), R.key(0, far_end)), (R.key(0, 5), R.key(0, far_end + 1))] + _short_run(2 * CHUNK - 1)]


@functools.lru_cache(maxsize=None)
def carry_one_long():
    """One long entry: m1 from the carry, m2 from the current pass — single in every gap between the short ones."""
    return [[(R.key(0, 0), R.key(0, 10000000))] + _short_run(2 * CHUNK)]


@functools.lru_cache(maxsize=None)
def last_slot_only():
    """Depth 2 or more everywhere until every other entry has ended: the only segment lies in the open last slot."""
    out = sorted([(R.key(0, 100 * k), R.key(0, 100 * k + 150)) for k in range(351)] * 2)
    return [out + [(R.key(0, 35050), R.key(0, 36000))], [(R.key(2, 7), R.key(2, 9))] * 2 + [(R.key(2, 8), R.key(2, 10))]]


@functools.lru_cache(maxsize=None)
def contig_border():
    """Entries that end and start at a contig border: an end key on contig 0 lies below every key of contig 1."""
    return [[(R.key(0, 90000), R.key(0, CONTIG_LEN)), (R.key(1, 0), R.key(1, 5000)), (R.key(1, 4000), R.key(1, CONTIG_LEN)),
             (R.key(2, 0), R.key(2, 10))],
            [(R.key(0, 10), R.key(0, CONTIG_LEN)), (R.key(0, 99999), R.key(0, CONTIG_LEN)), (R.key(1, 0), R.key(1, 1))]]


@functools.lru_cache(maxsize=None)
def far():
    """Contig 2^16 and position 2^31 - 1."""
    rng = random.Random(17)
    top, c = (1 << 31) - 1, 1 << 16
    ivs = sorted([(R.key(c, top - 5000), R.key(c, top)), (R.key(c, 0), R.key(c, 1 << 30)), (R.key(c - 1, top - 10), R.key(c - 1, top)),
                  (R.key(0, top - 1), R.key(0, top)), (R.key(c, top - 1), R.key(c, top))] +
                 [(R.key(c, s), R.key(c, s + 4000)) for s in (rng.randrange(1 << 30, top - 4000) for _ in range(200))])
    return [ivs]


# batches of more lists than one pass of the offsets kernel takes: one pass exactly, one list into the second, one into the third
MANY_LISTS = (CHUNK, CHUNK + 1, 2 * CHUNK + 1)


@functools.lru_cache(maxsize=None)
def many_lists(n):
    """n lists, list l of l % 4 short disjoint entries (a segment each): counts of 0 to 3 on both sides of every pass
    border of the exclusive sum over the lists.  Kept out of CASES: the tests that walk CASES need no batch of this size."""
    return [_short_run(l % 4, first=100 + 7 * l) for l in range(n)]


@functools.lru_cache(maxsize=None)
def many_lists_answers(n):
    return R.flat(R.single(many_lists(n)))


MIXED = {"mixed": mixed, "empty_between": empty_between}
TARGETED = {"disjoint": disjoint, "duplicated": duplicated, "abutting": abutting, "equal_starts": equal_starts, "nested": nested,
            "carry_two_long": carry_two_long, "carry_one_long": carry_one_long, "last_slot_only": last_slot_only,
            "contig_border": contig_border, "far": far}
CASES = dict(MIXED, **TARGETED)


@functools.lru_cache(maxsize=None)
def answers(name):
    """(seg_lo, seg_hi, seg_off) of the case, as lists."""
    return R.flat(R.single(CASES[name]()))


def is_balanced(name):
    segments = len(answers(name)[0])
    slots = sum(len(ivs) for ivs in CASES[name]())
    return slots > 0 and slots <= 10 * segments <= 9 * slots


def check_inputs(lists):
    """What svx_cover_single requires of a valid batch."""
    for ivs in lists:
        assert all(a[0] <= b[0] for a, b in zip(ivs, ivs[1:]))
        assert all(s >> 32 == e >> 32 and s < e for s, e in ivs)
