"""Inputs of the svx_cover_query tests (tests/test_gpu_cover.py) with their answers by the plain loops of
tests/cover_restatement.py, computed once per case and shared.  A case is (lists, queries): lists of (start_key, end_key)
sorted by start key, queries of (lo_key, hi_key) in no order.  Every case has to answer both 0 and 1 for at least a tenth
of its (list, query) pairs — is_balanced, asserted on the restatement here and in tests/test_cover_host.py, so that a
kernel answering a constant cannot pass."""
import functools
import random

from svim_asm_amd import _lib
from tests import cover_restatement as R

CHUNK = _lib.COVER_SCAN_CHUNK  # entries per pass of the scan kernel: one workgroup of 256 lanes, four entries per lane
# wave (64), workgroup (256) and chunk-carry (CHUNK) edges of the scan, an empty and a one-entry list, several chunks
MIXED_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, CHUNK + 1, 4 * CHUNK + 1, CHUNK, 2 * CHUNK + 1)
QUERY_COUNTS = (0, 1, 63, 64, 65, 1000)
CONTIG_LEN = 100000


def random_list(rng, n, contigs=(0, 1, 2), contig_len=CONTIG_LEN, reach=3.0):
    """n intervals over `contigs`, sorted by start key; lengths up to `reach` times the mean spacing (nested and
    overlapping intervals in plenty), clipped to the contig."""
    span = len(contigs) * contig_len
    out = []
    for _ in range(n):
        c = rng.choice(contigs)
        start = rng.randrange(contig_len)
        length = 1 + rng.randrange(max(2, int(reach * span / max(n, 1))))
        out.append((R.key(c, start), R.key(c, min(contig_len, start + length))))
    out.sort(key=lambda t: t[0])
    return out


def random_queries(rng, n, contigs=(0, 1, 2), contig_len=CONTIG_LEN, longest=400):
    out = []
    for _ in range(n):
        c = rng.choice(contigs)
        lo = rng.randrange(contig_len)
        out.append((R.key(c, lo), R.key(c, min(contig_len, lo + rng.randrange(longest)))))
    return out


@functools.lru_cache(maxsize=None)
def mixed():
    rng = random.Random(20261019)
    lists = [random_list(rng, n, reach=6.0 if n < 100 else 2.0) for n in MIXED_SIZES]
    # the one-entry list: an alignment over most of a contig
    lists[1] = [(R.key(1, 500), R.key(1, CONTIG_LEN - 500))]
    return lists, random_queries(rng, max(QUERY_COUNTS))


@functools.lru_cache(maxsize=None)
def nested():
    """One long early alignment that contains 300 short later ones: the LAST interval with start <= lo does not cover
    the query, an earlier one does.  The second list holds the short ones alone."""
    rng = random.Random(7)
    short = sorted((R.key(0, 2000 + 100 * k + rng.randrange(30)), R.key(0, 2000 + 100 * k + 60 + rng.randrange(30))) for k in range(300))
    long_one = (R.key(0, 1000), R.key(0, 40000))
    queries = []
    for k in range(300):
        lo = 2000 + 100 * k + 40 + rng.randrange(20)
        queries.append((R.key(0, lo), R.key(0, lo + 80 + rng.randrange(100))))  # over the end of short k: inside the long one only
    for k in range(60):
        lo = 2000 + 100 * k + 31
        queries.append((R.key(0, lo), R.key(0, lo + 20)))                        # inside short k
    for k in range(120):
        lo = 39000 + 50 * k
        queries.append((R.key(0, lo), R.key(0, lo + 990)))                       # over the long one's end and beyond
    rng.shuffle(queries)
    return [[long_one] + short, short], queries


@functools.lru_cache(maxsize=None)
def boundaries():
    """lo equal to a start and hi equal to an end answer 1, one base beyond either answers 0."""
    rng = random.Random(11)
    ivs = sorted((R.key(c, 1000 * k + 100), R.key(c, 1000 * k + 600)) for c in (0, 1) for k in range(40))
    queries = []
    for start, end in ivs:
        queries += [(start, end), (start, start), (end, end), (start, end - 1), (start + 1, end),
                    (start - 1, end), (start, end + 1), (start - 1, start), (end, end + 1), (start - 1, end + 1)]
    rng.shuffle(queries)
    return [ivs], queries


@functools.lru_cache(maxsize=None)
def contig_border():
    """A long interval at the end of contig 0 and queries at the start of contig 1: its end key is above nothing there."""
    rng = random.Random(13)
    ivs = [(R.key(0, 10), R.key(0, 5000)), (R.key(0, 90000), R.key(0, CONTIG_LEN)), (R.key(1, 300), R.key(1, 9000)),
           (R.key(2, 0), R.key(2, 700))]
    queries = [(R.key(1, 0), R.key(1, 50)), (R.key(1, 0), R.key(1, 0)), (R.key(1, 299), R.key(1, 300)), (R.key(2, 0), R.key(2, 700)),
               (R.key(0, 95000), R.key(0, CONTIG_LEN)), (R.key(1, 300), R.key(1, 300)), (R.key(2, 0), R.key(2, 701)),
               (R.key(0, 99999), R.key(0, CONTIG_LEN)), (R.key(1, 1), R.key(1, 299)), (R.key(1, 8000), R.key(1, 9000))]
    for _ in range(40):
        c = rng.choice((0, 1, 2))
        lo = rng.randrange(12000)
        queries.append((R.key(c, lo), R.key(c, lo + rng.randrange(300))))
    return [ivs, ivs[:2], ivs[2:]], queries


@functools.lru_cache(maxsize=None)
def far():
    """Positions up to 2^31 - 1 and contig id 2^16."""
    rng = random.Random(17)
    top, c = (1 << 31) - 1, 1 << 16
    ivs = sorted([(R.key(c, top - 5000), R.key(c, top)), (R.key(c, 0), R.key(c, 1 << 30)), (R.key(c - 1, top - 10), R.key(c - 1, top)),
                  (R.key(0, top - 1), R.key(0, top))] +
                 [(R.key(c, s), R.key(c, s + 4000)) for s in (rng.randrange(1 << 30, top - 4000) for _ in range(200))])
    queries = [(R.key(c, top - 5000), R.key(c, top)), (R.key(c, top), R.key(c, top)), (R.key(c, top - 5001), R.key(c, top)),
               (R.key(c - 1, top), R.key(c - 1, top)), (R.key(0, top - 1), R.key(0, top)), (R.key(0, top - 2), R.key(0, top)),
               (R.key(c + 1, 0), R.key(c + 1, 5)), (R.key(c, 0), R.key(c, 1 << 30)), (R.key(c, 0), R.key(c, (1 << 30) + 1))]
    for start, end in [iv for iv in ivs if iv[1] - iv[0] >= 4000][:150]:
        queries += [(start + rng.randrange(2000), end - rng.randrange(2000))]
    for _ in range(60):
        lo = rng.randrange(1 << 30, top - 9000)
        queries.append((R.key(c, lo), R.key(c, lo + 4001 + rng.randrange(4000))))
    rng.shuffle(queries)
    return [ivs], queries


@functools.lru_cache(maxsize=None)
def empty_between():
    rng = random.Random(19)
    return [random_list(rng, 300), [], random_list(rng, 700, reach=1.5)], random_queries(rng, 200)


CASES = {"mixed": mixed, "nested": nested, "boundaries": boundaries, "contig_border": contig_border, "far": far,
         "empty_between": empty_between}


GRID_Y = 65535  # the most lists one launch of a search kernel takes side by side: list l + GRID_Y is the same thread's next trip


@functools.lru_cache(maxsize=None)
def many_lists():
    """GRID_Y + 2 lists of 0 to 2 entries and three queries: lists GRID_Y and GRID_Y + 1 are the second trip of the threads
    that answered lists 0 and 1, and the two of each pair are built to answer differently.  Kept out of CASES: the tests
    that walk CASES need no batch of this size."""
    rng = random.Random(65537)
    lists = [random_list(rng, rng.randrange(3), contigs=(0,), contig_len=10000, reach=0.4) for _ in range(GRID_Y + 2)]
    lists[0] = [(R.key(0, 0), R.key(0, 10000))]
    lists[1] = []
    lists[GRID_Y] = []
    lists[GRID_Y + 1] = [(R.key(0, 500), R.key(0, 2500)), (R.key(0, 4000), R.key(0, 9500))]
    return lists, [(R.key(0, 5000), R.key(0, 5200)), (R.key(0, 1000), R.key(0, 2000)), (R.key(0, 100), R.key(0, 9000))]


@functools.lru_cache(maxsize=None)
def many_lists_answers():
    return R.cover(*many_lists())


@functools.lru_cache(maxsize=None)
def answers(name):
    lists, queries = CASES[name]()
    return R.cover(lists, queries)


def is_balanced(rows):
    flat = [v for row in rows for v in row]
    ones = sum(flat)
    return len(flat) > 0 and 10 * ones >= len(flat) and 10 * (len(flat) - ones) >= len(flat)


def check_inputs(lists, queries):
    """What svx_cover_query requires of a valid batch."""
    for ivs in lists:
        assert all(a[0] <= b[0] for a, b in zip(ivs, ivs[1:]))
        assert all(s >> 32 == e >> 32 for s, e in ivs)
    assert all(lo <= hi and lo >> 32 == hi >> 32 for lo, hi in queries)
