"""The case table of the pair sort (tests/pair_cases.py) where there is no GPU: the C oracle and a numpy restatement of
form_partitions (reference SVIM_COMBINE.py:15-32: a stable sort by key, a new partition where type / contig differ or
the positions lie more than max_distance apart) agree on every case and on the combined batch, so that what
tests/test_gpu_pair_cases.py expects of the kernels rests on two independent computations; every case shows the classes
it lists and the numbers its name promises, every class is shown on each plan it applies to; the table's constants are
those of svx_pair.hip; a constant moved by one makes the preconditions fail, and so does a case that belies its name."""
import os
import re

import numpy as np
import pytest

from oracle import orc
from tests import pair_cases as P

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svim_asm_amd", "csrc", "svx_pair.hip")


def restated_partition(keys, max_dist):
    """form_partitions on packed keys (group << 32 | pos): -> (perm, part_id, n_parts)."""
    keys = np.asarray(keys, np.uint64)
    perm = np.argsort(keys, kind="stable")
    s = keys[perm]
    group, pos = (s >> np.uint64(32)).astype(np.int64), (s & np.uint64(0xFFFFFFFF)).astype(np.int64)
    brk = (group[1:] != group[:-1]) | (np.abs(pos[1:] - pos[:-1]) > max_dist)
    part = np.concatenate(([0], np.cumsum(brk))) if len(keys) else np.zeros(0, np.int64)
    return perm.astype(np.uint32), part.astype(np.uint32), (int(part[-1]) + 1 if len(keys) else 0)


def assert_two_answers(keys, max_dist, what):
    e_perm, e_part, e_n = orc.pair_partition(keys, max_dist)
    r_perm, r_part, r_n = restated_partition(keys, max_dist)
    assert e_n == r_n and np.array_equal(e_perm, r_perm) and np.array_equal(e_part, r_part), what


@pytest.mark.parametrize("family", P.FAMILIES)
def test_oracle_equals_the_restatement(family):
    cases = P.family(family)
    assert cases
    for c in cases:
        assert not c.keys.flags.writeable and c.keys.dtype == np.uint64 and c.max_dists, c.name
        for d in c.max_dists:
            assert_two_answers(c.keys, d, (c.name, d))


def test_combined_batch():
    keys, at = P.combined()
    assert 30_000 <= len(keys) <= 131072 and len(at) >= 20 and not keys.flags.writeable
    names = list(at)
    for i, name in enumerate(names):   # every case under a group field of its own, its keys otherwise unchanged
        part = keys[at[name]:at[name] + len(P.CASES[name].keys)]
        assert np.array_equal(part & np.uint64((1 << 40) - 1), P.CASES[name].keys) and (part >> np.uint64(40) == i).all(), name
    for d in (0, 1):
        assert_two_answers(keys, d, d)
        F = P.facts(keys, d, "single_launch", 256)
        for fam in P.COMBINED_FAMILIES:
            assert P.shown_by(F, families=(fam,)), (fam, d)
    # ... and not by one accident: both kinds of storage, a merged and a counted window, borders that open
    F = P.facts(keys, 0, "single_launch", 256)
    assert any(w.lds and w.sort == "count" and w.low_passes for w in F.filled) and any(not w.lds for w in F.filled)
    assert any(w.sort == "merge" for w in F.filled) and any(x.opens for x in F.borders)


def test_preconditions():
    shown = P.check_preconditions()
    assert len(P.CASES) >= 40 and {c.family for c in P.CASES.values()} == set(P.FAMILIES)
    assert {cid for cid, _ in shown} == set(P.CLASSES) - set(P.EXEMPT)
    assert {fam for fam, _, _ in P.CLASSES.values()} == set(P.FAMILIES)
    # the one case above 300 k keys is the sweep's two-chunk case, at the smallest n that has two chunks per workgroup
    assert [c.name for c in P.CASES.values() if len(c.keys) > 300_000] == [P.TWO_CHUNK_CASE]
    assert len(P.CASES[P.TWO_CHUNK_CASE].keys) == (256 // 2) * 8192 + 1


def test_a_case_that_belies_its_name_fails():
    """A 33rd run planted into the window of 32 runs: two neighbours of one run change places."""
    c = P.CASES["sort-run-counts"]
    w = P.case_facts(c.name, 0, "single_launch").windows[5]
    assert w.runs == 32 and w.sort == "merge"
    keys = c.keys.copy()
    bucket = (keys >> np.uint64(3)).astype(np.int64)
    at = np.nonzero((bucket >= w.lo) & (bucket < w.hi))[0]
    assert (np.diff(at) == 1).all()                              # the window's keys are consecutive in the input
    j = at[np.nonzero(keys[at][1:] > keys[at][:-1])[0][0]]
    keys[j], keys[j + 1] = keys[j + 1], keys[j]
    assert P.facts(keys, 0, "single_launch", 256).windows[5].runs == 33
    with pytest.raises(AssertionError, match="sort-run-counts"):
        P.check_preconditions(cases={c.name: c._replace(keys=keys)})
    P.check_preconditions(cases={c.name: c})


def test_constants_are_those_of_the_kernel_source():
    """A retune has to move the table in the same change, not move the thresholds off it."""
    text = open(SOURCE).read()

    def one(pattern):
        found = re.findall(pattern, text, re.M)
        assert len(found) == 1, (pattern, found)
        return found[0]
    K = P.K
    assert int(one(r"^constexpr int kMaxDigitBits = (\d+);")) == K["MAX_DIGIT_BITS"]
    assert int(one(r"^constexpr uint32_t kFineBits = (\d+);")) == K["FINE_BITS"]
    assert int(one(r"^constexpr uint32_t kWinCap = (\d+);")) == K["WIN_CAP"]
    assert int(one(r"^constexpr uint32_t kSingleGridMax = (\d+);")) == K["SINGLE_GRID_MAX"]
    assert int(one(r"^constexpr uint32_t kMergeRuns = (\d+);")) == K["MERGE_RUNS"]
    assert int(one(r"^constexpr uint32_t kSingleBlockMax = (\d+);")) == K["SINGLE_BLOCK_MAX"]
    assert int(one(r"^constexpr uint32_t kSmallSortMax = (\d+);")) == K["SMALL_SORT_MAX"] == P.SINGLE_LAUNCH_MAX
    assert int(one(r"^constexpr int kPartPer = (\d+);")) == K["PART_PER"]
    assert int(one(r"^constexpr uint32_t kPartChunk = (\d+)u \* kPartPer;")) == P.WG
    small, large = one(r"block_keys = small \? 256u \* (\d+) : 256u \* (\d+);")
    assert (256 * int(small), 256 * int(large)) == (K["BLOCK_SMALL"], K["BLOCK_LARGE"])
    assert int(one(r"for \(uint32_t c = 0; c < b\.n_blocks; c \+= (\d+)\)")) == K["ROWS"] == int(one(r"uint2 x\[(\d+)\];"))
    assert int(one(r"while \(runs\.size\(\) > (\d+)\)")) == K["FIELDS"] == int(one(r"uint32_t shift\[(\d+)\], off\[\d+\];"))
    cap, threads = one(r"k_key_or, dim3\(std::min<uint32_t>\(\(n \+ 255\) / 256, \(uint32_t\)ctx->n_cu \* (\d+)u\)\), dim3\((\d+)\)")
    assert (int(cap), int(threads)) == (K["KEY_OR_PER_CU"], P.KEY_OR_WG)
    assert int(one(r"ctx->n_cu / 2\), \(n \+ \d+\) / (\d+)\);")) == K["PART_GRAIN"]
    assert one(r"kSingleGridMax, std::max<uint32_t>\(1u, \(uint32_t\)ctx->n_cu / (\d+)\)\)") == "4"
    assert one(r"a\.target = std::max<uint32_t>\(\(n \+ grid_max - 1\) / grid_max, (\d+)u\);") == str(P.WG)


# SINGLE_GRID_MAX + 1 and PART_GRAIN - 1 are not felt at 256 CUs: min(65, 256 / 4) is still 64 workgroups, and a grain of
# 4095 gives 16385 keys the same five workgroups
MOVES = [(key, delta) for key in P.K for delta in (-1, 1) if (key, delta) not in (("SINGLE_GRID_MAX", 1), ("PART_GRAIN", -1))]


@pytest.mark.parametrize("key,delta", MOVES)
def test_a_threshold_moved_by_one_fails_the_preconditions(key, delta):
    assert {"WIN_CAP", "MERGE_RUNS", "FINE_BITS", "PART_PER", "SINGLE_BLOCK_MAX", "ROWS"} <= {k for k, _ in MOVES}
    k = dict(P.K)
    k[key] += delta
    with pytest.raises(AssertionError):
        P.check_preconditions(k)


def test_another_cu_count_fails_the_preconditions():
    """The table is laid out for 256 CUs: the device module says so instead of running cases that miss their classes."""
    with pytest.raises(AssertionError, match="n_cu 304"):
        P.check_preconditions(n_cu=304)
    with pytest.raises(AssertionError, match="n_cu 128"):
        P.check_preconditions(n_cu=128)
