"""A case table for the pair sort (svim_asm_amd/csrc/svx_pair.hip): the field plan of fields_of, the grid, the slices and
the window cut of the one-launch plan (pair_single_launch, k_pair_single), how a gathered window is sorted (merged runs,
counting passes, LDS or HBM), the borders between windows, the digit plan and the blocks of the radix passes, the spans
and chunks of the partition sweep (k_partition<0> and the wait-free pair of launches) and the stride loop of k_key_or.
tests/test_pair_cases.py holds the table to its own preconditions where there is no GPU, tests/test_gpu_pair_cases.py
runs it on the device.

Builder.  A case is built from a description, seeded by its name: `described` takes the windows it means to produce —
per window the population of every fine bucket, how the low bits are drawn, into how many sorted runs (or runs of which
lengths) the window's keys are dealt in input order — and the order of the windows in the input; `masked` draws keys
under a mask of live bits; `swept` lays positions along the sorted order with a jump at every chunk and span border of
the sweep.  A case carries the distances it runs with (`max_dists`): the distance at a named border is set by the
buckets and low bits next to it, whether a partition opens there by the distance the case runs with.

Facts.  facts(keys, max_dist, plan, n_cu, key_bits) computes from the inputs and the constants K alone (never from an
output): the bit fields, `live`; for the one-launch plan grid, target, slice length, the slices behind the input's end,
per window lo, hi, start, M, per, LDS or HBM, the runs of the gathered window, the sort taken, the passes and their
widths, and per border between filled windows whether a partition opens and how many empty windows lie between; for the
radix plans passes, digit width, blocks, the last block's keys, per pass whether a block holds one digit value only and
whether every value occurs; the sweep's grid, span, workgroups, chunks, where its flags lie; k_key_or's workgroups.

Classes.  CLASSES names every situation the table has to show and the plans it applies to (S: one launch, R: radix with
k_partition<0>, W: the wait-free plan); a case lists the classes it shows (`shows`, `id@max_dist` where the distance
matters) and the numbers its name promises (`expect`).  check_preconditions holds every case to both and every class to
at least one case on every plan it applies to.  The constants are literals HERE (K): a retune of svx_pair.hip has to
move the table with it, and a literal moved by one makes check_preconditions fail."""
import collections
import functools
import types
import zlib

import numpy as np

# The thresholds of svx_pair.hip, as literals (the one place the table can be moved from).  PART_PER: keys per thread
# and chunk of the sweep (chunk = 1024 * PART_PER = 8192); BLOCK_SMALL / BLOCK_LARGE: keys per radix block up to and
# beyond SMALL_SORT_MAX; ROWS: histogram rows in flight; FIELDS: fields_of's limit; KEY_OR_PER_CU: k_key_or's grid cap
# in workgroups per CU; PART_GRAIN: keys per workgroup below which the sweep's grid shrinks.
K = dict(MAX_DIGIT_BITS=9, FINE_BITS=9, WIN_CAP=5120, SINGLE_GRID_MAX=64, MERGE_RUNS=32, SINGLE_BLOCK_MAX=16384,
         SMALL_SORT_MAX=131072, PART_PER=8, BLOCK_SMALL=2048, BLOCK_LARGE=4096, ROWS=16, FIELDS=4, KEY_OR_PER_CU=4,
         PART_GRAIN=4096)
WG = 1024                       # threads of k_pair_single and k_partition: the least target, keys per `per`
KEY_OR_WG = 256                 # threads of k_key_or
SINGLE_LAUNCH_MAX = 131072      # what the GPU module sets with set_pair_single_launch_max for the one-launch plan
PLANS = ("single_launch", "radix", "wait_free")
PLAN_OF = dict(S="single_launch", R="radix", W="wait_free")
FAR = 0xFFFFFFFF
U = np.uint64

Case = collections.namedtuple("Case", "name family keys max_dists plans shows expect superset")


# -------------------------------------------------------------------------------------------------------- fields
def fields_of(bits, k=None):
    """fields_of of svx_pair.hip: -> (fields [(lo, hi)], live, number of bit runs, live forced to 1)."""
    k = k or K
    runs, i = [], 0
    while i < 64:
        if not (bits >> i) & 1:
            i += 1
            continue
        j = i
        while j < 64 and (bits >> j) & 1:
            j += 1
        runs.append([i, j])
        i = j
    raw = len(runs)
    while len(runs) > k["FIELDS"]:
        best = 0
        for r in range(1, len(runs) - 1):
            if runs[r + 1][0] - runs[r][1] < runs[best + 1][0] - runs[best][1]:
                best = r
        runs[best][1] = runs[best + 1][1]
        del runs[best + 1]
    live = sum(hi - lo for lo, hi in runs)
    if live == 0:
        return [(0, 1)], 1, raw, True
    return [tuple(r) for r in runs], live, raw, False


def dense_of(keys, fields):
    d, off = np.zeros(len(keys), U), 0
    for lo, hi in fields:
        w = hi - lo
        d |= ((keys >> U(lo)) & U((1 << w) - 1)) << U(off)
        off += w
    return d


def expand(dense, fields):
    """The original keys of dense keys (every set bit of a key lies inside the fields)."""
    k, off = np.zeros(len(dense), U), 0
    for lo, hi in fields:
        w = hi - lo
        k |= ((dense >> U(off)) & U((1 << w) - 1)) << U(lo)
        off += w
    return k


def _ceil(a, b):
    return -(-a // b)


def opens(a, b, max_dist):
    """The break rule between two neighbours of the sorted order (original keys, numpy arrays or ints)."""
    a, b = np.asarray(a, U), np.asarray(b, U)
    pa, pb = (a & U(FAR)).astype(np.int64), (b & U(FAR)).astype(np.int64)
    return ((a >> U(32)) != (b >> U(32))) | (np.abs(pa - pb) > max_dist)


# --------------------------------------------------------------------------------------------------------- facts
_LAST = []   # (keys, fields, dense, sorted keys) of the latest call: a case's plans and distances share one sort


def _dense_and_sorted(keys, fields):
    if not (_LAST and _LAST[0] is keys and not keys.flags.writeable and _LAST[1] == fields):
        dense = dense_of(keys, fields)
        _LAST[:] = [keys, fields, dense, keys[np.argsort(dense, kind="stable")]]
    return _LAST[2], _LAST[3]


def facts(keys, max_dist, plan, n_cu, key_bits=None, k=None):
    """Every quantity of the module docstring for `plan`, from the inputs and the constants `k` alone."""
    k = k or K
    keys = np.asarray(keys, U)
    n = len(keys)
    derived = int(np.bitwise_or.reduce(keys)) if n else 0
    bits = derived if key_bits is None else int(key_bits)
    assert derived & ~bits == 0
    fields, live, raw, forced = fields_of(bits, k)
    covered = 0
    for lo, hi in fields:
        covered |= ((1 << (hi - lo)) - 1) << lo
    F = types.SimpleNamespace(n=n, max_dist=max_dist, plan=plan, n_cu=n_cu, bits=bits, fields=fields, live=live, raw_runs=raw,
                              merged=raw > len(fields), forced=forced, dead_inside=bool(covered & ~bits) and not forced,
                              bit63=bool(bits >> 63), all_zero=derived == 0)
    dense, skeys = _dense_and_sorted(keys, fields)
    flags = np.zeros(n, bool)
    flags[1:] = opens(skeys[:-1], skeys[1:], max_dist)
    F.n_flags = int(flags.sum())
    same = (skeys[1:] >> U(32)) == (skeys[:-1] >> U(32))
    dist = np.abs((skeys[1:] & U(FAR)).astype(np.int64) - (skeys[:-1] & U(FAR)).astype(np.int64))
    F.group_change_at_equal_pos = bool((~same & (dist == 0)).any())
    F.bit31 = bool(((skeys[1:] ^ skeys[:-1]) & U(1 << 31))[same].any())   # neighbours of one group to both sides of 2^31
    F.dist_at = {d for d in (0, 1) if (same & (dist == max_dist + d)).any()}
    F.one_launch = plan == "single_launch" and n <= SINGLE_LAUNCH_MAX
    # ---- k_key_or (svx_pair_partition_dev)
    F.or_workgroups = min(_ceil(n, KEY_OR_WG), k["KEY_OR_PER_CU"] * n_cu)
    F.or_strided = n > F.or_workgroups * KEY_OR_WG
    F.or_bits_behind_first_stride = derived & ~int(np.bitwise_or.reduce(keys[:F.or_workgroups * KEY_OR_WG]))
    if F.one_launch:
        _one_launch(F, keys, dense, max_dist, n_cu, k)
    else:
        _radix(F, dense, flags, n_cu, k)
    return F


def _one_launch(F, keys, dense, max_dist, n_cu, k):
    n, live = F.n, F.live
    F.grid_max = min(k["SINGLE_GRID_MAX"], max(1, n_cu // 4))
    F.target = max(_ceil(n, F.grid_max), WG)
    F.grid = _ceil(n, F.target)
    F.slice_len = _ceil(_ceil(n, F.grid), 64) * 64
    F.slices_behind = sum(1 for g in range(F.grid) if g * F.slice_len >= n)
    F.fine_bits = min(live, k["FINE_BITS"])
    F.low_bits = live - F.fine_bits
    n_fine = 1 << k["FINE_BITS"]
    fine = (dense >> U(F.low_bits)).astype(np.int64)
    counts = np.bincount(fine, minlength=n_fine)
    cp = np.cumsum(counts)
    ex = cp - counts
    win_of = ex // F.target
    starts = ex[(counts > 0) & (ex > 0)]
    F.cut_offsets = {int(d) for d in ((starts + 1) % F.target - 1) if d in (-1, 0, 1)}   # bucket starts around a window border
    F.windows = []
    for g in range(F.grid):
        bs = np.nonzero(win_of == g)[0]
        w = types.SimpleNamespace(index=g, lo=0, hi=0, start=0, M=0, per=0, lds=True, runs=0, run_lens=[], sort="none", rounds=0,
                                  low_passes=0, low_width=0, bucket_pass=False, bucket_width=0, n_buckets=0, filled_buckets=0,
                                  empty_lo=0, empty_hi=0, ties_in_pair=False, ties_across_pairs=False, ranged=len(bs) > 0)
        F.windows.append(w)
        if not len(bs):
            continue
        w.lo, w.hi = int(bs[0]), int(bs[-1]) + 1
        w.start, w.M = int(ex[w.lo]), int(cp[w.hi - 1] - ex[w.lo])
        w.n_buckets = w.hi - w.lo
        if not w.M:
            continue
        c = counts[w.lo:w.hi]
        w.filled_buckets = int((c > 0).sum())
        w.empty_lo, w.empty_hi = int(np.argmax(c > 0)), int(np.argmax(c[::-1] > 0))
        w.per, w.lds = _ceil(w.M, WG), w.M <= k["WIN_CAP"]
        g_keys = dense[(fine >= w.lo) & (fine < w.hi)]            # the window as it is gathered: input order
        desc = np.nonzero(g_keys[1:] < g_keys[:-1])[0] + 1
        w.runs = len(desc) + 1
        w.run_lens = np.diff(np.concatenate(([0], desc, [w.M]))).tolist()
        srt = np.sort(g_keys, kind="stable")
        w.first, w.last = expand(srt[:2], F.fields), expand(srt[-2:], F.fields)
        if w.lds and w.runs <= k["MERGE_RUNS"]:
            w.rounds = (w.runs - 1).bit_length()
            w.sort = "merge" if w.rounds else "none"
            rid = np.repeat(np.arange(w.runs), w.run_lens)
            o = np.lexsort((rid, g_keys))
            eq = (g_keys[o][1:] == g_keys[o][:-1]) & (rid[o][1:] != rid[o][:-1])
            pair = rid[o][1:] // 2 == rid[o][:-1] // 2
            w.ties_in_pair, w.ties_across_pairs = bool((eq & pair).any()), bool((eq & ~pair).any())
        else:
            if F.low_bits:
                w.low_passes = _ceil(F.low_bits, k["FINE_BITS"])
                w.low_width = _ceil(F.low_bits, w.low_passes)
            w.bucket_pass = w.n_buckets > 1
            w.bucket_width = (w.n_buckets - 1).bit_length()
            w.sort = "count" if w.low_passes or w.bucket_pass else "none"
    F.filled = [w for w in F.windows if w.M]
    F.borders = []
    for a, b in zip(F.filled, F.filled[1:]):
        x = types.SimpleNamespace(left=a.index, right=b.index, empties_between=b.index - a.index - 1)
        x.opens = bool(opens(a.last[-1], b.first[0], max_dist))
        x.same_group = int(a.last[-1]) >> 32 == int(b.first[0]) >> 32
        x.dist = abs((int(a.last[-1]) & FAR) - (int(b.first[0]) & FAR))
        # nothing opens next to the border: the last two keys of the left window, the first two of the right one
        x.quiet = a.M > 1 and b.M > 1 and not opens(a.last[0], a.last[1], max_dist) and not opens(b.first[0], b.first[1], max_dist)
        F.borders.append(x)


def _radix(F, dense, flags, n_cu, k):
    n, live = F.n, F.live
    F.passes = _ceil(live, k["MAX_DIGIT_BITS"])
    F.digit_bits = _ceil(live, F.passes)
    F.small = n <= k["SMALL_SORT_MAX"]
    F.block_keys = k["BLOCK_SMALL"] if F.small else k["BLOCK_LARGE"]
    F.n_blocks = _ceil(n, F.block_keys)
    F.last_block = n - (F.n_blocks - 1) * F.block_keys
    F.empty_quarter = F.last_block <= 3 * (F.block_keys // 4)
    F.row_batches = _ceil(F.n_blocks, k["ROWS"])
    F.last_row_batch = F.n_blocks - (F.row_batches - 1) * k["ROWS"]

    @functools.lru_cache(maxsize=None)
    def per_pass():
        """Per pass (uniform_block, all_values): the keys of a pass arrive sorted by the digits below it."""
        out, cur = [], dense
        for p in range(F.passes):
            dig = ((cur >> U(p * F.digit_bits)) & U((1 << F.digit_bits) - 1)).astype(np.int64)
            full = dig[:n // F.block_keys * F.block_keys].reshape(-1, F.block_keys)
            uniform = bool(len(full) and (full == full[:, :1]).all(axis=1).any())
            out.append((uniform, len(np.unique(dig)) == 1 << F.digit_bits))
            cur = cur[np.argsort(dig, kind="stable")]
        return out
    F.per_pass = per_pass
    # ---- the sweep
    chunk = WG * k["PART_PER"]
    F.part_grid = 1 if n <= k["SINGLE_BLOCK_MAX"] else min(max(1, n_cu // 2), _ceil(n, k["PART_GRAIN"]))
    F.span = _ceil(_ceil(n, F.part_grid), WG) * WG
    F.workgroups = _ceil(n, F.span)
    F.chunks = [_ceil(min(F.span, n - g * F.span), chunk) for g in range(F.workgroups)]
    at = np.nonzero(flags)[0]
    inner = at[((at % F.span) % chunk == 0) & (at % F.span != 0)]
    outer = at[at % F.span == 0]
    F.flag_inner, F.flag_span = len(inner) > 0, len(outer) > 0
    j = np.arange(1, n)
    all_borders = j[(j % F.span) % chunk == 0]
    F.flags_exactly_at_borders = len(all_borders) > 0 and np.array_equal(at, all_borders)


# ------------------------------------------------------------------------------------------------------- classes
def _w(pred):
    return lambda F, k: any(w.M and pred(w, F, k) for w in F.windows)


def _b(pred):
    return lambda F, k: any(pred(x, F, k) for x in F.borders)


def _classes():
    """id -> (family, plans, predicate(facts, k))."""
    c = collections.OrderedDict()

    def add(cid, plans, pred):
        assert cid not in c
        c[cid] = (cid.split(".")[0], tuple(PLAN_OF[p] for p in plans), pred)

    # ---- grid
    add("grid.one_window", "S", lambda F, k: F.grid == 1 and F.n > WG // 2)
    add("grid.1024", "S", lambda F, k: F.n == WG and F.grid == 1)
    add("grid.1025", "S", lambda F, k: F.n == WG + 1 and F.grid == 2)
    add("grid.max_with_target_above_1024", "S", lambda F, k: F.grid == F.grid_max and F.target > WG)
    add("grid.slices_behind_the_end", "S", lambda F, k: F.slices_behind > 0)
    # ---- windows
    add("windows.empty_between_filled", "S", _b(lambda x, F, k: x.empties_between > 0))
    add("windows.empty_at_the_end", "S", lambda F, k: F.windows[-1].M == 0 and not F.windows[-1].ranged)
    add("windows.empty_at_the_end_with_buckets", "S", lambda F, k: F.windows[-1].M == 0 and F.windows[-1].ranged)
    add("windows.cut_on_a_bucket_border", "S", lambda F, k: F.grid > 1 and 0 in F.cut_offsets)
    add("windows.cut_one_key_before", "S", lambda F, k: F.grid > 1 and -1 in F.cut_offsets)
    add("windows.cut_one_key_behind", "S", lambda F, k: F.grid > 1 and 1 in F.cut_offsets)
    add("windows.empty_buckets_at_the_low_edge", "S", _w(lambda w, F, k: w.empty_lo > 0))
    add("windows.empty_buckets_at_the_high_edge", "S", _w(lambda w, F, k: w.empty_hi > 0))
    add("windows.1_bucket", "S", _w(lambda w, F, k: w.n_buckets == 1 and F.grid > 1))
    add("windows.2_buckets", "S", _w(lambda w, F, k: w.n_buckets == 2 and w.filled_buckets == 2))
    add("windows.all_buckets", "S", _w(lambda w, F, k: w.n_buckets == 1 << k["FINE_BITS"] and w.filled_buckets > 256))
    # ---- storage: LDS | HBM, and the steps of `per`
    counted = lambda w, k: w.runs > k["MERGE_RUNS"] and w.low_passes >= 1 and w.bucket_pass
    add("storage.win_cap", "S", _w(lambda w, F, k: w.M == k["WIN_CAP"] and w.lds and counted(w, k)))
    add("storage.win_cap+1", "S", _w(lambda w, F, k: w.M == k["WIN_CAP"] + 1 and not w.lds and counted(w, k)))
    for m in (1024, 4096):
        add("storage.per.%d" % m, "S", _w(lambda w, F, k, m=m: w.M == m and w.per == m // WG))
        add("storage.per.%d" % (m + 1), "S", _w(lambda w, F, k, m=m: w.M == m + 1 and w.per == m // WG + 1))
    # ---- sort
    for r in (1, 2, 3, 4, 5):
        add("sort.runs.%d" % r, "S", _w(lambda w, F, k, r=r: w.runs == r and w.lds and w.M > 2 * WG // 4
                                        and w.rounds == (r - 1).bit_length()))
    add("sort.runs.merge_runs", "S", _w(lambda w, F, k: w.runs == k["MERGE_RUNS"] and w.sort == "merge"))
    add("sort.runs.merge_runs+1", "S", _w(lambda w, F, k: w.runs == k["MERGE_RUNS"] + 1 and w.sort == "count" and w.lds))
    add("sort.a_run_of_one_key", "S", _w(lambda w, F, k: w.sort == "merge" and 1 in w.run_lens[1:-1] and w.run_lens[0] == 1))
    add("sort.uneven_runs", "S", _w(lambda w, F, k: w.sort == "merge" and max(w.run_lens) >= 100 * min(w.run_lens)))
    add("sort.ties_inside_a_pair_of_runs", "S", _w(lambda w, F, k: w.sort == "merge" and w.ties_in_pair))
    add("sort.ties_across_pairs_of_runs", "S", _w(lambda w, F, k: w.sort == "merge" and w.runs > 2 and w.ties_across_pairs))
    add("sort.merge_with_per_5", "S", _w(lambda w, F, k: w.sort == "merge" and w.per == 5 and w.runs >= 3))
    # ---- digits of the window passes
    many = lambda w, k: w.runs > k["MERGE_RUNS"]
    add("digits.bucket_only", "S", _w(lambda w, F, k: F.low_bits == 0 and F.live == k["FINE_BITS"] and w.filled_buckets > 1
                                      and many(w, k) and w.sort == "count" and w.low_passes == 0))
    add("digits.low_bits.1", "S", _w(lambda w, F, k: F.low_bits == 1 and many(w, k) and (w.low_passes, w.low_width) == (1, 1)))
    for p in (1, 2, 3):
        add("digits.low_bits.%d" % (9 * p), "S", _w(lambda w, F, k, p=p: F.low_bits == k["FINE_BITS"] * p and many(w, k)
                                                    and (w.low_passes, w.low_width) == (p, k["FINE_BITS"])))
        add("digits.low_bits.%d" % (9 * p + 1), "S", _w(lambda w, F, k, p=p: F.low_bits == k["FINE_BITS"] * p + 1 and many(w, k)
                                                        and w.low_passes == p + 1))
    add("digits.low_bits.55", "S", _w(lambda w, F, k: F.live == 64 and F.low_bits == 64 - k["FINE_BITS"] and many(w, k)
                                      and w.low_passes == _ceil(F.low_bits, k["FINE_BITS"])))
    add("digits.live_below_fine_bits", "S", _w(lambda w, F, k: F.live < k["FINE_BITS"] and F.low_bits == 0 and many(w, k)
                                               and w.bucket_pass))
    # ---- fields
    add("fields.one", "SRW", lambda F, k: len(F.fields) == 1 and not F.forced and F.raw_runs == 1)
    add("fields.limit", "SRW", lambda F, k: len(F.fields) == k["FIELDS"] == F.raw_runs)
    add("fields.merged_with_dead_bits", "SRW", lambda F, k: F.raw_runs > k["FIELDS"] and F.merged and F.dead_inside)
    add("fields.bit63", "SRW", lambda F, k: F.bit63 and F.n_flags > 0)
    add("fields.all_zero", "SRW", lambda F, k: F.all_zero and F.forced and F.live == 1 and F.n > WG)
    # ("fields.superset" is held by check_preconditions itself: it compares two sets of facts)
    add("fields.superset", "SRW", None)
    # ---- borders
    mixed = lambda F: 0 < F.n_flags < F.n - 1
    add("borders.continues.window_border", "S", _b(lambda x, F, k: not x.opens and x.empties_between == 0 and mixed(F)))
    add("borders.opens.window_border", "S", _b(lambda x, F, k: x.opens and x.quiet and x.empties_between == 0))
    add("borders.continues.one_empty_window", "S", _b(lambda x, F, k: not x.opens and x.empties_between == 1 and mixed(F)))
    add("borders.opens.one_empty_window", "S", _b(lambda x, F, k: x.opens and x.quiet and x.empties_between == 1))
    add("borders.continues.empty_windows", "S", _b(lambda x, F, k: not x.opens and x.empties_between > 1 and mixed(F)))
    add("borders.opens.empty_windows", "S", _b(lambda x, F, k: x.opens and x.quiet and x.empties_between > 1))
    add("borders.max_dist_at_a_window_border", "S", _b(lambda x, F, k: x.same_group and x.dist == F.max_dist))
    add("borders.max_dist+1_at_a_window_border", "S", _b(lambda x, F, k: x.same_group and x.dist == F.max_dist + 1))
    add("borders.max_dist_between_neighbours", "SRW", lambda F, k: 0 in F.dist_at)
    add("borders.max_dist+1_between_neighbours", "SRW", lambda F, k: 1 in F.dist_at)
    add("borders.group_change_at_equal_positions", "SRW", lambda F, k: F.group_change_at_equal_pos)
    add("borders.max_dist_0", "SRW", lambda F, k: F.max_dist == 0 and mixed(F))
    add("borders.max_dist_2^32-1", "SRW", lambda F, k: F.max_dist == FAR and mixed(F))
    add("borders.bit31", "SRW", lambda F, k: F.bit31 and mixed(F))
    # ---- radix
    for p in range(1, 9):
        add("radix.passes.%d" % p, "RW", lambda F, k, p=p: F.passes == p and F.n > WG)
    add("radix.blocks.1", "RW", lambda F, k: F.n_blocks == 1)
    add("radix.blocks.rows", "RW", lambda F, k: F.n_blocks == k["ROWS"] and F.last_block == F.block_keys)
    add("radix.blocks.rows+1", "RW", lambda F, k: F.n_blocks == k["ROWS"] + 1)
    add("radix.last_block_of_one_key", "RW", lambda F, k: F.last_block == 1 and F.n_blocks > 1)
    add("radix.quarter_without_a_key", "RW", lambda F, k: F.empty_quarter and F.last_block > 1)
    add("radix.small_sort_max", "RW", lambda F, k: F.n == k["SMALL_SORT_MAX"] and F.block_keys == k["BLOCK_SMALL"] == 2048
        and F.n_blocks == F.n // 2048)
    add("radix.small_sort_max+1", "RW", lambda F, k: F.n == k["SMALL_SORT_MAX"] + 1 and F.block_keys == k["BLOCK_LARGE"] == 4096
        and F.n_blocks == F.n // 4096 + 1)
    add("radix.one_digit_value_in_a_block", "RW", lambda F, k: F.n < 10000 and F.passes > 1 and F.per_pass()[0][0]
        and all(a for _, a in F.per_pass()))
    # ---- sweep
    chunk = lambda k: WG * k["PART_PER"]
    add("sweep.chunk", "RW", lambda F, k: F.n == chunk(k) == 8192 and F.chunks == [1])
    add("sweep.chunk+1", "RW", lambda F, k: F.n == chunk(k) + 1 == 8193 and F.chunks == [2] and F.flag_inner)
    add("sweep.single_block_max", "RW", lambda F, k: F.n == k["SINGLE_BLOCK_MAX"] == 2 * chunk(k) and F.chunks == [2] and F.flag_inner)
    add("sweep.single_block_max+1", "RW", lambda F, k: F.n == k["SINGLE_BLOCK_MAX"] + 1 and F.workgroups > 1)
    add("sweep.workgroups_of_one_chunk", "RW", lambda F, k: F.workgroups > 2 and set(F.chunks) == {1} and F.flag_span
        and 0 < F.n_flags)
    two = lambda F: F.workgroups > 2 and F.chunks.count(2) >= F.workgroups - 1 and max(F.chunks) == 2
    add("sweep.two_chunks.no_flag", "RW", lambda F, k: two(F) and F.n_flags == 0)
    add("sweep.two_chunks.every_flag", "RW", lambda F, k: two(F) and F.n_flags == F.n - 1)
    add("sweep.two_chunks.flags_at_the_borders", "RW", lambda F, k: two(F) and F.flags_exactly_at_borders and F.flag_inner and F.flag_span)
    add("sweep.two_chunks.smallest_n", "RW", lambda F, k: two(F) and F.n == (F.n_cu // 2) * chunk(k) + 1)
    # ---- the device entry that derives the key bits
    add("entry.stride_loop", "RW", lambda F, k: F.or_strided and F.or_bits_behind_first_stride >> 32
        and F.n == KEY_OR_WG * k["KEY_OR_PER_CU"] * F.n_cu + 1)
    return c


CLASSES = _classes()
FAMILIES = ("grid", "windows", "storage", "sort", "digits", "fields", "borders", "radix", "sweep", "entry")
# classes no input reaches, and why (none: every class of the list is shown)
EXEMPT = {}


# ------------------------------------------------------------------------------------------------------- builder
def _rng(name, attempt=0):
    return np.random.default_rng([zlib.crc32(name.encode()), attempt])


def deal(sorted_keys, runs, rng):
    """The keys of a window in input order: dealt into `runs` ascending runs (a number, or the runs' lengths) with a
    descent at every border between runs."""
    m = len(sorted_keys)
    if runs is None:
        return sorted_keys[rng.permutation(m)]
    lens = list(runs) if not isinstance(runs, int) else [m // runs + (1 if r < m % runs else 0) for r in range(runs)]
    assert sum(lens) == m and min(lens) > 0
    for _ in range(200):
        rid = rng.permutation(np.repeat(np.arange(len(lens)), lens))
        out = np.concatenate([sorted_keys[rid == r] for r in range(len(lens))])
        if int((out[1:] < out[:-1]).sum()) == len(lens) - 1:
            return out
    raise AssertionError("no dealing into %d runs" % len(lens))


def W(buckets, runs=None, lows="rand"):
    """One window of a description: {bucket: count}, the runs of its keys in input order, how the low bits are drawn
    ('rand': the whole range; 'edges': the whole range, the bucket's least and greatest value included)."""
    return dict(buckets=buckets, runs=runs, lows=lows)


def described(name, family, windows, max_dists, shows, expect=(), live=12, group=0, window_order="reverse", plans="SRW"):
    """A case from a description of its windows (module docstring).  The keys are `live` contiguous bits from bit 0,
    the leading nine the fine bucket; `group` is put into the bits from 32 up."""
    rng = _rng(name)
    low_bits = live - 9
    parts = []
    for w in windows:
        ks = []
        for b in sorted(w["buckets"]):
            cnt = w["buckets"][b]
            low = rng.integers(0, 1 << low_bits, size=cnt).astype(U)
            if w["lows"] == "edges" and cnt >= 2:
                low[0], low[1] = 0, (1 << low_bits) - 1
            ks.append((U(b) << U(low_bits)) | np.sort(low))
        parts.append(deal(np.concatenate(ks), w["runs"], rng))
    if window_order == "reverse":
        parts = parts[::-1]
    keys = np.concatenate(parts) | (U(group) << U(32))
    assert int(np.bitwise_or.reduce(keys)) == ((1 << live) - 1) | (group << 32), name
    return _case(name, family, keys, max_dists, plans, shows, expect)


def masked(name, family, n, mask, max_dists, shows, expect=(), plans="SRW", superset=None, plant=None):
    """n random keys under `mask` (every bit of it live); `plant`: {index: key} placed last."""
    rng = _rng(name)
    keys = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * U(2) + rng.integers(0, 2, size=n).astype(U)
    keys &= U(mask)
    if n:
        keys[n // 2] = U(mask)
    for i, v in (plant or {}).items():
        keys[i] = U(v)
    return _case(name, family, keys, max_dists, plans, shows, expect, superset)


def swept(name, family, n, borders, shows, expect=(), plans="SRW"):
    """Positions 0 .. n-1 along the sorted order with a jump of 10 at every position of `borders(j)`, shuffled: with a
    distance of 1 the flags lie exactly there, with 0 everywhere, with 2^32 - 1 nowhere."""
    j = np.arange(n, dtype=np.int64)
    pos = j + 10 * np.cumsum(borders(j) & (j > 0))
    keys = (U(3) << U(32)) | pos.astype(U)
    return _case(name, family, keys[_rng(name).permutation(n)], (0, 1, FAR), plans, shows, expect)


def _case(name, family, keys, max_dists, plans, shows, expect, superset=None):
    keys = np.ascontiguousarray(keys, U)
    keys.setflags(write=False)
    return Case(name, family, keys, tuple(max_dists), tuple(PLAN_OF[p] for p in plans), tuple(shows), tuple(expect), superset)


def spread(n_keys, lo, hi):
    """n_keys over the buckets lo .. hi, as evenly as they go."""
    nb = hi - lo + 1
    return {lo + i: n_keys // nb + (1 if i < n_keys % nb else 0) for i in range(nb)}


# --------------------------------------------------------------------------------------------------------- table
def _table():
    out = []
    S = "single_launch"
    D, M, SW = (lambda *a, **kw: out.append(described(*a, **kw))), (lambda *a, **kw: out.append(masked(*a, **kw))), \
        (lambda *a, **kw: out.append(swept(*a, **kw)))
    # ---- grid
    D("grid-1024-keys-one-window", "grid", [W(spread(1024, 0, 511), 40)], (0, 3),
      ["grid.one_window", "grid.1024", "windows.all_buckets"],
      [(S, "grid", 1), (S, "windows[0].M", 1024), (S, "windows[0].sort", "count"), (S, "windows[0].bucket_width", 9)])
    D("grid-1025-keys-two-windows", "grid", [W(spread(1025, 0, 511), 3)], (0, 3),
      ["grid.1025", "windows.empty_at_the_end", "storage.per.1025", "sort.runs.3"],
      [(S, "grid", 2), (S, "windows[0].M", 1025), (S, "windows[1].M", 0), (S, "windows[0].runs", 3), (S, "windows[0].rounds", 2)])
    M("grid-65537-keys", "grid", 65537, (1 << 20) - 1, (0, 2),
      ["grid.max_with_target_above_1024", "grid.slices_behind_the_end"],
      [(S, "grid", 64), (S, "target", 1025), (S, "slice_len", 1088), (S, "slices_behind", 3)])
    # ---- windows
    D("windows-trailing-empty-buckets", "windows", [W({255: 500, 256: 525}, 7)], (0, 8),
      ["windows.empty_at_the_end_with_buckets", "windows.empty_buckets_at_the_low_edge"],
      [(S, "grid", 2), (S, "windows[0].lo", 0), (S, "windows[0].hi", 257), (S, "windows[0].empty_lo", 255),
       (S, "windows[1].lo", 257), (S, "windows[1].hi", 512), (S, "windows[1].M", 0)])
    D("windows-both-edges-empty", "windows", [W({255: 500, 256: 400}, 4)], (0, 8),
      ["windows.empty_buckets_at_the_high_edge", "windows.empty_buckets_at_the_low_edge", "grid.one_window", "sort.runs.4"],
      [(S, "windows[0].empty_hi", 255), (S, "windows[0].n_buckets", 512), (S, "windows[0].rounds", 2)])
    D("windows-cut-on-and-around-bucket-borders", "windows",
      [W({0: 1024}, 2), W({1: 1023, 2: 1026}, 40), W({3: 600, 511: 1}, 5)], (0, 1),
      ["windows.cut_on_a_bucket_border", "windows.cut_one_key_before", "windows.cut_one_key_behind", "windows.1_bucket",
       "windows.2_buckets", "windows.empty_between_filled", "storage.per.1024", "sort.runs.2", "sort.runs.5"],
      [(S, "grid", 4), (S, "cut_offsets", {-1, 0, 1}), (S, "[w.M for w in F.windows]", [1024, 2049, 0, 601]),
       (S, "windows[1].n_buckets", 2), (S, "windows[0].n_buckets", 1), (S, "windows[3].lo", 3)])
    # ---- storage
    D("storage-5120-in-two-buckets", "storage", [W({0: 1000, 1: 4120}, 40), W({511: 1})], (0, 1),
      ["storage.win_cap", "windows.empty_between_filled"],
      [(S, "windows[0].M", 5120), (S, "windows[0].lds", True), (S, "windows[0].runs", 40), (S, "windows[0].per", 5),
       (S, "windows[0].low_passes", 1), (S, "windows[0].bucket_width", 1), (S, "windows[5].M", 1), (S, "grid", 6)])
    D("storage-5121-in-two-buckets", "storage", [W({0: 1000, 1: 4121}, 40), W({511: 1})], (0, 1),
      ["storage.win_cap+1"],
      [(S, "windows[0].M", 5121), (S, "windows[0].lds", False), (S, "windows[0].runs", 40), (S, "windows[0].per", 6),
       (S, "windows[0].low_passes", 1), (S, "windows[0].bucket_pass", True)])
    D("storage-per-steps", "storage", [W({0: 1024}, 33), W({1: 1025}, 32), W({2: 4096}, 3), W({3: 4097}, 5), W({511: 3}, 1)], (0, 1),
      ["storage.per.1024", "storage.per.1025", "storage.per.4096", "storage.per.4097", "sort.merge_with_per_5",
       "sort.runs.merge_runs", "sort.runs.merge_runs+1"],
      [(S, "grid", 11), (S, "[w.M for w in F.filled]", [1024, 1025, 4096, 4097, 3]), (S, "[w.index for w in F.filled]", [0, 1, 2, 6, 10]),
       (S, "[w.per for w in F.filled]", [1, 2, 4, 5, 1]), (S, "[w.runs for w in F.filled]", [33, 32, 3, 5, 1]),
       (S, "[w.sort for w in F.filled]", ["count", "merge", "merge", "merge", "none"]), (S, "windows[1].rounds", 5)])
    # ---- sort: a window of two buckets (512 + 512 keys) per run count; the low bits have eight values, so that equal keys
    # lie in every run
    runs = [1, 2, 3, 4, 5, 32, 33, [1, 700, 1, 3, 299, 20], [1000, 24]]
    D("sort-run-counts", "sort", [W({2 * i: 512, 2 * i + 1: 512}, r) for i, r in enumerate(runs)] + [W({510: 50, 511: 50}, 2)], (0, 1),
      ["sort.runs.%d" % r for r in (1, 2, 3, 4, 5)] + ["sort.runs.merge_runs", "sort.runs.merge_runs+1", "sort.a_run_of_one_key",
                                                      "sort.uneven_runs", "sort.ties_inside_a_pair_of_runs", "sort.ties_across_pairs_of_runs"],
      [(S, "grid", 10), (S, "[w.M for w in F.windows]", [1024] * 9 + [100]), (S, "[w.runs for w in F.windows]", [1, 2, 3, 4, 5, 32, 33, 6, 2, 2]),
       (S, "[w.rounds for w in F.windows]", [0, 1, 2, 2, 3, 5, 0, 3, 1, 1]), (S, "windows[6].sort", "count"),
       (S, "windows[7].run_lens", [1, 700, 1, 3, 299, 20]), (S, "windows[9].empty_lo", 492)])
    # ---- digits: random order (far more than 32 runs per window), every bit below `live` live
    for live, shows in ((5, ["digits.live_below_fine_bits", "radix.passes.1"]), (9, ["digits.bucket_only", "fields.one"]),
                        (10, ["digits.low_bits.1", "radix.passes.2"]), (18, ["digits.low_bits.9"]), (19, ["digits.low_bits.10", "radix.passes.3"]),
                        (27, ["digits.low_bits.18"]), (28, ["digits.low_bits.19", "radix.passes.4"]), (36, ["digits.low_bits.27"]),
                        (37, ["digits.low_bits.28", "radix.passes.5"]), (54, ["radix.passes.6"]), (63, ["radix.passes.7"]),
                        (64, ["digits.low_bits.55", "radix.passes.8", "fields.bit63"])):
        M("digits-live-%d" % live, "digits", 1300, (1 << live) - 1, (0, 1000), shows + ["radix.blocks.1", "radix.quarter_without_a_key"],
          [(S, "live", live), (S, "grid", 2), ("radix", "passes", _ceil(live, 9)), ("radix", "digit_bits", _ceil(live, _ceil(live, 9)))])
    # ---- fields
    four = 0xFFF | (0xF << 20) | (0xF << 32) | (1 << 63)
    M("fields-four", "fields", 1500, four, (0, 100, FAR), ["fields.limit", "fields.bit63"],
      [(S, "live", 21), (S, "fields", [(0, 12), (20, 24), (32, 36), (63, 64)])])
    five = 0x7 | (0x3 << 5) | (0xF << 10) | (0x7 << 33) | (0x3 << 40)
    M("fields-five-runs-merged", "fields", 1500, five, (0, 40), ["fields.merged_with_dead_bits"],
      [(S, "raw_runs", 5), (S, "fields", [(0, 7), (10, 14), (33, 36), (40, 42)]), (S, "live", 16)])
    scattered = 0x8040201008040201
    M("fields-eight-runs-merged", "fields", 1500, scattered, (0, FAR), ["fields.merged_with_dead_bits", "fields.bit63"],
      [(S, "raw_runs", 8), (S, "live", 40), (S, "fields", [(0, 37), (45, 46), (54, 55), (63, 64)])])
    M("fields-all-zero", "fields", 1500, 0, (0, 5), ["fields.all_zero"], [(S, "live", 1), (S, "windows[0].M", 1500), (S, "windows[1].M", 0)])
    M("fields-superset", "fields", 3000, 0xFFF | (0x3 << 32), (0, 2), ["fields.superset"], superset=0xFFFFF | (0xFF << 32),
      expect=[(S, "live", 14), (S, "grid", 3)])
    # ---- borders: the distance between the last key of a bucket and the first of the next is 1 (low bits 7 and 0)
    D("borders-adjacent-and-across-empties", "borders",
      [W({0: 1024}, 2, "edges"), W({1: 2049}, 3, "edges"), W({2: 3100}, 4, "edges"), W({3: 100, 511: 1}, 2, "edges")], (0, 1, FAR),
      ["borders.%s.%s@%d" % (v, w, d) for w in ("window_border", "one_empty_window", "empty_windows")
       for v, d in (("opens", 0), ("continues", 1))]
      + ["borders.max_dist_at_a_window_border@1", "borders.max_dist+1_at_a_window_border@0", "borders.max_dist_between_neighbours@0",
         "borders.max_dist+1_between_neighbours@0", "borders.max_dist_0@0"],
      [(S, "[w.index for w in F.filled]", [0, 1, 3, 6]), (S, "[x.dist for x in F.borders]", [1, 1, 1]),
       (S, "[x.empties_between for x in F.borders]", [0, 1, 2]), (S, "grid", 7)])
    # groups 0 .. 5, group g holds the positions 100 g .. 100 g + 100: a group ends where the next begins
    rng = _rng("borders-group-change")
    grp = rng.integers(0, 6, size=2500).astype(U)
    pos = grp * U(100) + rng.integers(0, 101, size=2500).astype(U)
    pos[:12] = np.repeat(np.arange(0, 600, 100), 2) + np.tile([0, 100], 6)
    grp[:12] = np.repeat(np.arange(6), 2)
    out.append(_case("borders-group-change", "borders", (grp << U(32)) | pos, (0, FAR), "SRW",
                     ["borders.group_change_at_equal_positions", "borders.max_dist_2^32-1@%d" % FAR, "borders.max_dist_0@0"], ()))
    M("borders-bit31", "borders", 2000, 0x80000FFF | (0x3 << 32), (1000, 1 << 31, FAR), ["borders.bit31@1000", "borders.bit31@%d" % (1 << 31)])
    # ---- radix
    M("radix-16-blocks", "radix", 32768, (1 << 18) - 1, (0, 2), ["radix.blocks.rows"], [("radix", "n_blocks", 16), ("radix", "row_batches", 1)])
    M("radix-17-blocks", "radix", 32769, (1 << 18) - 1, (0, 2), ["radix.blocks.rows+1", "radix.last_block_of_one_key"],
      [("radix", "n_blocks", 17), ("radix", "row_batches", 2), ("radix", "last_row_batch", 1)])
    M("radix-131072-keys", "radix", 131072, (1 << 20) - 1, (1,), ["radix.small_sort_max"], [("radix", "n_blocks", 64), (S, "grid", 64)])
    M("radix-131073-keys", "radix", 131073, (1 << 20) - 1, (1,), ["radix.small_sort_max+1", "radix.last_block_of_one_key"],
      [("radix", "n_blocks", 33), ("radix", "block_keys", 4096)], plans="RW")
    # the first block of 2048 keys holds digit 0 = 7 only; behind it every value of both digits
    rng = _rng("radix-one-digit-value-in-a-block")
    k18 = rng.integers(0, 1 << 18, size=4608).astype(U)
    k18[:2048] = (k18[:2048] & ~U(511)) | U(7)
    k18[2048:2560] = np.arange(512, dtype=U) * U(513)
    out.append(_case("radix-one-digit-value-in-a-block", "radix", k18, (0, 3), "SRW", ["radix.one_digit_value_in_a_block"],
                     [("radix", "passes", 2), ("radix", "digit_bits", 9)]))
    # ---- sweep
    chunk = 8192
    SW("sweep-8192-keys", "sweep", 8192, lambda j: j % chunk == 0, ["sweep.chunk"], [("radix", "part_grid", 1)])
    SW("sweep-8193-keys", "sweep", 8193, lambda j: j % chunk == 0, ["sweep.chunk+1@1"], [("radix", "part_grid", 1)])
    SW("sweep-16384-keys", "sweep", 16384, lambda j: j % chunk == 0, ["sweep.single_block_max@1"], [("radix", "part_grid", 1), ("radix", "span", 16384)])
    SW("sweep-16385-keys", "sweep", 16385, lambda j: j % 4096 == 0, ["sweep.single_block_max+1", "sweep.workgroups_of_one_chunk@1"],
       [("radix", "part_grid", 5), ("radix", "span", 4096), ("radix", "chunks", [1, 1, 1, 1, 1])])
    n2, span2 = 128 * chunk + 1, 9216
    SW("sweep-two-chunks", "sweep", n2, lambda j: (j % span2 == 0) | (j % span2 == chunk),
       ["sweep.two_chunks.no_flag@%d" % FAR, "sweep.two_chunks.every_flag@0", "sweep.two_chunks.flags_at_the_borders@1",
        "sweep.two_chunks.smallest_n"],
       [("radix", "part_grid", 128), ("radix", "span", span2), ("radix", "workgroups", 114), ("radix", "chunks", [2] * 113 + [1])], plans="RW")
    # ---- entry: the one key of another group sits behind the first stride of k_key_or; without its bit it would sort first
    # (too large for one launch: under that setting it takes the radix plan as well)
    n3 = 256 * 4 * 256 + 1
    M("entry-stride-loop", "entry", n3, 0xFFFFF, (0, 3), ["entry.stride_loop"], [("radix", "or_workgroups", 1024), ("radix", "or_strided", True)],
      plant={n3 - 1: 1 << 40})
    return collections.OrderedDict((c.name, c) for c in out)


CASES = _table()
TWO_CHUNK_CASE = "sweep-two-chunks"
DEVICE_ENTRY_FAMILIES = ("fields", "borders", "entry")
POISON_FAMILIES = ("storage", "sweep")


def family(name):
    return [c for c in CASES.values() if c.family == name]


@functools.lru_cache(maxsize=None)
def case_facts(name, max_dist, plan, n_cu=256, superset=False):
    c = CASES[name]
    return facts(c.keys, max_dist, plan, n_cu, key_bits=c.superset if superset else None)


COMBINED_MAX_KEYS = 7000      # cases of at most this many keys, below bit 40, go into the combined batch


@functools.lru_cache(maxsize=1)
def combined():
    """The small cases' keys as ONE batch, case c under the group field c << 40 (input order: case after case).
    -> (keys, {name: first index})."""
    parts, at, n = [], {}, 0
    for c in CASES.values():
        if len(c.keys) <= COMBINED_MAX_KEYS and (not len(c.keys) or int(c.keys.max()) < 1 << 40):
            at[c.name] = n
            parts.append(c.keys | (U(len(parts)) << U(40)))
            n += len(c.keys)
    keys = np.concatenate(parts)
    keys.setflags(write=False)
    assert n <= 131072
    return keys, at


COMBINED_FAMILIES = ("storage", "sort", "borders")


def shown_by(F, k=None, families=None):
    """The classes (of `families`) the facts F show on their plan."""
    k = k or K
    return [cid for cid, (fam, plans, pred) in CLASSES.items()
            if pred is not None and F.plan in plans and (families is None or fam in families)
            and (F.one_launch or plans != ("single_launch",)) and pred(F, k)]


def split_shows(entry):
    cid, _, d = entry.partition("@")
    return cid, (int(d) if d else None)


def check_preconditions(k=None, n_cu=256, cases=None):
    """Every case shows what it lists and holds the numbers its name promises; every class of CLASSES is shown on every
    plan it applies to.  `k`: the constants (default K); `n_cu`: the device's CU count (the table is laid out for 256)."""
    k = k or K
    default = cases is None
    cases = list((cases or CASES).values())
    shown = set()
    for c in cases:
        cache = {}

        def F(plan, d, superset=False):
            key = (plan, d, superset)
            if key not in cache:
                cache[key] = facts(c.keys, d, plan, n_cu, c.superset if superset else None, k)
            return cache[key]
        for entry in c.shows:
            cid, d = split_shows(entry)
            fam, plans, pred = CLASSES[cid]
            for plan in plans:
                if plan not in c.plans:
                    continue
                if cid == "fields.superset":
                    own, sup = F(plan, c.max_dists[0]), F(plan, c.max_dists[0], True)
                    assert sup.live > own.live and sup.fields != own.fields, "%s: the superset keeps the fields" % c.name
                    a, b = F("single_launch", c.max_dists[0]), F("single_launch", c.max_dists[0], True)
                    assert [(w.lo, w.hi, w.M) for w in a.windows] != [(w.lo, w.hi, w.M) for w in b.windows] and a.low_bits != b.low_bits, \
                        "%s: the superset keeps the window cut" % c.name
                    shown.add((cid, plan))
                    continue
                ds = c.max_dists if d is None else (d,)
                assert set(ds) <= set(c.max_dists), (c.name, entry)
                assert all(pred(F(plan, x), k) for x in ds), "%s does not show %s on the %s plan (n_cu %d: the table is laid out " \
                    "for 256 CUs and has to move with the device)" % (c.name, cid, plan, n_cu)
                shown.add((cid, plan))
        for plan, expr, value in c.expect:
            if plan not in c.plans:
                continue
            f = F(plan, c.max_dists[0])
            got = eval(expr if "F." in expr else "F." + expr, {"F": f})
            assert got == value, "%s: %s on the %s plan is %r, not %r (n_cu %d)" % (c.name, expr, plan, got, value, n_cu)
    if default:
        missing = [(cid, p) for cid, (fam, plans, _) in CLASSES.items() for p in plans if (cid, p) not in shown and cid not in EXEMPT]
        assert not missing, missing
        assert not EXEMPT
    return shown
