"""Where a sample could be called at all: the reference ranges that exactly ONE alignment of a haplotype's assembly lies
over (`--callable_bed`).

Input: the intervals `(tid, start, end)` of the records COLLECT visited, one list per haplotype — SVIM_COLLECT._coverage_of,
what `--keep_coverage` persists as coverage.svxt.  All lists of a call go to the device ONCE (svx_cover_single: per list the
maximal ranges on which depth is 1 and the covering alignment stays the same; two alignments that abut give two abutting
segments — an alignment boundary is a breakpoint of the assembly).  The rest is host arithmetic on sorted, disjoint
segment lists:
  * a sample's callable set — the list's segments for a haploid run, the intersection of the two lists' segments for a
    diploid one (a line therefore never crosses an alignment end of either haplotype; abutting lines stay separate):
    OUT/callable.bed, contig / start / end, 0-based and half-open, in the header's contig order;
  * a cohort's count track — how many samples' callable sets contain a range (+1 / -1 events, a running sum), ranges
    without a sample left out and adjacent ranges with the same count joined: OUT/cohort.callable.bed, with the count
    as the fourth column.
Keys are contig << 32 | position throughout, as on the device."""
import os

import numpy as np

from svim_asm_amd import _lib

SAMPLE_NAME = "callable.bed"
COHORT_NAME = "cohort.callable.bed"
_EMPTY = np.zeros(0, np.uint64)


def check_min_length(options):
    n = int(getattr(options, "callable_min_length", 0) or 0)
    if n < 0:
        raise ValueError("--callable_min_length %d: a number of bases, 0 or more" % n)
    return n


def keys_of(lists, min_length=0):
    """(start_key, end_key, list_off) of (tid, start, end) lists for svx_cover_single, without the alignments of fewer
    than `min_length` reference bases: they neither cover nor disturb."""
    starts, ends, counts = [], [], []
    for tid, start, end in lists:
        tid, start, end = (np.asarray(a, dtype=np.int64) for a in (tid, start, end))
        keep = (end - start) >= min_length  # (0: all of them — none is empty, a record without reference bases gives no interval)
        c = tid[keep].astype(np.uint64) << np.uint64(32)
        starts.append(c | start[keep].astype(np.uint64))
        ends.append(c | end[keep].astype(np.uint64))
        counts.append(int(keep.sum()))
    list_off = np.zeros(len(counts) + 1, np.uint64)
    if counts:
        np.cumsum(counts, out=list_off[1:])
    cat = lambda parts: np.concatenate(parts) if parts else _EMPTY
    return cat(starts), cat(ends), list_off


def single_segments(lists, ctx, min_length=0):
    """[(lo, hi)] per list, uint64 keys: its single-coverage segments, all lists in ONE device call."""
    if not lists:
        return []
    seg_lo, seg_hi, seg_off = ctx.cover_single(*keys_of(lists, min_length))
    seg_lo, seg_hi = np.asarray(seg_lo, dtype=np.uint64), np.asarray(seg_hi, dtype=np.uint64)
    off = [int(x) for x in seg_off]
    return [(seg_lo[off[l]:off[l + 1]], seg_hi[off[l]:off[l + 1]]) for l in range(len(lists))]


def intersect(a, b):
    """The ranges inside a segment of `a` AND a segment of `b` — two sorted, disjoint lists of (lo, hi); every pair that
    overlaps gives a range of its own, in ascending order."""
    (a_lo, a_hi), (b_lo, b_hi) = a, b
    if len(a_lo) == 0 or len(b_lo) == 0:
        return _EMPTY, _EMPTY
    first = np.searchsorted(b_hi, a_lo, side="right")  # the first segment of b that ends behind a's start
    last = np.searchsorted(b_lo, a_hi, side="left")    # the first one that starts at or behind a's end
    n = np.maximum(last - first, 0)
    ia = np.repeat(np.arange(len(a_lo)), n)
    ib = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(first, n)
    return np.maximum(a_lo[ia], b_lo[ib]), np.minimum(a_hi[ia], b_hi[ib])


def sample_set(segments):
    """A sample's callable set from the segments of its 1 (haploid) or 2 (diploid) lists."""
    if len(segments) == 1:
        return segments[0]
    if len(segments) == 2:
        return intersect(segments[0], segments[1])
    raise ValueError("a sample has %d coverage lists (1: haploid, 2: diploid)" % len(segments))


def count_track(sample_sets):
    """(lo, hi, count): the ranges that `count` >= 1 of the samples' sets contain, adjacent ranges with the same count
    joined."""
    los = [s[0] for s in sample_sets if len(s[0])]
    if not los:
        return _EMPTY, _EMPTY, np.zeros(0, np.int64)
    lo, hi = np.concatenate(los), np.concatenate([s[1] for s in sample_sets if len(s[0])])
    key = np.concatenate([lo, hi])
    step = np.concatenate([np.ones(len(lo), np.int64), -np.ones(len(hi), np.int64)])
    order = np.argsort(key, kind="stable")
    key, step = key[order], step[order]
    at = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))  # one event per distinct key: the sum of its steps
    depth = np.cumsum(np.add.reduceat(step, at))
    key = key[at]
    # a new range where the count changes
    edge = np.flatnonzero(np.concatenate([[True], depth[1:] != depth[:-1]]))
    lo, count = key[edge], depth[edge]
    hi = np.concatenate([lo[1:], key[-1:]])
    keep = count > 0
    return lo[keep], hi[keep], count[keep]


def bed_text(contigs, lo, hi, count=None):
    """contig <tab> start <tab> end [<tab> count] per range; a range lies on one contig (it is inside an alignment)."""
    lo, hi = np.asarray(lo, dtype=np.uint64), np.asarray(hi, dtype=np.uint64)
    tid = (lo >> np.uint64(32)).tolist()
    a, b = (lo & np.uint64(0xFFFFFFFF)).tolist(), (hi & np.uint64(0xFFFFFFFF)).tolist()
    if count is None:
        return "".join("%s\t%d\t%d\n" % (contigs[t], s, e) for t, s, e in zip(tid, a, b))
    return "".join("%s\t%d\t%d\t%d\n" % (contigs[t], s, e, c) for t, s, e, c in zip(tid, a, b, np.asarray(count).tolist()))


def _write(path, text):
    with open(path + ".tmp", "w") as out:
        out.write(text)
    os.replace(path + ".tmp", path)
    return path


def write_sample_bed(contigs, lists, options, working_dir, ctx=None):
    """WORKING_DIR/callable.bed of one sample from its coverage lists: one svx_cover_single for the sample's lists."""
    min_length = check_min_length(options)
    ctx = ctx or _lib.default_context(getattr(options, "device", 0) or 0)
    lo, hi = sample_set(single_segments(list(lists), ctx, min_length))
    return _write(os.path.join(working_dir, SAMPLE_NAME), bed_text(list(contigs), lo, hi))


def write_cohort_bed(contigs, coverages, options, working_dir, ctx=None, sample_names=None):
    """WORKING_DIR/cohort.callable.bed from the samples' Coverage objects (SVIM_MERGE.read_coverage): all lists of all
    samples in ONE svx_cover_single, then per sample its set and over the samples the count track."""
    min_length = check_min_length(options)
    coverages = list(coverages)
    names = list(sample_names) if sample_names is not None else ["#%d" % (k + 1) for k in range(len(coverages))]
    for name, cov in zip(names, coverages):
        if len(cov.lists) not in (1, 2):
            raise ValueError("the coverage of sample %s has %d lists (1: haploid, 2: diploid)" % (name, len(cov.lists)))
    ctx = ctx or _lib.default_context(getattr(options, "device", 0) or 0)
    segments = single_segments([t for cov in coverages for t in cov.lists], ctx, min_length)
    sets, at = [], 0
    for cov in coverages:
        sets.append(sample_set(segments[at:at + len(cov.lists)]))
        at += len(cov.lists)
    lo, hi, count = count_track(sets)
    return _write(os.path.join(working_dir, COHORT_NAME), bed_text(list(contigs), lo, hi, count))
