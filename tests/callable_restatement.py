"""Plain-loop restatement of --callable_bed: the yardstick of tests/test_callable_host.py and
tests/test_gpu_callable.py.  Tuples and loops only — no prefix maxima, no slots, no numpy.

  single(lists)                 svx_cover_single: per list of (start_key, end_key) its single-coverage segments
  intersect(a, b)               the ranges inside a segment of a and a segment of b
  sample_set(segments)          a sample's callable set from its 1 or 2 lists' segments
  count_track(sample_sets)      (lo, hi, count): how many samples' sets contain a range, equal neighbours joined
  bed_text(contigs, rows)       the file's text

An entry is the half-open key range [start, end); depth(p) is the number of entries of the list with start <= p < end;
a list's segments are the maximal ranges on which depth is 1 and the one covering entry is the same entry throughout."""


def key(contig, position):
    return (contig << 32) | position


def single_one(entries):
    """Segments of one list (sorted by start): between two neighbouring keys of the sorted distinct starts and ends no
    entry begins or ends, so the set of entries over such an elementary piece is one set; consecutive pieces whose set
    is the same single entry are joined."""
    points = sorted(set([s for s, _ in entries] + [e for _, e in entries]))
    out = []
    current = None  # [entry, lo, hi]
    for a, b in zip(points, points[1:]):
        over = []
        for i, (s, e) in enumerate(entries):
            if s > a:
                break  # (sorted by start: none of the later ones has begun)
            if s <= a and b <= e:
                over.append(i)
        if len(over) == 1 and current is not None and current[0] == over[0] and current[2] == a:
            current[2] = b
            continue
        if current is not None:
            out.append((current[1], current[2]))
            current = None
        if len(over) == 1:
            current = [over[0], a, b]
    if current is not None:
        out.append((current[1], current[2]))
    return out


def single(lists):
    return [single_one(entries) for entries in lists]


def flat(per_list):
    """(seg_lo, seg_hi, seg_off) as svx_cover_single lays them out."""
    lo, hi, off = [], [], [0]
    for segs in per_list:
        lo += [a for a, _ in segs]
        hi += [b for _, b in segs]
        off.append(len(lo))
    return lo, hi, off


def intersect(a, b):
    out = []
    for a_lo, a_hi in a:
        for b_lo, b_hi in b:
            lo, hi = max(a_lo, b_lo), min(a_hi, b_hi)
            if lo < hi:
                out.append((lo, hi))
    return sorted(out)


def sample_set(segments):
    if len(segments) == 1:
        return list(segments[0])
    first, second = segments
    return intersect(first, second)


def count_track(sample_sets):
    points = sorted(set(p for segs in sample_sets for seg in segs for p in seg))
    out = []
    for a, b in zip(points, points[1:]):
        n = 0
        for segs in sample_sets:
            for lo, hi in segs:
                if lo <= a and b <= hi:
                    n += 1
        if n == 0:
            continue
        if out and out[-1][1] == a and out[-1][2] == n:
            out[-1] = (out[-1][0], b, n)
        else:
            out.append((a, b, n))
    return out


def bed_text(contigs, rows):
    """rows of (lo_key, hi_key) or (lo_key, hi_key, count)."""
    lines = []
    for row in rows:
        lo, hi = row[0], row[1]
        assert lo >> 32 == hi >> 32
        fields = [contigs[lo >> 32], str(lo & 0xFFFFFFFF), str(hi & 0xFFFFFFFF)] + [str(v) for v in row[2:]]
        lines.append("\t".join(fields) + "\n")
    return "".join(lines)
