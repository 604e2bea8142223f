"""Plain-loop restatement of svx_cigar_lift and svx_cover_locate (include/svx.h): the yardstick of
tests/test_gpu_lift.py, tests/test_gpu_cover_locate.py and tests/test_genotype_host.py.  Loops over tuples only — no
prefix sums, no searches, no numpy.

  lift(ops, ref_start, r)      ops: [(op code, length)] of one alignment; returns (query offset, state)
  lift_batch(...)              the batch in the layout of Context.cigar_lift, as lists
  locate(lists, queries)       svx_cover_locate: the index inside each list of the covering entry, NONE without one"""

OUTSIDE, ALIGNED, DELETED, END = 0, 1, 2, 3
NONE = 0xFFFFFFFF
CODES = "MIDNSHP=XB"


def lift(ops, ref_start, r):
    ref, qry, last = ref_start, 0, None          # qry counts SEQ bases: M I S = X (H, P, D, N: none)
    for op, n in ops:
        name = CODES[op] if op < len(CODES) else "?"
        cr = n if name in "MDN=X" else 0
        cq = n if name in "MIS=X" else 0
        if cr and ref <= r < ref + n:
            return (qry + (r - ref), ALIGNED) if cq else (qry, DELETED)   # D / N: the next aligned base
        ref += cr
        qry += cq
        if cr:
            last = qry
    return (last, END) if (last is not None and r == ref) else (0, OUTSIDE)


def lift_batch(cigar, aln_off, ref_start, q_aln, q_ref):
    """cigar: packed words (length << 4 | op) of all alignments; returns ([query offsets], [states])."""
    alignments = []
    for a in range(len(aln_off) - 1):
        alignments.append([(int(w) & 15, int(w) >> 4) for w in cigar[int(aln_off[a]):int(aln_off[a + 1])]])
    query, state = [], []
    for a, r in zip(q_aln, q_ref):
        x, s = lift(alignments[int(a)], int(ref_start[int(a)]), int(r))
        query.append(x)
        state.append(s)
    return query, state


def locate(lists, queries):
    """out[l][q]: of the entries (start, end) of lists[l] with start <= lo the one with the largest end, the lowest
    index among equal ends — its index when that end is >= hi, NONE otherwise."""
    out = []
    for intervals in lists:
        row = []
        for lo, hi in queries:
            best = None
            for i, (start, end) in enumerate(intervals):
                if start <= lo and (best is None or end > intervals[best][1]):
                    best = i
            row.append(best if best is not None and intervals[best][1] >= hi else NONE)
        out.append(row)
    return out
