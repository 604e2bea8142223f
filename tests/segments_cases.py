"""The case table of the split-segment chain: which inputs reach which leaf of tests/segments_restatement.py, on which
side of which comparison.

A case is a function cur -> nxt and the leaf the pair must reach.  It is made of relative quantities (the gap on the
read, the strands, same or other contig, where nxt lies on the reference relative to cur), so cases stand alone as
reads of two segments (`pairs`) or follow each other in one read (`chains`).  The table depends on the parameter set:
every threshold of that set is approached from -1, 0 and +1.

Segments are 3000-3399 long and every |gap| on the read is at most 1100, so the (q_start, q_end) order is the order of
construction.  The exceptions are the cases that NEED another length, and they say so (cur_len / nxt_len): an
inversion's size is at least the length of one of its two segments (cases 1 and 4: nxt, cases 2 and 3: cur), so the
lower edge of its window wants a segment of min_sv_size +-1 and the upper edge one of max_sv_size +-1; a tandem
duplication that is not fully covered has both segments inside max_sv_size.  Such a case follows only a segment of
exactly that length, or starts a read.  Every segment is as long on the reference as on the read, so one `M` run
describes it (the fused forms take CIGARs).  Reference coordinates start at 5 * 10^6: nothing goes negative."""
import collections
import random

import numpy as np

from tests import segments_restatement as R

Seg = R.Seg
DEFAULT = (40, 100000, 50, 50, 50, 50)
DISTINCT = (40, 1000, 30, 60, 70, 20)   # all six differ pairwise
ZERO = (50, 20, 0, 0, 0, 0)            # empty window: min_sv_size > max_sv_size
PARAM_SETS = collections.OrderedDict((("DEFAULT", DEFAULT), ("DISTINCT", DISTINCT), ("ZERO", ZERO)))
N_CONTIGS = 3
CONTIG_RANK = [2, 0, 1]                 # rank of contig id under the str order of its name: not the id order
REF0 = 5000000
LONG = (3000, 3399)

Case = collections.namedtuple("Case", "name leaf cur_rev nxt_rev gap other place nxt_len cur_len any_cur")


def _long_len(k):
    return LONG[0] + (k * 37) % 400


def tree_cases(params):
    """The table for one parameter set."""
    mn, mx, qgt, qot, rgt, rot = params
    big = mx >= 7000  # two segments of 3000-3399 fit into max_sv_size
    assert big or mx <= 2000
    cases = []

    def add(name, leaf, cur_rev, nxt_rev, gap, place, other=False, nxt_len=None, cur_len=None, any_cur=False):
        assert abs(gap) <= 1100 and name not in [c.name for c in cases], name
        if gap < -qot or (gap > qgt and not leaf.startswith("ins")):
            leaf = "none"  # every leaf but the insertions lies behind both tests of the gap on the read
        cases.append(Case(name, leaf, cur_rev, nxt_rev, gap, other, place, nxt_len, cur_len, any_cur))

    for rev in (0, 1):
        s = ".rev" if rev else ".fwd"

        def same(name, d, d_read, d_ref, leaf, **kw):
            # forward: distance_on_reference = nxt.ref_start - cur.ref_end; reverse: cur.ref_start - nxt.ref_end
            if rev:
                place = lambda cur, n, d_ref=d_ref: cur.ref_start - d_ref - n
            else:
                place = lambda cur, n, d_ref=d_ref: cur.ref_end + d_ref
            add("same.%s%+d%s" % (name, d, s), leaf + s if leaf != "none" else leaf, rev, rev, d_read, place, **kw)

        for d in (-1, 0, 1):
            # a deletion beyond max_sv_size behind the read-overlap test: a breakend, or nothing
            same("read_overlap", d, -qot + d, -qot + d + mx + 7, "none" if d < 0 else "bnd")
            # an insertion of min_sv_size + 3 on one side of the reference-overlap test, a tandem duplication on the other
            d_ref = -rot + d
            d_read = d_ref + mn + 3
            assert d_read >= -qot
            same("ref_overlap", d, d_read, d_ref, ("ins" if d_ref <= rgt else "none") if d >= 0 else "dup_full")
            same("ins.min", d, mn + d, 0, "ins" if d >= 0 else "none")
            assert rgt + d >= -rot or rgt + d + mn + 5 > qgt
            same("ins.ref_gap", d, rgt + d + mn + 5, rgt + d, "ins" if -rot <= rgt + d <= rgt else "none")
            dev = -mx + d  # the lower edge of the deletion window, which is the breakend's edge too
            same("del.lo", d, 0, -dev, "bnd" if d < 0 else ("del" if dev <= -mn else "none"))
            dev = -mn + d
            same("del.hi", d, 0, -dev, ("del" if d <= 0 else "none") if dev >= -mx else "bnd")
            dev = -(mn + 5)
            same("del.read_gap", d, qgt + d, qgt + d - dev, ("del" if dev >= -mx else "bnd") if d <= 0 else "none")
            dev = -(mx + 7)
            same("bnd.read_gap", d, qgt + d, qgt + d - dev, "bnd" if d <= 0 else "none")
            same("dup.read_gap", d, qgt + d, -(rot + mn + 5), "dup_full" if d <= 0 else "none")
            d_read = min(qgt, mn + d - rot - 1)
            d_ref = d_read - (mn + d)
            assert d_read >= -qot and d_ref < -rot
            same("dup.min", d, d_read, d_ref, "dup_full" if d >= 0 else "none")
            # fully covered or not: forward nxt.ref_end > cur.ref_start, reverse nxt.ref_start < cur.ref_end
            part = "dup_part" if big else "dup_bnd"
            if rev:
                add("same.dup.full%+d%s" % (d, s), ("dup_full" if d < 0 else part) + s, 1, 1, 0, lambda cur, n, d=d: cur.ref_end + d)
            else:
                add("same.dup.full%+d%s" % (d, s), ("dup_full" if d > 0 else part) + s, 0, 0, 0, lambda cur, n, d=d: cur.ref_start + d - n)
            # not fully covered, inside max_sv_size or not: both segments within max_sv_size, so short ones unless it is big
            if big:
                same("dup.max", d, 0, -mx + d, "dup_part" if d >= 0 else "dup_bnd")
            elif mx - 1 >= mn and (mx - 1) // 2 >= 1 and -mx + 1 < -rot:
                h = (mx - 1) // 2
                same("dup.max", d, 0, -mx + d, "dup_part" if d >= 0 else "dup_bnd", cur_len=h, nxt_len=h)

    # inversions: fr = forward then reverse (cases 1 and 3), rf = reverse then forward (cases 2 and 4)
    for tag, cur_rev, near, far in (("fr", 0, "1", "3"), ("rf", 1, "2", "4")):
        nxt_rev = 1 - cur_rev
        at_x = lambda x: (lambda cur, n: cur.ref_end + x)           # nxt.ref_start - cur.ref_end = x: cases 1, 2
        at_y = lambda y: (lambda cur, n: cur.ref_start - y - n)     # cur.ref_start - nxt.ref_end = y: cases 3, 4
        hit = lambda c: "inv" + c + ("" if big else "_bnd")         # segments of 3000-3399: inside the window or above it
        for d in (-1, 0, 1):
            add("%s.read_overlap%+d" % (tag, d), "none" if d < 0 else hit(near), cur_rev, nxt_rev, -qot + d, at_x(10))
            add("%s.read_gap%+d" % (tag, d), hit(near) if d <= 0 else "none", cur_rev, nxt_rev, qgt + d, at_x(10))
            add("%s.case%s%+d" % (tag, near, d), "none" if d < 0 else hit(near), cur_rev, nxt_rev, 0, at_x(-rot + d))
            add("%s.case%s%+d" % (tag, far, d), "none" if d < 0 else hit(far), cur_rev, nxt_rev, 0, at_y(-rot + d))
            # the size is the length of nxt (cases 1, 4) or of cur (cases 2, 3) when the gap and x / y are 0
            for c, place, which in ((near, at_x(0), "nxt_len" if tag == "fr" else "cur_len"),
                                    (far, at_y(0), "cur_len" if tag == "fr" else "nxt_len")):
                add("%s.case%s.min%+d" % (tag, c, d), "inv" + c + ("" if d >= 0 and mn + d <= mx else "_bnd"), cur_rev, nxt_rev,
                    0, place, **{which: mn + d})
                if mn <= mx + d:  # (otherwise the lower edge has failed before the upper one is looked at)
                    add("%s.case%s.max%+d" % (tag, c, d), "inv" + c + ("" if d <= 0 else "_bnd"), cur_rev, nxt_rev,
                        0, place, **{which: mx + d})

    # another contig: only the gap on the read counts, for each of the four strand pairs
    for cur_rev in (0, 1):
        for nxt_rev in (0, 1):
            leaf = "other." + "fr"[cur_rev] + "fr"[nxt_rev]
            for d in (-1, 0, 1):
                add("%s.read_overlap%+d" % (leaf, d), "none" if d < 0 else leaf, cur_rev, nxt_rev, -qot + d,
                    lambda cur, n: cur.ref_start + 777, other=True, any_cur=True)
                add("%s.read_gap%+d" % (leaf, d), leaf if d <= 0 else "none", cur_rev, nxt_rev, qgt + d,
                    lambda cur, n: cur.ref_start + 777, other=True, any_cur=True)
    return cases


def apply(case, cur, k):
    """nxt of `case` behind `cur`; k picks the length where the case leaves it open."""
    n = case.nxt_len or _long_len(k)
    q_start = cur.q_end + case.gap
    ref_start = case.place(cur, n)
    return Seg(q_start, q_start + n, (cur.ref_id + 1) % N_CONTIGS if case.other else cur.ref_id, ref_start, ref_start + n,
               case.nxt_rev)


def first_segment(case, r):
    n = case.cur_len or _long_len(r + 5)
    ref_start = REF0 + 1000 * (r % 997)
    return Seg(40 + r % 9, 40 + r % 9 + n, r % N_CONTIGS, ref_start, ref_start + n, case.cur_rev)


def follows(case, cur):
    """May `case` stand behind the segment `cur`?"""
    n = cur.q_end - cur.q_start
    if case.cur_rev != cur.is_reverse or n + case.gap <= 0:
        return False
    if case.cur_len is not None:
        return n == case.cur_len
    return case.any_cur or LONG[0] <= n <= LONG[1]


def _read(segs, r, steps):
    """steps: the cases of the adjacent pairs in (q_start, q_end) order; segs in the order they are handed over."""
    return dict(segs=list(segs), read_len=max(s.q_end for s in segs) + 11 + r if segs else 17 + r, steps=list(steps))


def _distinct_lengths(reads):
    """No read has the read length of one of the 32 in front of it (the reads of a workgroup of k_segments): a lane
    that took a neighbour's length shows in the reverse-strand insertions."""
    for i, rd in enumerate(reads):
        while rd["read_len"] in [x["read_len"] for x in reads[max(0, i - 32):i]]:
            rd["read_len"] += 1
    return reads


def pairs(cases):
    """Every case as a read of two segments, in table order."""
    out = []
    for i, c in enumerate(cases):
        cur = first_segment(c, i)
        out.append(_read([cur, apply(c, cur, i)], i, [i]))
    return _distinct_lengths(out)


def _walk(rng, cases, k, r, want=(), first=None):
    """A read of k segments: a walk through the table, handed over in shuffled order."""
    if k == 0:
        return _read([], r, [])
    if first is None:
        first = rng.choice(sorted(want)) if want else rng.randrange(len(cases))
    segs, steps = [first_segment(cases[first], r)], []
    for step in range(k - 1):
        opts = [first] if step == 0 else [i for i, c in enumerate(cases) if follows(c, segs[-1])]
        pref = [i for i in opts if i in want and i not in steps]
        i = rng.choice(pref or opts)
        segs.append(apply(cases[i], segs[-1], r + step))
        steps.append(i)
    shuffled = list(segs)
    rng.shuffle(shuffled)
    return _read(shuffled, r, steps)


SHUFFLE_SIZES, SERIAL_SIZES = (3, 4, 5, 6, 7, 8), (9, 16, 17, 40)


def chains(cases, seed=1):
    """Reads of 3-8 segments (the shuffle path) and of 9, 16, 17 and 40 (the serial path), as many as it takes for
    either kind to have used every case."""
    rng = random.Random(seed)
    out = []
    for sizes in (SHUFFLE_SIZES, SERIAL_SIZES):
        want, n = set(range(len(cases))), 0
        while want or n < len(sizes):
            assert n < 40 * len(cases)
            special = sorted(i for i in want if cases[i].cur_len is not None)  # these start a read
            rd = _walk(rng, cases, sizes[n % len(sizes)], len(out), want, rng.choice(special) if special else None)
            want -= set(rd["steps"])
            out.append(rd)
            n += 1
    return _distinct_lengths(out)


PACKED_COUNTS = (1, 7, 8, 9, 31, 32, 33)
FILLERS = (0, 1, 3, 8, 9)


def packed(cases, n_reads, seed=2):
    """The reads of `pairs` with reads of 0, 1, 3, 8 and 9 segments between them, n_reads in all."""
    rng = random.Random(seed)
    two = pairs(cases)
    fill = [_walk(rng, cases, FILLERS[j % len(FILLERS)], 1000 + j) for j in range(4 * len(FILLERS))]
    out = []
    for j in range(n_reads):
        src = two[(j // 2) % len(two)] if j % 2 == 0 else fill[(j // 2) % len(fill)]
        out.append(dict(src, read_len=src["read_len"] + j % 50021))
    return _distinct_lengths(out)


def ties(cases, seed=3):
    """Reads in which 2, 3 and 8 segments share (q_start, q_end) and differ on the reference and in strand, bare, between
    two other segments and with a walk behind them (more than 8 segments), each in several input orders."""
    rng = random.Random(seed)
    out = []
    for m in (2, 3, 8):
        for form in ("bare", "flanked", "long"):
            lead = Seg(60, 60 + 3100, 1, REF0 + 7000, REF0 + 7000 + 3100, 0)
            q0 = lead.q_end + 5
            tied = [Seg(q0, q0 + 20, 1 if j % 3 != 2 else 2, lead.ref_end - 60 + 40 * j, lead.ref_end - 40 + 40 * j, j % 2)
                    for j in range(m)]
            segs = list(tied)
            if form != "bare":
                tail = [Seg(q0 + 20 + 8, q0 + 28 + 3050, 1, lead.ref_end + 130, lead.ref_end + 130 + 3050, 1)]
                for step in range(7 if form == "long" else 0):
                    opts = [c for c in cases if follows(c, tail[-1])]
                    tail.append(apply(rng.choice(opts), tail[-1], step))
                segs = [lead] + tied + tail
            orders = [list(segs), list(reversed(segs))]
            for _ in range(3):
                orders.append(rng.sample(segs, len(segs)))
            for o in orders:
                out.append(_read(o, len(out), []))
    return _distinct_lengths(out)


def mirrored(cases=None):
    """Reads A B C with B on another contig and C where A ended (forward) or in front of where A began (reverse): two
    breakends that mirror each other, |pos1 - pos2| 19 (an interspersed duplication of B's 500 bases) and 20 (none)."""
    out = []
    for rev in (0, 1):
        for near in (-20, -19, 0, 19, 20):
            a = Seg(50, 3050, 0, REF0 + 9000, REF0 + 12000, rev)
            b = Seg(3050, 3550, 1, REF0 + 400000, REF0 + 400500, rev)
            at = a.ref_start + 1 + near - 3000 if rev else a.ref_end - 1 + near
            c = Seg(3550, 6550, 0, at, at + 3000, rev)
            out.append(_read([c, a, b], len(out), []))
    return _distinct_lengths(out)


def to_arrays(reads, seg_dtype):
    """(segs, read_off, read_len) as svx_segments_classify takes them."""
    rows = [tuple(s) for rd in reads for s in rd["segs"]]
    segs = np.array(rows, dtype=seg_dtype) if rows else np.zeros(0, dtype=seg_dtype)
    off = np.concatenate(([0], np.cumsum([len(rd["segs"]) for rd in reads]))).astype(np.uint32)
    return segs, off, np.array([rd["read_len"] for rd in reads], np.int32)


def expected_raw(reads, params):
    """classify_read of every read, as rows of eight int32 (pad 0)."""
    rows = [rec + (0,) for rd in reads for rec in R.classify_read(rd["segs"], rd["read_len"], params)]
    return np.array(rows, np.int32).reshape(-1, 8)


# ------------------------------------------------------------------------------------------ post-pass table
POST_PARAMS = ((40, 100000), (10, 300))
POST_CONTIGS = 12
POST_RANK = [k for _, k in sorted((i, k) for k, i in enumerate(sorted(range(POST_CONTIGS), key=lambda i: "chr%d" % (i + 1))))]
# chr1 chr10 chr11 chr12 chr2 ...: contig 9 (chr10) sorts in front of contig 1 (chr2)


def _t(start, end, fully=0, direction=1, ref=0):
    return (R.TANDEM, ref, start, end, fully, direction, 0)


def _b(c1, p1, d1, c2, p2, d2):
    return (R.BND, c1, p1, d1, c2, p2, d2)


def _i(start, end, side, ref=0):
    return (R.INV, ref, start, end, side, 0, 0)


def postpass_cases(min_sv, max_sv):
    """[(name, raw records of one read)]."""
    out = []
    S, E = 10000, 10100
    # tandem merge (:261-290)
    for ds, de in ((19, 0), (20, 0), (21, 0), (0, 19), (0, 20), (0, 21), (-19, 0), (-20, 0), (-21, 0), (0, -19), (0, -20), (0, -21)):
        out.append(("tandem.second%+d%+d" % (ds, de), [_t(S, E), _t(S + ds, E + de)]))
    # counts 2 and 3 with a non-integer mean, on the start and on the end: 20 * count is where a scaled compare goes wrong
    for group in ([0, 1], [0, 2], [0, 1, 1], [0, 0, 2], [0, 2, 2]):
        for off in (-22, -21, -20, -19, -18, 19, 20, 21, 22, 23):
            out.append(("tandem.count%d.start%s%+d" % (len(group), group, off), [_t(S + g, E) for g in group] + [_t(S + off, E)]))
            out.append(("tandem.count%d.end%s%+d" % (len(group), group, off), [_t(S, E + g) for g in group] + [_t(S, E + off)]))
    out.append(("tandem.direction", [_t(S, E, direction=1), _t(S, E, direction=0)]))
    out.append(("tandem.contig", [_t(S, E, ref=3), _t(S, E, ref=4)]))
    # a split keeps the FIRST group's direction
    out.append(("tandem.stale_direction.joins", [_t(S, E, direction=1), _t(S + 500, E + 500, direction=0), _t(S + 500, E + 500, direction=1)]))
    out.append(("tandem.stale_direction.splits", [_t(S, E, direction=1), _t(S + 500, E + 500, direction=0), _t(S + 500, E + 500, direction=0)]))
    out.append(("tandem.stale_direction.rev", [_t(S, E, direction=0), _t(S + 500, E + 500, direction=1), _t(S + 501, E + 500, direction=0)]))
    out.append(("tandem.fully.second", [_t(S, E, fully=0), _t(S + 1, E, fully=1)]))
    out.append(("tandem.fully.third", [_t(S, E), _t(S + 1, E), _t(S + 1, E + 1, fully=1), _t(S + 900, E + 900)]))
    out.append(("tandem.fully.none", [_t(S, E), _t(S + 1, E)]))
    out.append(("tandem.truncate", [_t(S, E), _t(S + 1, E + 1), _t(S + 500, E), _t(S + 500, E), _t(S + 502, E + 1), _t(S + 900, E + 7)]))
    out.append(("tandem.single", [_t(S, E, fully=1, direction=0, ref=5)]))
    out.append(("tandem.between_others", [_i(100, 200, 0), _t(S, E), (R.INS, 0, 5, 55, 0, 50, 0), _t(S + 3, E - 3), (R.NONE, 0, 0, 0, 0, 0, 0)]))

    # breakend mirror (:293-320): b = before, t = this
    def fwd(length, near=0, **kw):
        b = dict(c1=0, p1=1000, d1=0, c2=1, p2=5000, d2=0)
        t = dict(c1=1, p1=5000 + length - 1, d1=0, c2=0, p2=1000 + near, d2=0)
        for k, v in kw.items():
            (b if k[0] == "b" else t)[k[2:]] = v
        return [_b(**b), _b(**t)]

    def rev(length, near=0, **kw):
        b = dict(c1=0, p1=1000, d1=1, c2=1, p2=5000, d2=1)
        t = dict(c1=1, p1=5000 + 1 - length, d1=1, c2=0, p2=1000 + near, d2=1)
        for k, v in kw.items():
            (b if k[0] == "b" else t)[k[2:]] = v
        return [_b(**b), _b(**t)]

    mid = (min_sv + max_sv) // 2
    for name, make in (("fwd", fwd), ("rev", rev)):
        for near in (-21, -20, -19, 0, 1, 2, 19, 20, 21):  # (0, 1, 2: odd and even sums under the halving)
            out.append(("mirror.%s.near%+d" % (name, near), make(mid, near)))
            out.append(("mirror.%s.odd_length.near%+d" % (name, near), make(mid + 1, near)))
        for length in (min_sv - 1, min_sv, min_sv + 1, max_sv - 1, max_sv, max_sv + 1):
            out.append(("mirror.%s.length%d" % (name, length), make(length)))
        other = 1 if name == "fwd" else 0
        out.append(("mirror.%s.dir1" % name, make(mid, t_d2=other)))
        out.append(("mirror.%s.dir2" % name, make(mid, t_d1=other)))
        out.append(("mirror.%s.chrom" % name, make(mid, t_c2=2)))
        out.append(("mirror.%s.origin" % name, make(mid, t_c1=2)))
        out.append(("mirror.%s.same_dir" % name, make(mid, b_d2=other, t_d1=other)))  # (t_d1 follows so that only :309 fails)
        two = make(mid)
        out.append(("mirror.%s.two_before" % name, [two[0], _b(0, 1005, two[0][3], 1, 5003, two[0][6]), two[1]]))
    out.append(("mirror.both", fwd(mid) + rev(mid + 3)))

    # inversions (:323-338, :42-60, :19-39); sides 0, 1 left, 2, 3 right
    out.append(("inv.one", [_i(100, 200, 0)]))
    out.append(("inv.two", [_i(100, 200, 0), _i(110, 210, 2)]))
    out.append(("inv.three", [_i(100, 200, 1), _i(110, 210, 3), _i(120, 190, 0)]))
    out.append(("inv.twelve", [_i(1000 + 3 * k, 1100 + 2 * k, (k * 3) % 4) for k in range(12)]))
    out.append(("inv.twelve.shuffled", [_i(1000 + 3 * k, 1100 + 2 * k, (k * 3) % 4) for k in (5, 0, 11, 3, 8, 1, 9, 2, 10, 4, 7, 6)]))
    for d in (-1, 0, 1):  # start - max(end): at 0 and +1 the group closes and the breakpoint is dropped
        out.append(("inv.overlap%+d" % d, [_i(100, 200, 0), _i(150, 180, 2), _i(200 + d, 300, 2), _i(250, 350, 0), _i(260, 340, 3)]))
    out.append(("inv.dropped_then_new", [_i(100, 200, 0), _i(200, 300, 2), _i(250, 350, 0), _i(260, 340, 2)]))
    out.append(("inv.dropped_last", [_i(100, 200, 0), _i(120, 220, 2), _i(220, 300, 2)]))
    out.append(("inv.contig_change", [_i(500, 600, 0, ref=0), _i(100, 200, 2, ref=4), _i(150, 250, 0, ref=4)]))
    out.append(("inv.contig_change.overlapping", [_i(500, 600, 0, ref=0), _i(510, 610, 2, ref=4)]))
    out.append(("inv.str_rank", [_i(100, 200, 0, ref=1), _i(110, 210, 2, ref=1), _i(100, 200, 0, ref=9), _i(120, 220, 2, ref=9)]))
    out.append(("inv.ratio.7/10", [_i(1000, 1010, 0), _i(1003, 1013, 2)]))      # 1 - 0.7 = 0.30000000000000004: apart
    out.append(("inv.ratio.70/100", [_i(1000, 1100, 1), _i(1030, 1130, 3)]))    # the same again
    out.append(("inv.ratio.3/4", [_i(1000, 1004, 0), _i(1001, 1005, 3)]))       # 0.25: joined
    out.append(("inv.ratio.inside", [_i(1000, 1100, 2), _i(1010, 1090, 0)]))    # overlap 80 of 100 and of 80: 0.2
    out.append(("inv.same_side", [_i(100, 200, 0), _i(110, 210, 1), _i(120, 220, 0), _i(130, 230, 1)]))
    for d in (-1, 0, 1):  # start2 - end1 of a pair inside one group
        out.append(("inv.apart%+d" % d, [_i(100, 300, 0), _i(150, 200, 0), _i(200 + d, 290, 2)]))
    out.append(("inv.same_start", [_i(100, 200, 0), _i(100, 201, 2), _i(101, 199, 3)]))
    out.append(("inv.unit_length", [_i(500, 600, 0), _i(500, 501, 2)]))
    out.append(("inv.unit_twins", [_i(500, 501, 0), _i(500, 501, 2)]))  # start1 - end2 = -1, the closest :28 gets to true
    out.append(("empty", []))
    out.append(("nothing_derived", [(R.INS, 0, 5, 55, 0, 50, 0), (R.DEL, 0, 5, 55, 0, 0, 0), (R.NONE, 0, 0, 0, 0, 0, 0)]))
    return out
