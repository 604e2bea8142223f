"""Plain restatement of the split-segment chain: the adjacent-pair decision tree of analyze_read_segments
(SVIM_inter.py:91-258) and its three post-passes (:260-338), branch for branch in the reference's nesting.

Every comparison goes through ONE helper and has a stable id (COMPARISONS below).  The helper can record
(id, outcome, lhs - rhs) into a trace, so that a table of cases can be shown to reach both sides of every
comparison and -1 | 0 | +1 around every threshold, and it can evaluate one comparison WRONGLY (a mutant), so that
the table can be shown to notice: tests/test_segments_restatement.py.  Records are in the svx_raw layout of
include/svx.h, (kind, a0..a5):
    INS     ref, start, end, read offset of the inserted bases, length, 0
    DEL     ref, start, end, 0, 0, 0
    BND     ref1, pos1, dir1, ref2, pos2, dir2          (dir: 0 fwd, 1 rev)
    TANDEM  ref, start, end, fully covered, direction (1 forward), 0
    INV     ref, start, end, side (0 left_fwd, 1 left_rev, 2 right_fwd, 3 right_rev), 0, 0
No numpy in here; the flat cut of the inversion groups' complete linkage is oracle/orc.linkage_cut (pinned to scipy by
tests/test_oracle_pins.py), handed the distances this module computes."""
import collections
import operator
from fractions import Fraction

NONE, INS, DEL, BND, TANDEM, INV = range(6)
FWD, REV = 0, 1
LEFT_FWD, LEFT_REV, RIGHT_FWD, RIGHT_REV = range(4)
PARAM_NAMES = ("min_sv_size", "max_sv_size", "query_gap_tolerance", "query_overlap_tolerance",
               "reference_gap_tolerance", "reference_overlap_tolerance")
TOLERANCES = PARAM_NAMES[2:]
Seg = collections.namedtuple("Seg", "q_start q_end ref_id ref_start ref_end is_reverse")
NONE_RECORD = (NONE, 0, 0, 0, 0, 0, 0)

_OPS = {">=": operator.ge, ">": operator.gt, "<=": operator.le, "<": operator.lt, "==": operator.eq}
_FLIP = {">=": ">", ">": ">=", "<=": "<", "<": "<="}
_SWAP = {"min_sv_size": "max_sv_size", "max_sv_size": "min_sv_size"}


def _table(text):
    """id: lhs op rhs.  rhs is a parameter (with its sign), the constant 20, or a value of the input."""
    out = collections.OrderedDict()
    for line in text.strip().splitlines():
        cid, expr = [s.strip() for s in line.split(":", 1)]
        lhs, op, rhs = expr.rsplit(None, 2)
        sign = -1 if rhs.startswith("-") else 1
        name = rhs.lstrip("-")
        out[cid] = (op, sign, name if name in PARAM_NAMES else None, int(name) if name.isdigit() else None)
    return out


# ---- the decision tree, SVIM_inter.py:91-258 (line numbers in the ids' comments)
COMPARISONS = _table("""
chrom:                 cur.ref_id == nxt.ref_id
same.strand:           cur.is_reverse == nxt.is_reverse
same.dref_rev:         cur.is_reverse == True
same.read_overlap:     distance_on_read >= -query_overlap_tolerance
same.ref_overlap:      distance_on_reference >= -reference_overlap_tolerance
same.ins.min:          deviation >= min_sv_size
same.ins.ref_gap:      distance_on_reference <= reference_gap_tolerance
same.ins.fwd:          cur.is_reverse == False
same.del.lo:           deviation >= -max_sv_size
same.del.hi:           deviation <= -min_sv_size
same.del.read_gap:     distance_on_read <= query_gap_tolerance
same.del.fwd:          cur.is_reverse == False
same.bnd.max:          deviation < -max_sv_size
same.bnd.read_gap:     distance_on_read <= query_gap_tolerance
same.bnd.fwd:          cur.is_reverse == False
same.dup.read_gap:     distance_on_read <= query_gap_tolerance
same.dup.min:          deviation >= min_sv_size
same.dup.fwd:          cur.is_reverse == False
same.dup_fwd.full:     nxt.ref_end > cur.ref_start
same.dup_fwd.max:      distance_on_reference >= -max_sv_size
same.dup_rev.full:     nxt.ref_start < cur.ref_end
same.dup_rev.max:      distance_on_reference >= -max_sv_size
inv.fr:                cur.is_reverse == False
fr.read_overlap:       distance_on_read >= -query_overlap_tolerance
fr.read_gap:           distance_on_read <= query_gap_tolerance
fr.case1:              nxt.ref_start-cur.ref_end >= -reference_overlap_tolerance
fr.case1.min:          -deviation >= min_sv_size
fr.case1.max:          -deviation <= max_sv_size
fr.case3:              cur.ref_start-nxt.ref_end >= -reference_overlap_tolerance
fr.case3.min:          deviation >= min_sv_size
fr.case3.max:          deviation <= max_sv_size
inv.rf:                cur.is_reverse == True
rf.read_overlap:       distance_on_read >= -query_overlap_tolerance
rf.read_gap:           distance_on_read <= query_gap_tolerance
rf.case2:              nxt.ref_start-cur.ref_end >= -reference_overlap_tolerance
rf.case2.min:          -deviation >= min_sv_size
rf.case2.max:          -deviation <= max_sv_size
rf.case4:              cur.ref_start-nxt.ref_end >= -reference_overlap_tolerance
rf.case4.min:          deviation >= min_sv_size
rf.case4.max:          deviation <= max_sv_size
other.strand:          cur.is_reverse == nxt.is_reverse
other.same.read_overlap: distance_on_read >= -query_overlap_tolerance
other.same.read_gap:   distance_on_read <= query_gap_tolerance
other.same.fwd:        cur.is_reverse == False
other.diff.read_overlap: distance_on_read >= -query_overlap_tolerance
other.diff.read_gap:   distance_on_read <= query_gap_tolerance
other.diff.fwd:        cur.is_reverse == False
""")
TREE_IDS = tuple(COMPARISONS)

# ---- the post-passes, SVIM_inter.py:260-338 and :12-39
COMPARISONS.update(_table("""
tandem.open:           current_chromosome == None
tandem.chrom:          current_chromosome == chromosome
tandem.start:          abs(mean(current_starts)-start) < 20
tandem.end:            abs(mean(current_ends)-end) < 20
tandem.direction:      current_direction == direction
mirror.dir1:           before_dir1 == this_dir2
mirror.dir2:           before_dir2 == this_dir1
mirror.chrom:          before_chr1 == this_chr2
mirror.near:           abs(before_pos1-this_pos2) < 20
mirror.origin:         before_chr2 == this_chr1
mirror.same_dir:       before_dir2 == before_dir1
mirror.fwd:            before_dir1 == fwd
mirror.fwd.min:        length >= min_sv_size
mirror.fwd.max:        length <= max_sv_size
mirror.rev.min:        length >= min_sv_size
mirror.rev.max:        length <= max_sv_size
inv.open:              len(active_inversions) == 0
inv.chrom:             chrom == active_inversions[-1].chrom
inv.overlap:           start < max(end)
inv.single:            len(active_inversions) < 2
dist.same_side:        direction1 == direction2
dist.apart1:           start2 >= end1
dist.apart2:           start1 >= end2
dist.left:             start2 >= start1
"""))
POST_IDS = tuple(c for c in COMPARISONS if c not in TREE_IDS)
# not routed, because they are no comparison of the input: `abs(0 - 0) < 20` of the mirror's is_similar (:305, both
# ends are the constant 0), `elif before_dir1 == 'rev'` (:314, the negation of mirror.fwd), `sum(current_fully_covered)`
# (:281, a truth value) and the 0.3 of fcluster (:48, inside scipy: a double compare that orc.linkage_cut restates).


def mutants_of(cid):
    """Every wrong evaluation of comparison `cid`: (cid, how)."""
    op, _, name, _ = COMPARISONS[cid]
    out = []
    if op in _FLIP:
        out.append((cid, "flip_strict"))
    if name in TOLERANCES:
        out += [(cid, "other_tolerance:" + t) for t in TOLERANCES if t != name]
    if name in _SWAP:
        out.append((cid, "min_max"))
    return out


class _Compare(object):
    """test(cid, lhs[, rhs]): the one place where the restatement compares."""

    def __init__(self, params, trace, mutant):
        self.p = dict(zip(PARAM_NAMES, (int(v) for v in params)))
        self.trace, self.mutant, self.leaf = trace, mutant, None

    def __call__(self, cid, lhs, rhs=None):
        op, sign, name, const = COMPARISONS[cid]
        how = self.mutant[1] if self.mutant is not None and self.mutant[0] == cid else None
        used = name
        if how is not None:
            assert (cid, how) in mutants_of(cid), (cid, how)
            if how == "flip_strict":
                op = _FLIP[op]
            elif how == "min_max":
                used = _SWAP[name]
            else:
                used = how.split(":", 1)[1]
        if name is not None:
            assert rhs is None
            rhs, rhs_used = sign * self.p[name], sign * self.p[used]
        else:
            rhs = const if const is not None else rhs
            rhs_used = rhs
        outcome = _OPS[op](lhs, rhs_used)
        if self.trace is not None:
            self.trace.append((cid, bool(outcome), (lhs - rhs) if op != "==" else int(lhs != rhs)))
        return outcome


def _bnd(ref1, pos1, dir1, ref2, pos2, dir2):
    return (BND, ref1, pos1, dir1, ref2, pos2, dir2)


def classify_pair(cur, nxt, read_len, params, trace=None, mutant=None, leaf=None):
    """The record of one adjacent pair of the sorted segments (:91-258).  `leaf`: a list that receives the name of the
    leaf reached."""
    test = _Compare(params, trace, mutant)
    rec, name = _classify(test, cur, nxt, read_len)
    if leaf is not None:
        leaf.append(name)
    return rec


def _classify(test, cur, nxt, read_len):
    distance_on_read = nxt.q_start - cur.q_end                                                            # :95
    if test("chrom", cur.ref_id, nxt.ref_id):                                                             # :98
        ref_chr = cur.ref_id
        if test("same.strand", cur.is_reverse, nxt.is_reverse):                                           # :101
            if test("same.dref_rev", cur.is_reverse, True):                                               # :103
                distance_on_reference = cur.ref_start - nxt.ref_end
            else:
                distance_on_reference = nxt.ref_start - cur.ref_end
            if test("same.read_overlap", distance_on_read):                                               # :108
                if test("same.ref_overlap", distance_on_reference):                                       # :110
                    deviation = distance_on_read - distance_on_reference
                    if test("same.ins.min", deviation):                                                   # :113
                        if test("same.ins.ref_gap", distance_on_reference):                               # :115
                            if test("same.ins.fwd", cur.is_reverse, False):                               # :116
                                return (INS, ref_chr, cur.ref_end, cur.ref_end + deviation, cur.q_end, deviation, 0), "ins.fwd"
                            else:                                                                         # :120
                                return (INS, ref_chr, cur.ref_start, cur.ref_start + deviation,
                                        read_len - nxt.q_start, deviation, 0), "ins.rev"
                    elif test("same.del.lo", deviation) and test("same.del.hi", deviation):               # :123
                        if test("same.del.read_gap", distance_on_read):                                   # :125
                            if test("same.del.fwd", cur.is_reverse, False):
                                return (DEL, ref_chr, cur.ref_end, cur.ref_end - deviation, 0, 0, 0), "del.fwd"
                            else:
                                return (DEL, ref_chr, nxt.ref_end, nxt.ref_end - deviation, 0, 0, 0), "del.rev"
                    elif test("same.bnd.max", deviation):                                                 # :131
                        if test("same.bnd.read_gap", distance_on_read):                                   # :133
                            if test("same.bnd.fwd", cur.is_reverse, False):
                                return _bnd(ref_chr, cur.ref_end - 1, FWD, ref_chr, nxt.ref_start, FWD), "bnd.fwd"
                            else:
                                return _bnd(ref_chr, cur.ref_start, REV, ref_chr, nxt.ref_end - 1, REV), "bnd.rev"
                else:                                                                                     # :141
                    if test("same.dup.read_gap", distance_on_read):                                       # :143
                        deviation = distance_on_read - distance_on_reference
                        if test("same.dup.min", deviation):                                               # :146
                            if test("same.dup.fwd", cur.is_reverse, False):                               # :147
                                if test("same.dup_fwd.full", nxt.ref_end, cur.ref_start):                 # :149
                                    return (TANDEM, ref_chr, nxt.ref_start, nxt.ref_start + deviation, 1, 1, 0), "dup_full.fwd"
                                elif test("same.dup_fwd.max", distance_on_reference):                     # :152
                                    return (TANDEM, ref_chr, nxt.ref_start, nxt.ref_start + deviation, 0, 1, 0), "dup_part.fwd"
                                else:                                                                     # :155
                                    return _bnd(ref_chr, cur.ref_end - 1, FWD, ref_chr, nxt.ref_start, FWD), "dup_bnd.fwd"
                            else:
                                if test("same.dup_rev.full", nxt.ref_start, cur.ref_end):                 # :160
                                    return (TANDEM, ref_chr, cur.ref_start, cur.ref_start + deviation, 1, 0, 0), "dup_full.rev"
                                elif test("same.dup_rev.max", distance_on_reference):                     # :163
                                    return (TANDEM, ref_chr, cur.ref_start, cur.ref_start + deviation, 0, 0, 0), "dup_part.rev"
                                else:                                                                     # :166
                                    return _bnd(ref_chr, cur.ref_start, REV, ref_chr, nxt.ref_end - 1, REV), "dup_bnd.rev"
        else:                                                                                             # :170
            # :172 is `not cur.is_reverse and nxt.is_reverse`, :198 its mirror image; the strands differ here, so the
            # second operand repeats the first
            if test("inv.fr", cur.is_reverse, False):                                                     # :172
                distance_on_reference = nxt.ref_end - cur.ref_end
                deviation = distance_on_read - distance_on_reference
                if test("fr.read_overlap", distance_on_read) and test("fr.read_gap", distance_on_read):   # :175
                    if test("fr.case1", nxt.ref_start - cur.ref_end):                                     # :176
                        if test("fr.case1.min", -deviation) and test("fr.case1.max", -deviation):         # :178
                            return (INV, ref_chr, cur.ref_end, cur.ref_end - deviation, LEFT_FWD, 0, 0), "inv1"
                        else:
                            return _bnd(ref_chr, cur.ref_end - 1, FWD, ref_chr, nxt.ref_end - 1, REV), "inv1_bnd"
                    elif test("fr.case3", cur.ref_start - nxt.ref_end):                                   # :185
                        if test("fr.case3.min", deviation) and test("fr.case3.max", deviation):           # :187
                            return (INV, ref_chr, nxt.ref_end, nxt.ref_end + deviation, LEFT_REV, 0, 0), "inv3"
                        else:
                            return _bnd(ref_chr, cur.ref_end - 1, FWD, ref_chr, nxt.ref_end - 1, REV), "inv3_bnd"
            if test("inv.rf", cur.is_reverse, True):                                                      # :198
                distance_on_reference = nxt.ref_start - cur.ref_start
                deviation = distance_on_read - distance_on_reference
                if test("rf.read_overlap", distance_on_read) and test("rf.read_gap", distance_on_read):   # :201
                    if test("rf.case2", nxt.ref_start - cur.ref_end):                                     # :202
                        if test("rf.case2.min", -deviation) and test("rf.case2.max", -deviation):         # :204
                            return (INV, ref_chr, cur.ref_start, cur.ref_start - deviation, RIGHT_FWD, 0, 0), "inv2"
                        else:
                            return _bnd(ref_chr, cur.ref_start, REV, ref_chr, nxt.ref_start, FWD), "inv2_bnd"
                    elif test("rf.case4", cur.ref_start - nxt.ref_end):                                   # :211
                        if test("rf.case4.min", deviation) and test("rf.case4.max", deviation):           # :213
                            return (INV, ref_chr, nxt.ref_start, nxt.ref_start + deviation, RIGHT_REV, 0, 0), "inv4"
                        else:
                            return _bnd(ref_chr, cur.ref_start, REV, ref_chr, nxt.ref_start, FWD), "inv4_bnd"
    else:                                                                                                 # :224
        c1, c2 = cur.ref_id, nxt.ref_id
        if test("other.strand", cur.is_reverse, nxt.is_reverse):                                          # :228
            if test("other.same.read_overlap", distance_on_read):                                         # :230
                if test("other.same.read_gap", distance_on_read):                                         # :232
                    if test("other.same.fwd", cur.is_reverse, False):
                        return _bnd(c1, cur.ref_end - 1, FWD, c2, nxt.ref_start, FWD), "other.ff"
                    else:
                        return _bnd(c1, cur.ref_start, REV, c2, nxt.ref_end - 1, REV), "other.rr"
        else:
            if test("other.diff.read_overlap", distance_on_read):                                         # :246
                if test("other.diff.read_gap", distance_on_read):                                         # :248
                    if test("other.diff.fwd", cur.is_reverse, False):
                        return _bnd(c1, cur.ref_end - 1, FWD, c2, nxt.ref_end - 1, REV), "other.fr"
                    else:
                        return _bnd(c1, cur.ref_start, REV, c2, nxt.ref_start, FWD), "other.rf"
    return NONE_RECORD, "none"


def sort_segments(segs):
    """:83 — sorted() is stable: ties of (q_start, q_end) keep the input order."""
    return sorted(segs, key=lambda aln: (aln.q_start, aln.q_end))


def classify_read(segs, read_len, params, trace=None, mutant=None, leaves=None):
    """One record per segment slot, as svx_segments_classify writes them: pair i of the sorted segments in slot i, NONE
    in the last slot."""
    s = sort_segments(segs)
    out = [classify_pair(a, b, read_len, params, trace, mutant, leaves) for a, b in zip(s, s[1:])]
    return out + [NONE_RECORD] * (1 if s else 0)


# ------------------------------------------------------------------------------------------ post-passes
def _mean(xs):
    return Fraction(sum(xs), len(xs))  # statistics.mean of ints is the exact rational


def _distance(test, inversion1, inversion2):
    """reciprocal_overlap_distance, :19-39."""
    start1, end1, direction1 = inversion1
    start2, end2, direction2 = inversion2
    if test("dist.same_side", direction1, direction2):
        return 1
    if test("dist.apart1", start2, end1):
        return 1
    if test("dist.apart2", start1, end2):
        return 1
    if test("dist.left", start2, start1):
        overlap = min(end1, end2) - start2
    else:
        overlap = min(end1, end2) - start1
    return 1 - min(overlap / float(end1 - start1), overlap / float(end2 - start2))


def _flat_clusters(dist, n):
    from oracle import orc
    return [int(x) for x in orc.linkage_cut(dist, n, 0.3)]


def postpass_read(raw, contig_rank, min_sv, max_sv, trace=None, mutant=None):
    """The derived records of one read from its raw records (kind, a0..a5), in the reference's order: what
    oracle/svim_oracle.postpass_records returns."""
    test = _Compare((min_sv, max_sv, 0, 0, 0, 0), trace, mutant)
    out = []
    tandem_duplications = [(r[1], r[2], r[3], bool(r[4]), bool(r[5])) for r in raw if r[0] == TANDEM]
    translocations = [(r[3], r[6], r[1], r[2], r[4], r[5]) for r in raw if r[0] == BND]
    inversions = [(r[1], r[2], r[3], r[4]) for r in raw if r[0] == INV]

    current_chromosome = None                                                                             # :261
    for td in tandem_duplications:
        if test("tandem.open", current_chromosome is None, True):                                         # :267
            current_chromosome, current_starts, current_ends, current_copy_number = td[0], [td[1]], [td[2]], 1
            current_fully_covered, current_direction = [td[3]], td[4]
        else:                                                                                             # :275, :13
            if (test("tandem.chrom", current_chromosome, td[0]) and test("tandem.start", abs(_mean(current_starts) - td[1]))
                    and test("tandem.end", abs(_mean(current_ends) - td[2]))
                    and test("tandem.direction", current_direction, td[4])):
                current_starts.append(td[1]); current_ends.append(td[2])
                current_copy_number += 1
                current_fully_covered.append(td[3])
            else:
                out.append(("TANDEM", current_chromosome, int(_mean(current_starts)), int(_mean(current_ends)),
                            current_copy_number, bool(sum(current_fully_covered))))
                # :283-287: current_direction is NOT set again
                current_chromosome, current_starts, current_ends, current_copy_number = td[0], [td[1]], [td[2]], 1
                current_fully_covered = [td[3]]
    if current_chromosome is not None:                                                                    # :288
        out.append(("TANDEM", current_chromosome, int(_mean(current_starts)), int(_mean(current_ends)),
                    current_copy_number, bool(sum(current_fully_covered))))

    for this_index in range(len(translocations)):                                                         # :293
        this_dir1, this_dir2, this_chr1, this_pos1, this_chr2, this_pos2 = translocations[this_index]
        for before_dir1, before_dir2, before_chr1, before_pos1, before_chr2, before_pos2 in translocations[:this_index]:
            if test("mirror.dir1", before_dir1, this_dir2) and test("mirror.dir2", before_dir2, this_dir1):   # :303
                if test("mirror.chrom", before_chr1, this_chr2) and test("mirror.near", abs(before_pos1 - this_pos2)):  # :305
                    if test("mirror.origin", before_chr2, this_chr1):                                     # :307
                        if test("mirror.same_dir", before_dir2, before_dir1):                             # :309
                            if test("mirror.fwd", before_dir1, FWD):                                      # :310
                                length = this_pos1 + 1 - before_pos2
                                if test("mirror.fwd.min", length) and test("mirror.fwd.max", length):     # :312
                                    m = int(_mean([before_pos1 + 1, this_pos2]))
                                    out.append(("DUP_INT", before_chr2, before_pos2, this_pos1 + 1, before_chr1, m, m + length))
                            else:                                                                         # :314
                                length = before_pos2 + 1 - this_pos1
                                if test("mirror.rev.min", length) and test("mirror.rev.max", length):     # :316
                                    m = int(_mean([before_pos1, this_pos2 + 1]))
                                    out.append(("DUP_INT", before_chr2, this_pos1, before_pos2 + 1, before_chr1, m, m + length))

    def process_overlapping_inversions(active):                                                           # :42-60
        if test("inv.single", len(active)):
            clusters = [active]
        else:
            data = [(i[1], i[2], 0 if i[3] < 2 else 1) for i in active]                                   # :46 left / right
            dist = [_distance(test, data[i], data[j]) for i in range(len(data) - 1) for j in range(i + 1, len(data))]
            labels = _flat_clusters(dist, len(data))
            clusters = [[] for _ in range(max(labels))]
            for index, label in enumerate(labels):
                clusters[label - 1].append(active[index])
        for cluster in clusters:
            out.append(("INV", cluster[0][0], max(i[1] for i in cluster), min(i[2] for i in cluster), len(cluster) > 1))

    # :323 sorts by the contig NAME; contig_rank[ref_id] is that name's rank
    active = []
    for inversion in sorted(inversions, key=lambda i: (contig_rank[i[0]], i[1], i[2])):
        if test("inv.open", len(active), 0):                                                              # :327
            active.append(inversion)
        else:
            if test("inv.chrom", inversion[0], active[-1][0]) and test("inv.overlap", inversion[1], max(i[2] for i in active)):  # :331
                active.append(inversion)
            else:
                process_overlapping_inversions(active)
                active = []                                                                               # :336 drops `inversion`
    if len(active) > 0:
        process_overlapping_inversions(active)
    return out
