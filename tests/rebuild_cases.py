"""Truth by construction for the small-variant commands: small genomes, haplotypes given as edit
scripts, and the alignments those scripts spell.  tests/test_small_rebuild_host.py (no GPU) and
tests/test_gpu_small_rebuild.py run `svim-asm-small` and `svim-asm-small-compare` on them and hold the answer to ONE
property that needs no restatement of the commands: over every stretch of the reference that a haplotype covers exactly
once, the reference with that haplotype's called records applied IS the assembled contig (tests/rebuild_judge.py).

Pure Python.  Nothing of the product is imported but four constants, read through `_lib`: the seams the named cases are
built around.  A case holds
  genome, order     {contig: bases, mixed case, a few N}; the contigs' order in the FASTA and the headers (not alphabetical)
  haps              per haplotype a list of Aln: (contig, start, ops, SEQ) — the tuple shape of tests/small_restatement.py —
                    plus flag, MAPQ, whether SEQ is stored, whether the file holds it in lower case, and a name
  edits             what the generator KNOWS: every truth edit (haplotype, alignment, contig, pos, ref_len, bases, kind) with
                    the cursors (r, q) and the most steps it may move (`limit`: up to the column behind the gap in front)
  expect            what the case's name promises, asserted on the case's own arrays when it is built (`shows`)
and the functions below say, from the truth alone, which records COLLECT must not visit (`status`), where a small gap
lies with --left_align (`left_shift`, `placed`: suffix runs of the two strings, not the product's loop) and which edits
are dropped for a reason the truth can see (`reason`: no_anchor, ambiguous_base; multiply_covered needs the depth of
tests/rebuild_judge.py)."""
import collections
import functools
import random

from svim_asm_amd import _lib
from tests import sam_text_writer as stw, spec_bam_writer as sbw

T = _lib.MISMATCH_TILE          # reference positions per workgroup of svx_cigar_mismatch, 16 per lane
LC = _lib.LIFT_CHUNK            # ops per workgroup of the prefix scan
W = _lib.SHIFT_WAVE_COLS        # steps per iteration of svx_indel_shift's wave form
LS = _lib.SHIFT_LANE_STEPS      # steps of its lane form before the hand-over
LANE = 16
ACGT = "ACGT"
ORDER = ("ctgM", "ctgA", "ctgZ")
SEEDS = (1, 2, 3, 4, 5, 6)
REF_OPS, QRY_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)

Aln = collections.namedtuple("Aln", "contig start ops seq flag mapq stored lower name")
Edit = collections.namedtuple("Edit", "hap aln contig pos ref_len bases kind r q limit")
Case = collections.namedtuple("Case", "name genome order haps edits min_sv_size min_mapq expect")


def other(base):
    return {"A": "C", "C": "G", "G": "T", "T": "A"}[base.upper()]


def ref_length(ops):
    return sum(n for op, n in ops if op in REF_OPS)


class Script(object):
    """An alignment as a list of (op, length or bases) with the reference cursor kept, so that a case can say where its
    SNVs lie relative to what it has just written: M(n, snv=[columns inside this run])."""

    def __init__(self):
        self.items, self.r, self.snv = [], 0, []

    def M(self, n, snv=()):
        assert n > 0
        self.snv += [self.r + c for c in snv if 0 <= c < n]
        if self.items and self.items[-1][0] == "M":
            self.items[-1] = ("M", self.items[-1][1] + n)
        else:
            self.items.append(("M", n))
        self.r += n
        return self

    def I(self, bases):
        self.items.append(("I", bases))
        return self

    def D(self, n):
        self.items.append(("D", n))
        self.r += n
        return self

    def S(self, bases):
        self.items.append(("S", bases))
        return self

    def H(self, n):
        self.items.append(("H", n))
        return self

    def N(self, n):
        self.items.append(("N", n))
        self.r += n
        return self


class Builder(object):
    def __init__(self, name, min_sv_size=40, random_n=0):
        self.name, self.min_sv_size = name, min_sv_size
        self.rng = rng = random.Random("rebuild " + name)
        self.ref = {}
        for c in ORDER:
            seq = [rng.choice(ACGT) for _ in range(rng.randrange(30000, 50001))]
            p = 0
            while p < len(seq):  # lower-case stretches: soft-masked repeats
                n = rng.randrange(200, 2000)
                if rng.random() < 0.3:
                    seq[p:p + n] = [b.lower() for b in seq[p:p + n]]
                p += n
            for k in range(4 + random_n):  # a few N: four at the contig's far end, `random_n` anywhere
                at = len(seq) - 10 + k if k < 4 else rng.randrange(200, len(seq) - 200)
                seq[at] = "Nn"[k % 2]
            self.ref[c] = seq
        self.haps, self.edits, self.spelled, self.expect = [[], []], [], [], {}

    def bases(self, n):
        return "".join(self.rng.choice(ACGT) for _ in range(n))

    def base(self, contig, p):
        return self.ref[contig][p].upper()

    def plant(self, contig, pos, text):
        """Overwrite the reference — only where nothing has been spelled yet."""
        assert 0 <= pos and pos + len(text) <= len(self.ref[contig])
        assert not any(c == contig and lo < pos + len(text) and pos < hi for c, lo, hi in self.spelled), "planted under an alignment"
        self.ref[contig][pos:pos + len(text)] = list(text)
        return pos

    def plant_run(self, contig, pos, unit, copies):
        """`copies` of `unit` from pos on, the bases around them chosen so that the run neither grows nor lets a gap of
        one unit move out of it."""
        run = unit * copies
        self.plant(contig, pos - 1, other(unit[-1]) if other(unit[-1]) != unit[0] else other(other(unit[-1])))
        self.plant(contig, pos, run)
        self.plant(contig, pos + len(run), other(unit[0]) if other(unit[0]) != unit[-1] else other(other(unit[0])))
        assert self.base(contig, pos - 1) not in (unit[-1], unit[0]) and self.base(contig, pos + len(run)) not in (unit[0], unit[-1])
        return pos, pos + len(run)

    def align(self, hap, contig, start, script, flag=0, mapq=60, stored=True, lower=False, name=None, snv_to=None):
        """Spell one alignment and note every edit it holds.  `snv_to`: {reference position: base} for columns whose SNV
        base the case chooses itself."""
        ref, index = self.ref[contig], len(self.haps[hap])
        snv = {start + o: None for o in script.snv}
        snv.update(snv_to or {})
        ops, seq, r, q, prev_end = [], [], 0, 0, 0
        for op, arg in script.items:
            if op == "M":
                for p in range(start + r, start + r + arg):
                    R = ref[p].upper()
                    if p in snv:
                        b = snv.pop(p) or other(R)
                        assert R in ACGT and b in ACGT and b != R, "an SNV needs two different bases of ACGT"
                        self.edits.append(Edit(hap, index, contig, p, 1, b, "SNV", p - start, q + p - start - r, 0))
                        seq.append(b)
                    else:
                        seq.append(R)  # (N under N: the contig was assembled from it)
                ops.append((0, arg))
                r, q = r + arg, q + arg
            elif op == "I":
                self.edits.append(Edit(hap, index, contig, start + r, 0, arg.upper(), "INS", r, q, max(0, r - prev_end - 1)))
                ops.append((1, len(arg)))
                seq.append(arg.upper())
                prev_end, q = r, q + len(arg)
            elif op == "D":
                self.edits.append(Edit(hap, index, contig, start + r, arg, "", "DEL", r, q, max(0, r - prev_end - 1)))
                ops.append((2, arg))
                prev_end = r = r + arg
            elif op == "S":
                ops.append((4, len(arg)))
                seq.append(arg.upper())
                q += len(arg)
            elif op == "H":
                ops.append((5, arg))
            else:
                assert op == "N"
                ops.append((3, arg))
                r += arg
        assert not snv, "an SNV outside the aligned columns"
        assert start + r <= len(ref)
        self.spelled.append((contig, start, start + r))
        self.haps[hap].append(Aln(contig, start, ops, "".join(seq), flag, mapq, stored, lower, name or "h%d_%03d" % (hap + 1, index)))
        return index

    def case(self):
        genome = {c: "".join(s) for c, s in self.ref.items()}
        return Case(self.name, genome, ORDER, [list(h) for h in self.haps], list(self.edits), self.min_sv_size, 20, dict(self.expect))


# ------------------------------------------------------------------------------------------------ what the truth knows
def status(case, a):
    """not_visited (unmapped, secondary, MAPQ below --min_mapq), no_sequence, spliced, or used — in COLLECT's order."""
    if a.flag & 4 or a.flag & 256 or a.mapq < case.min_mapq:
        return "not_visited"
    if not a.stored:
        return "no_sequence"
    if any(op == 3 for op, _ in a.ops):
        return "spliced"
    return "used"


def size(e):
    return e.ref_len if e.kind == "DEL" else len(e.bases)


def is_small_gap(case, e):
    return e.kind != "SNV" and size(e) < case.min_sv_size


def _suffix_run(a, ia, b, ib, cap, letters=False):
    """How many bases in front of a[ia] and b[ib] agree, walking down, at most cap."""
    j = 0
    while j < cap and ia - 1 - j >= 0 and ib - 1 - j >= 0 and a[ia - 1 - j] == b[ib - 1 - j] and (not letters or a[ia - 1 - j] in ACGT):
        j += 1
    return j


def left_shift(case, e):
    """The columns a small gap moves with --left_align: as many as (1) the aligned columns in front of it are matches of
    one ACGT base and (2) the string that holds the gap's bases repeats itself at the gap's length, never more than the
    limit (one aligned column stays between it and the gap or the start in front)."""
    if not is_small_gap(case, e):
        return 0
    a = case.haps[e.hap][e.aln]
    ref, seq, n = case.genome[e.contig].upper(), a.seq.upper(), size(e)
    cap = min(e.limit, e.r, e.q)
    matches = _suffix_run(ref, e.pos, seq, e.q, cap, letters=True)
    repeats = _suffix_run(ref, e.pos, ref, e.pos + n, cap) if e.kind == "DEL" else _suffix_run(seq, e.q, seq, e.q + n, cap)
    return min(matches, repeats)


def placed(case, e, left_align):
    """(pos, ref_len, bases) of an edit as the command reports it."""
    k = left_shift(case, e) if left_align else 0
    if k == 0:
        return e.pos, e.ref_len, e.bases
    if e.kind == "DEL":
        return e.pos - k, e.ref_len, ""
    seq = case.haps[e.hap][e.aln].seq.upper()
    return e.pos - k, 0, seq[e.q - k:e.q - k + len(e.bases)]


def reason(case, e, left_align):
    """Why the command leaves a truth edit out, as far as the truth alone can tell: `large` (svim-asm's), `no_anchor`,
    `ambiguous_base`, or None (kept unless its span is not singly covered)."""
    if e.kind == "SNV":
        return None
    if not is_small_gap(case, e):
        return "large"
    if e.r == 0:
        return "no_anchor"
    pos, ref_len, bases = placed(case, e, left_align)
    ref = case.genome[e.contig].upper()
    if set(ref[pos - 1:pos + ref_len] + bases) - set(ACGT):
        return "ambiguous_base"
    return None


def span(kind, pos, ref_len):
    """The REF span of a record: the anchor in front of a gap belongs to it."""
    return (pos, pos + 1) if kind == "SNV" else (pos - 1, pos + ref_len)


def edits_of(case, hap, aln=None):
    return [e for e in case.edits if e.hap == hap and (aln is None or e.aln == aln)]


# ------------------------------------------------------------------------------------------------ the files
def write_fasta(path, case, line=70):
    with open(path, "w") as fh, open(path + ".fai", "w") as fai:
        for c in case.order:
            seq = case.genome[c]
            fh.write(">%s\n" % c)
            off = fh.tell()
            for p in range(0, len(seq), line):
                fh.write(seq[p:p + line] + "\n")
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (c, len(seq), off, line, line + 1))
    return path


def write_sam(path, case, hap, shuffle_seed):
    lines = []
    for a in case.haps[hap]:
        seq = (a.seq.lower() if a.lower else a.seq) if a.stored else None
        lines.append(stw.record_line(a.name, a.flag, a.contig, a.start, a.mapq, stw.cigar_string([(n << 4) | op for op, n in a.ops]), seq))
    return stw.write_sam(path, list(case.order), [len(case.genome[c]) for c in case.order], lines, shuffle_seed=shuffle_seed)


def write_bam(path, case, hap):
    alns = sorted(case.haps[hap], key=lambda a: (case.order.index(a.contig), a.start))  # (stable: coordinate-sorted, indexed)
    records = [dict(name=a.name, flag=a.flag, tid=case.order.index(a.contig), pos=a.start, mapq=a.mapq, cigar=list(a.ops),
                    seq=a.seq if a.stored else "") for a in alns]
    sbw.write_bam(path, [(c, len(case.genome[c])) for c in case.order], records, chunk=20000)
    return path


# ------------------------------------------------------------------------------------------------ the named cases
def _columns(case, hap, aln, kind):
    return [e.r for e in edits_of(case, hap, aln) if e.kind == kind]


def tile_columns():
    """One M window of 2T + 5 reference positions per alignment; SNVs in the first and last column of a lane, a tile and the
    window; a D that ends at column T - 1, one that starts at T, an I between T - 1 and T."""
    b = Builder("tile-columns")
    span_, start = 2 * T + 5, 1003
    cols = [0, LANE - 1, LANE, T - 1, T, T + 1, 2 * T - 1, 2 * T, span_ - 1]
    c0, c1 = ORDER[0], ORDER[1]
    b.align(0, c0, start, Script().M(span_, snv=cols))
    b.align(1, c0, start, Script().M(T - 3).D(3).M(span_ - T, snv=[0, 7]))
    b.align(0, c1, start + 5, Script().M(T, snv=[T - 1]).D(3).M(span_ - T - 3))
    b.align(1, c1, start + 5, Script().M(T).I("GAT").M(span_ - T, snv=[0]))
    case = b.case()
    assert all(ref_length(a.ops) == span_ for h in case.haps for a in h)
    assert _columns(case, 0, 0, "SNV") == cols and cols[-1] == 2 * T + 4
    (d1,), (d2,), (i1,) = edits_of(case, 1, 0)[:1], [e for e in edits_of(case, 0, 1) if e.kind == "DEL"], [e for e in edits_of(case, 1, 1) if e.kind == "INS"]
    assert d1.kind == "DEL" and d1.r + d1.ref_len - 1 == T - 1 and d2.r == T and i1.r == T
    return case


def op_per_column():
    """Alignments of LC + 1 and 2 LC + 1 ops: a long M up to shortly before the tile border, then `1I1M` / `1D1M` pairs
    across it; every other one-column M mismatches."""
    b = Builder("op-per-column")

    def pairs(lead, n_ops, gap):
        s = Script().M(lead)
        for j in range((n_ops - 1) // 2):
            s = s.I(b.rng.choice(ACGT)) if gap == "I" else s.D(1)
            s.M(1, snv=[0] if j % 2 == 0 else [])
        return s

    plan = [(0, ORDER[0], 2001, T - 200, LC + 1, "I"), (1, ORDER[0], 2001, T - 500, 2 * LC + 1, "D"),
            (0, ORDER[1], 777, T - 700, 2 * LC + 1, "I"), (1, ORDER[1], 777, T - 300, LC + 1, "D")]
    for hap, contig, start, lead, n_ops, gap in plan:
        b.align(hap, contig, start, pairs(lead, n_ops, gap))
    case = b.case()
    for hap, contig, start, lead, n_ops, gap in plan:
        (a,) = [x for x in case.haps[hap] if x.contig == contig]
        assert len(a.ops) == n_ops and lead < T < ref_length(a.ops) and all(n == 1 for _, n in a.ops[1:])
        single = (n_ops - 1) // 2
        assert len(_columns(case, hap, case.haps[hap].index(a), "SNV")) == (single + 1) // 2
        assert all(e.limit == 0 for e in edits_of(case, hap, case.haps[hap].index(a)) if e.kind != "SNV" and e.r > lead)
    return case


def adjacent(min_sv_size):
    """Gaps beside gaps, SNVs beside gaps, gaps at and one column behind an alignment's start, and the sizes on either side
    of --min_sv_size."""
    L = min_sv_size
    b = Builder("adjacent" if L == 40 else "adjacent-min%d" % L, min_sv_size=L)
    c = ORDER[2]
    s = Script().M(30)
    s.I("ACG").D(2).M(30)                                   # I directly followed by D
    s.D(2).I("TT").M(30)                                    # D directly followed by I
    s.M(30, snv=[28, 29]).I("GA").M(30, snv=[0])            # SNVs two columns and one column (the anchor) in front, and right behind
    s.M(10, snv=[9]).D(3).M(30, snv=[0])                    # the same around a deletion
    s.D(1).M(1).D(1).M(30)                                  # two gaps one aligned column apart
    s.I("CA").D(L).M(30)                                    # a small gap directly in front of a large one
    s.D(L).I("GT").M(30)                                    # ... and directly behind it
    s.D(2).I(b.bases(L)).M(30)
    s.D(L - 1).M(30).D(L).M(30)                             # min_sv_size - 1 and min_sv_size
    s.I(b.bases(L - 1)).M(30).I(b.bases(L)).M(30)
    b.align(0, c, 1000, s)
    b.align(0, c, 3000, Script().M(1).D(2).M(50, snv=[10]))             # a gap one column behind the start
    b.align(0, c, 3200, Script().I("AC").M(50, snv=[0]))               # at the first reference position: no_anchor
    b.align(0, c, 3400, Script().S("ACG").D(2).M(50))                  # ... behind a soft clip
    b.align(0, c, 3600, Script().H(7).I("G").M(50).H(3), flag=2048)    # ... behind a hard clip
    b.align(1, c, 900, Script().M(3000, snv=[150, 2120]))              # the other haplotype: the reference nearly everywhere
    case = b.case()
    gaps = [e for e in edits_of(case, 0, 0) if e.kind != "SNV"]
    pairs = [(x.kind, y.kind) for x, y in zip(gaps, gaps[1:]) if y.limit == 0 and y.r == x.r + x.ref_len]
    assert ("INS", "DEL") in pairs and ("DEL", "INS") in pairs
    assert any(y.r == x.r + x.ref_len + 1 and x.kind == y.kind == "DEL" for x, y in zip(gaps, gaps[1:]))
    assert sorted(size(e) for e in gaps if size(e) >= L - 1) == [L - 1, L - 1, L, L, L, L, L]
    snv = set(e.r for e in edits_of(case, 0, 0) if e.kind == "SNV")
    assert any(g.r - 2 in snv and g.r - 1 in snv and g.r in snv for g in gaps if g.kind == "INS")
    assert any(g.r - 1 in snv and g.r + g.ref_len in snv for g in gaps if g.kind == "DEL")
    assert [reason(case, e, False) for a in (2, 3, 4) for e in edits_of(case, 0, a) if e.kind != "SNV"] == ["no_anchor"] * 3
    assert [e.r for e in edits_of(case, 0, 1) if e.kind == "DEL"] == [1]
    b.expect["no_anchor"] = [3, 0]
    return case._replace(expect=dict(b.expect))


def repeats():
    """Gaps at the right end of homopolymers and short tandem repeats, for --left_align: true shifts on either side of the
    lane form's steps and the wave form's columns, and every way a walk ends early."""
    b = Builder("repeats")
    c0, c1 = ORDER[1], ORDER[0]
    shifts = [LS - 1, LS, LS + 1, W - 1, W, W + 1, 2 * W + 1]
    want = {}
    at, del_runs, ins_runs = 1000, [], []
    for k, base in zip(shifts, "ACGTACG"):          # a deleted unit needs k + 1 copies to move k, an inserted one k
        del_runs.append(b.plant_run(c0, at, base, k + 1) + (base, k))
        at += k + 80
        ins_runs.append(b.plant_run(c0, at, base, k) + (base, k))
        at += k + 80
    for unit in ("AC", "ACG"):                      # period 2 and 3, longer than 2 W
        copies = (2 * W) // len(unit) + 4
        del_runs.append(b.plant_run(c0, at, unit, copies) + (unit, (copies - 1) * len(unit)))
        at += copies * len(unit) + 80
        ins_runs.append(b.plant_run(c0, at, unit, copies) + (unit, copies * len(unit)))
        at += copies * len(unit) + 80
    end = at
    for hap, mine, runs in ((0, "DEL", del_runs), (1, "INS", ins_runs)):
        s, r0 = Script(), 900
        for lo, hi, unit, k in runs:
            if mine == "DEL":
                s.M(hi - len(unit) - r0 - s.r).D(len(unit))
            else:
                s.M(hi - r0 - s.r).I(unit)
            want[(hap, c0, hi - len(unit) if mine == "DEL" else hi, mine)] = k
        s.M(end - r0 - s.r)
        b.align(hap, c0, r0, s)
    # every way a walk ends early, on the other contig: haplotype 1 writes, haplotype 2 is the reference
    lo, hi = b.plant_run(c1, 1000, "A", 20)         # the run reaches the alignment's first position: the limit binds
    b.align(0, c1, lo, Script().M(19).D(1).M(100))
    want[(0, c1, lo + 19, "DEL")] = 18
    lo, hi = b.plant_run(c1, 1400, "C", 30)         # an SNV of the contig inside the run
    b.align(0, c1, lo - 100, Script().M(100 + 29, snv=[110]).D(1).M(100))
    want[(0, c1, lo + 29, "DEL")] = 18
    lo, hi = b.plant_run(c1, 1800, "G", 30)         # another small gap inside the run: the limit binds
    b.align(0, c1, lo - 100, Script().M(110).D(1).M(18).D(1).M(100))
    want[(0, c1, lo + 10, "DEL")], want[(0, c1, lo + 29, "DEL")] = 10, 17
    lo, hi = b.plant_run(c1, 2200, "T", 30)         # a large op inside the run
    b.align(0, c1, lo - 100, Script().M(110).I(b.bases(45)).M(19).D(1).M(100))
    want[(0, c1, lo + 29, "DEL")] = 18
    b.plant(c1, 2699, "T" + "ACG" * 20 + "AC" + "T")   # a period-3 run that ends inside a unit: the inserted bases come out rotated
    b.align(0, c1, 2600, Script().M(100 + 62).I("GAC").M(100))
    want[(0, c1, 2762, "INS")] = 62
    b.align(1, c1, 800, Script().M(2400))
    case = b.case()
    assert placed(case, [e for e in case.edits if e.pos == 2762][0], True) == (2700, 0, "ACG")
    got = {(e.hap, e.contig, e.pos, e.kind): left_shift(case, e) for e in case.edits if is_small_gap(case, e)}
    assert got == want, (got, want)
    assert sorted(set(k for (h, c, p, kind), k in want.items() if c == c0 and k <= 2 * W + 1)) == shifts
    assert all(k > 2 * W for lo, hi, unit, k in del_runs + ins_runs if len(unit) > 1)
    return case._replace(expect={"shift": want})


def letters():
    """Letter case on either side, and N in the reference under a column, in inserted bases, as an anchor and among deleted
    bases."""
    b = Builder("letters")
    c = ORDER[0]
    b.plant(c, 1000, b.bases(400).lower())
    b.align(0, c, 1000, Script().M(100, snv=[0, 50, 99]).I("ACC").M(100, snv=[3]).D(4).M(196, snv=[195]))   # lower-case reference
    b.plant(c, 2000, b.bases(400).upper())
    b.align(0, c, 2000, Script().M(100, snv=[1, 50]).I("GT").M(100).D(2).M(198, snv=[7]), lower=True)        # lower-case SEQ
    b.plant(c, 3000, b.bases(200).upper())
    b.plant(c, 3050, "N")
    b.plant(c, 3060, "n")
    b.align(0, c, 3000, Script().M(200, snv=[49, 51, 100]))      # N under an M column: no event
    b.plant(c, 4000, b.bases(100).upper())
    b.align(0, c, 4000, Script().M(50).I("ACNGT").M(50))         # N among inserted bases
    b.plant(c, 5000, b.bases(49).upper() + "N" + b.bases(50).upper())
    b.align(0, c, 5000, Script().M(50).I("AC").M(50))            # N as the anchor
    b.plant(c, 6000, b.bases(51).upper() + "N" + b.bases(48).upper())
    b.align(0, c, 6000, Script().M(50).D(3).M(47))               # N among deleted bases
    # the other haplotype: the reference, with an SNV beside each of haplotype 1's dropped gaps (DESIGN §3.18's `0` looks at
    # kept events only — tests/test_small_rebuild_host.py says what that means here)
    b.align(1, c, 900, Script().M(5600, snv=[4049 - 900, 6050 - 900]))
    case = b.case()
    drops = [(e.pos, reason(case, e, False)) for e in edits_of(case, 0) if e.kind != "SNV" and reason(case, e, False)]
    assert drops == [(4050, "ambiguous_base"), (5050, "ambiguous_base"), (6050, "ambiguous_base")]
    assert case.genome[c][1000:1400].islower() and case.haps[0][1].lower and case.genome[c][2000:2400].isupper()
    assert case.haps[0][2].seq[50] == "N" and case.haps[0][2].seq[60] == "N" and len(_columns(case, 0, 2, "SNV")) == 3
    return case._replace(expect={"ambiguous_base": [3, 0], "zero_over_dropped": [(c, 4050), (c, 6051)]})


def records():
    """What COLLECT visits and what the command uses: strand, supplementary with hard clips, secondary, low MAPQ, no SEQ, an N
    op — and records on every contig."""
    b = Builder("records")
    c0, c1, c2 = ORDER
    plain = lambda n: Script().M(n // 2, snv=[5, n // 4]).I("CT").M(20).D(3).M(n - n // 2 - 23, snv=[11])
    b.align(0, c0, 1000, plain(400), flag=16, name="reverse")
    b.align(0, c0, 1100, plain(200), flag=256, name="secondary")                      # over `reverse`: it must not count as cover
    b.align(0, c0, 2000, Script().H(50).M(100, snv=[0, 99]).I("A").M(100).H(30), flag=2048, name="supplementary")
    b.align(0, c0, 3500, plain(300), mapq=5, name="low_mapq")
    b.align(0, c0, 3600, plain(300), flag=4, name="flagged_unmapped")
    b.align(0, c0, 4000, plain(300), stored=False, name="no_sequence")
    b.align(0, c0, 4250, Script().M(250, snv=[20, 150]), name="beside_no_sequence")    # [4250, 4300) lies under `no_sequence` too
    b.align(0, c0, 5000, Script().M(50, snv=[10]).N(20).M(50, snv=[10]), name="spliced")
    b.align(0, c0, 5060, Script().M(100, snv=[5, 80]), name="beside_spliced")          # [5060, 5120) lies under `spliced` too
    for hap in (0, 1):
        for k, c in enumerate((c1, c2, c0)):
            b.align(hap, c, 7000 + 40 * k + hap * 150, plain(500 + 10 * k), flag=16 * (k % 2), name="every_contig_%d_%d" % (hap, k))
    b.align(1, c0, 900, Script().M(4500, snv=[130, 1150, 3370]))
    b.align(1, c0, 6000, plain(400), mapq=19, name="one_below_min_mapq")
    b.align(1, c0, 6000, plain(400), mapq=20, name="at_min_mapq")
    case = b.case()
    names = lambda want: sorted(a.name for h in case.haps for a in h if status(case, a) == want)
    assert names("not_visited") == ["flagged_unmapped", "low_mapq", "one_below_min_mapq", "secondary"]
    assert names("no_sequence") == ["no_sequence"] and names("spliced") == ["spliced"]
    assert set(a.contig for a in case.haps[0] if status(case, a) == "used") == set(ORDER) == set(a.contig for a in case.haps[1])
    return case._replace(expect={"not_visited": names("not_visited"), "no_sequence": [1, 0], "spliced": [1, 0]})


def coverage():
    """Alignments of one haplotype that overlap by 1, by 100, one inside another, and two that abut."""
    b = Builder("coverage")
    c = ORDER[1]
    b.align(0, c, 1000, Script().M(2000, snv=[10, 1998, 1999]), name="A")                  # 2998: the last singly covered column; 2999: in the overlap
    b.align(0, c, 2999, Script().M(2001, snv=[0, 1, 500]), name="B")
    b.align(0, c, 6000, Script().M(1897, snv=[100]).D(5).M(98, snv=[50]), name="C")       # the deletion [7897, 7902) crosses into the overlap
    b.align(0, c, 7900, Script().M(50, snv=[48]).I("GG").M(2050, snv=[1000]), name="D")   # both say the SNV at 7948; the insertion lies in the overlap
    b.align(0, c, 11000, Script().M(4000, snv=[500, 1500, 3500]), name="E")
    b.align(0, c, 12000, Script().M(500, snv=[100]).D(2).M(498), name="F")                # inside E: no stretch of its own
    b.align(0, c, 16000, Script().M(1990, snv=[1989]).D(5).M(5, snv=[4]), name="G")       # G and H abut at 18000
    b.align(0, c, 18000, Script().M(2000, snv=[0, 3]), name="H")
    # the other haplotype: one alignment over each place; a deletion over haplotype 1's abutment
    b.align(1, c, 900, Script().M(4500, snv=[2098, 2099]))                                 # 2998 and 2999 as haplotype 1 has them
    b.align(1, c, 5900, Script().M(4300, snv=[2048]))                                      # 7948
    b.align(1, c, 10900, Script().M(4300, snv=[600]))
    b.align(1, c, 15900, Script().M(2097).D(6).M(2100))                                    # [17997, 18003)
    case = b.case()
    a = {x.name: x for x in case.haps[0]}
    end = lambda x: x.start + ref_length(x.ops)
    assert end(a["A"]) - a["B"].start == 1 and end(a["C"]) - a["D"].start == 100 and end(a["G"]) == a["H"].start
    assert a["E"].start < a["F"].start and end(a["F"]) < end(a["E"])
    # not singly covered on haplotype 1: A's and B's SNV at 2999, C's deletion and its SNV at 7952, D's SNV at 7948 and its
    # insertion, E's SNV at 12500, F's SNV and deletion
    return case._replace(expect={"multiply_covered": [9, 0], "no_stretch": [1, 0], "over_abutment": (c, 17997)})


def diploid():
    """The same event on both haplotypes in the same and in different placements, het events over the other haplotype's
    reference, overlapping alleles, and events where the other haplotype has nothing."""
    b = Builder("diploid")
    c = ORDER[2]
    t_lo, _ = b.plant_run(c, 2000, "T", 12)
    g_lo, g_hi = b.plant_run(c, 2200, "G", 9)
    b.plant(c, 2598, "CATGA")
    both = lambda s: s.M(100, snv=[50]).I("CAT").M(100).D(4).M(300)                        # 1|1 three times
    to = lambda s, r: s.M(r - s.r)
    h1 = both(Script())
    to(h1, t_lo + 11 - 1000).D(1)                                                          # the T run's last base
    to(h1, g_hi - 1000).I("G")                                                             # behind the G run
    to(h1, 1400).M(100, snv=[0])                                                           # a het SNV at 2400
    to(h1, 1600).M(100, snv=[0])                                                           # the SNV at 2600
    to(h1, 1900)
    h2 = both(Script())
    to(h2, t_lo + 4 - 1000).D(1)                                                           # the T run's fifth base
    to(h2, g_lo + 3 - 1000).I("G")                                                         # inside the G run
    to(h2, 1598).D(5)                                                                      # the deletion [2598, 2603) over that SNV
    to(h2, 1900)
    assert h1.r == h2.r
    b.align(0, c, 1000, h1)
    b.align(1, c, 1000, h2)
    b.align(0, c, 5000, Script().M(100, snv=[40]).D(2).M(100).I("AC").M(100))             # nothing of haplotype 2 here
    b.align(1, c, 6000, Script().M(100, snv=[60]).I("T").M(200))                           # nothing of haplotype 1 here
    case = b.case()
    U = case.genome[c].upper()
    gt = {False: {}, True: {}}
    gt[False][(c, 1051, "SNV")] = gt[True][(c, 1051, "SNV")] = "1|1"
    for mode in (False, True):
        gt[mode][(c, 2401, "SNV")] = "1|0"
        gt[mode][(c, 2601, "SNV")], gt[mode][(c, 2598, "DEL")] = "1|.", ".|1"
        gt[mode][(c, 5041, "SNV")], gt[mode][(c, 6061, "SNV")] = "1|.", ".|1"
    gt[False][(c, t_lo + 11, "DEL")], gt[False][(c, t_lo + 4, "DEL")] = "1|0", "0|1"       # two placements, two records
    gt[True][(c, t_lo, "DEL")] = "1|1"                                                      # one record at the leftmost position
    gt[False][(c, g_hi, "INS")], gt[False][(c, g_lo + 3, "INS")] = "1|0", "0|1"
    gt[True][(c, g_lo, "INS")] = "1|1"
    assert U[t_lo:t_lo + 12] == "T" * 12 and U[g_lo:g_hi] == "G" * 9 and U[2598:2603] == "CATGA"
    return case._replace(expect={"genotype": gt})


def random_case(seed):
    """About 25 alignments per haplotype laid over the three contigs with gaps, abutments and overlaps between them; blocks of
    1 to 100 aligned columns with 8 % SNVs, gaps of 1 to 5 bases — 60 % of them tandem copies of the bases in front —, now
    and then I-then-D, D-then-I, a leading insertion, clips, an op of --min_sv_size or more, and a record the command must
    not use."""
    b = Builder("random-%d" % seed, random_n=6)
    rng = b.rng
    for c in ORDER:  # a genome with short tandem repeats, so that deletions find copies in front of them too
        seq, p = b.ref[c], 300
        while p < len(seq) - 300:
            n, copies = rng.randrange(1, 6), rng.randrange(2, 9)
            unit = seq[p:p + n]
            for k in range(1, copies):
                seq[p + k * n:p + (k + 1) * n] = unit
            p += n * copies + rng.randrange(20, 200)
    for hap in (0, 1):
        for c in ORDER:
            at, length = rng.randrange(100, 600), len(b.ref[c])
            while at < length - 8000:
                want = rng.randrange(1500, 7000)
                s, special = Script(), rng.random()
                if special < 0.15:
                    s.S(b.bases(rng.randrange(1, 30)))
                elif special < 0.25:
                    s.H(rng.randrange(1, 30))
                if rng.random() < 0.15:
                    s.I(b.bases(rng.randrange(1, 4)))                   # a leading insertion: no_anchor
                while s.r < want:
                    n = rng.randrange(1, 101)
                    cols = [j for j in range(n) if rng.random() < 0.08 and b.base(c, at + s.r + j) in ACGT]
                    s.M(n, snv=cols)
                    kind, g = rng.random(), rng.randrange(1, 6)
                    if kind < 0.03:
                        g = rng.randrange(40, 60)                       # svim-asm's
                    tandem = rng.random() < 0.6
                    here = at + s.r
                    if kind < 0.5 or 0.9 <= kind < 0.95:                # an insertion (from 0.9 on: directly followed by a deletion)
                        front = "".join(b.base(c, p) for p in range(here - g, here))
                        s.I(front if tandem and g < 40 and set(front) <= set(ACGT) else b.bases(g))
                        if kind >= 0.9:
                            s.D(rng.randrange(1, 6))
                    else:                                               # a deletion (from 0.95 on: directly followed by an insertion)
                        if tandem and g < 40:
                            fits = [m for m in range(1, 6) if b.ref[c][here - m:here] == b.ref[c][here:here + m]]
                            g = rng.choice(fits) if fits else g
                        s.D(g)
                        if kind >= 0.95:
                            s.I(b.bases(rng.randrange(1, 6)))
                s.M(rng.randrange(1, 101))
                kw, odd = {}, rng.random()
                if odd < 0.04:
                    kw = dict(flag=256)
                elif odd < 0.08:
                    kw = dict(mapq=rng.randrange(0, 20))
                elif odd < 0.12:
                    kw = dict(stored=False)
                elif odd < 0.16:
                    s.N(rng.randrange(5, 50)).M(rng.randrange(10, 100))
                if special >= 0.9:
                    s.S(b.bases(rng.randrange(1, 30)))
                b.align(hap, c, at, s, flag=kw.pop("flag", 0) | (16 if rng.random() < 0.5 else 0), **kw)
                step = rng.random()
                at += s.r + (0 if step < 0.1 else -rng.randrange(1, 300) if step < 0.4 else rng.randrange(1, 800))
    case = b.case()
    n_aln = [len(h) for h in case.haps]
    gaps = [e for e in case.edits if e.kind != "SNV"]
    assert all(18 <= n <= 40 for n in n_aln), n_aln
    assert len(gaps) > 600 and sum(1 for e in gaps if e.limit == 0 and e.r > 0) > 10 and sum(1 for e in gaps if e.r == 0) > 0
    return case


NAMED = {"tile-columns": tile_columns, "op-per-column": op_per_column, "adjacent": lambda: adjacent(40), "adjacent-min5": lambda: adjacent(5),
         "repeats": repeats, "letters": letters, "records": records, "coverage": coverage, "diploid": diploid}
NAMES = tuple(NAMED) + tuple("random-%d" % s for s in SEEDS)
LEFTMOST = ("repeats", "diploid")                                   # where every shifted record is held to be leftmost
COMPARED = ("repeats", "adjacent", "adjacent-min5", "diploid") + tuple("random-%d" % s for s in SEEDS)


@functools.lru_cache(maxsize=None)
def case(name):
    return NAMED[name]() if name in NAMED else random_case(int(name.split("-")[1]))
