"""svim-asm-small, --left_align and svim-asm-small-compare held to the contigs they must rebuild, where there is no GPU
(DESIGN.md §3.18-§3.20): the commands with the kernels answered exactly as tests/test_small_host.py,
tests/test_small_leftalign_host.py and tests/test_smallcmp_host.py answer them, on the cases of tests/rebuild_cases.py,
judged by tests/rebuild_judge.py.  tests/test_gpu_small_rebuild.py runs the same checks (the functions below) on the real
kernels.

What is asserted, for every case, with and without --left_align, from SAM text (records shuffled) and from BAM:
  a  rebuild     per haplotype, per used alignment, per maximal stretch of depth 1 inside it: the reference with the records
                 the haplotype carries there, the truth's ops of --min_sv_size or more and the truth edits the command must
                 drop IS the contig's aligned bases.  Every carried record lies in exactly one such stretch.
  b  accounting  every count of summary.json is the generator's own, per haplotype; multiply_covered from the judge's depth.
  c  genotypes   1: the carried records ARE the kept truth edits (as a set, in the placement of the run);
                 0: the record's REF span lies inside ONE stretch of the haplotype and none of its kept truth edits' spans
                 overlaps it; `.` everywhere else — both directions, every record, every haplotype.
  d  left_align  a to c unchanged, the SNV lines are those of the run without the option, and in `repeats` and `diploid` every
                 carried gap is leftmost: one base further left the alignment's string changes, or the column in front of the
                 anchor is the end of the gap in front (or the alignment's start) in the truth's CIGAR.
  e  knobs       --batch_bases for at least three batches, the largest record alone in its batch: the same bytes.
  4  compare     the truth in another spelling (isolated gaps right-aligned, neighbouring SNVs as one MNP, phased) against
                 small.vcf inside the stretches: no FN, no FP, no ref_mismatch.

Two places where `0` is narrower than "the haplotype shows the reference", both as DESIGN §3.18 states it and both held
here by name: (1) a span over two ABUTTING alignments of the haplotype has depth 1 throughout and is `.` — an alignment
boundary is a breakpoint of the assembly (§3.15), the stretches above end there too; (2) only KEPT events count as
touching, so a haplotype whose dropped event (ambiguous_base, multiply_covered, no_anchor) lies under the other
haplotype's record is `0` there, and so is a haplotype over the single coverage of a record the command does not use
(no_sequence, spliced): such a record covers, and none of its events is ever kept.
(2) is the rule the text states in these words, not a reading of it, so the tests hold the command to it and `letters`
pins the two records where it shows; whether `0` should ask for more is a change of the command's outputs and not made
here."""
import functools
import json
import os

import pytest

from svim_asm_amd import small_cli, smallcmp_cli
from tests import helpers, rebuild_cases as RC, rebuild_judge as J
from tests import test_small_host as host, test_small_leftalign_host as la, test_smallcmp_host as cmp_host
from tests.test_compare_host import restated_cover_query

COUNTS = ("records_used", "no_sequence", "spliced", "mismatches", "small_indels", "no_anchor", "ambiguous_base", "multiply_covered")
KINDS = ("sam", "bam")
MODES = (False, True)
_FILES = {}    # (backend, case, left_align, kind) -> (small.vcf text, summary.json text)


@pytest.fixture
def stand_ins(monkeypatch):
    ctx = helpers.OracleBackedContext
    monkeypatch.setattr(ctx, "cigar_mismatch", host.restated_cigar_mismatch, raising=False)
    monkeypatch.setattr(ctx, "cover_single", host.restated_cover_single, raising=False)
    monkeypatch.setattr(ctx, "indel_shift", la.restated_indel_shift, raising=False)
    monkeypatch.setattr(ctx, "variant_replay", cmp_host.restated_variant_replay, raising=False)
    monkeypatch.setattr(ctx, "cover_query", restated_cover_query, raising=False)
    monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", "0")
    for calls in (host.CALLS, la.CALLS, cmp_host.CALLS):
        for k in calls:
            calls[k] = 0
    return helpers.oracle_backed_device(monkeypatch)


# ------------------------------------------------------------------------------------------------ inputs and runs
@pytest.fixture(scope="session")
def rebuild_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rebuild"))


def inputs(root, name, kind):
    """[genome, hap1, hap2] of a case, written once per session."""
    case = RC.case(name)
    d = os.path.join(root, "in", name)
    os.makedirs(d, exist_ok=True)
    genome = os.path.join(d, "genome.fa")
    if not os.path.exists(genome):
        RC.write_fasta(genome, case)
    paths = [genome]
    for h in (0, 1):
        p = os.path.join(d, "hap%d.%s" % (h + 1, kind))
        if not os.path.exists(p):
            RC.write_sam(p, case, h, shuffle_seed=17 + h) if kind == "sam" else RC.write_bam(p, case, h)
        paths.append(p)
    return paths


def argv_of(root, name, kind, left_align, out, extra=()):
    case = RC.case(name)
    argv = [out] + inputs(root, name, kind)
    if case.min_sv_size != 40:
        argv += ["--min_sv_size", str(case.min_sv_size)]
    return argv + (["--left_align"] if left_align else []) + list(extra)


def read_outputs(out):
    assert sorted(os.listdir(out)) == ["small.vcf", "summary.json"]
    return open(os.path.join(out, "small.vcf")).read(), open(os.path.join(out, "summary.json")).read()


def plain_run(root, backend, name, left_align, kind):
    """The files of the run without further options, made once per session and backend; returns (out_dir, vcf, summary)."""
    key = (backend, name, left_align, kind)
    out = os.path.join(root, backend, "%s.%s.%s" % (name, "left" if left_align else "asis", kind))
    if key not in _FILES:
        assert small_cli.main(argv_of(root, name, kind, left_align, out)) == 0
        _FILES[key] = read_outputs(out)
    return (out,) + _FILES[key]


# ------------------------------------------------------------------------------------------------ what the truth expects
class Truth(object):
    pass


@functools.lru_cache(maxsize=None)
def truth(name, left_align):
    """Per haplotype, from the generator and the judge alone: the counts, the kept edits, the dropped and the large ones per
    alignment (each as (pos, ref_len, bases) in the placement of the run), the depth and the stretches."""
    case = RC.case(name)
    lengths = {c: len(case.genome[c]) for c in case.order}
    t = Truth()
    t.case, t.lengths, t.haps = case, lengths, []
    by_aln = {}
    for e in case.edits:
        by_aln.setdefault((e.hap, e.aln), []).append(e)
    for h, alns in enumerate(case.haps):
        x = Truth()
        x.depth = J.depth(alns, lengths, case.min_mapq)
        x.counts = dict.fromkeys(COUNTS + (("left_aligned", "shifted_bases") if left_align else ()), 0)
        x.kept, x.extra, x.used, x.stretches, x.gap_ends, x.segments = set(), {}, [], {}, {}, {c: [] for c in case.order}
        for i, a in enumerate(alns):
            st = RC.status(case, a)
            if st != "not_visited":  # (a record that is visited covers, used or not)
                x.segments[a.contig] += J.stretches(a, x.depth)
            if st in ("no_sequence", "spliced"):
                x.counts[st] += 1
            if st != "used":
                continue
            x.counts["records_used"] += 1
            x.used.append(i)
            x.stretches[i] = J.stretches(a, x.depth)
            x.extra[i] = []   # the truth edits of this alignment that are NOT records: svim-asm's, and the dropped ones
            x.gap_ends[i] = set([a.start] + [e.pos + e.ref_len for e in by_aln.get((h, i), ()) if e.kind != "SNV"])
            for e in by_aln.get((h, i), ()):
                why, where = RC.reason(case, e, left_align), RC.placed(case, e, left_align)
                if why == "large":
                    x.extra[i].append(where)
                    continue
                if e.kind == "SNV":
                    x.counts["mismatches"] += 1
                else:
                    x.counts["small_indels"] += 1
                    if left_align:
                        k = RC.left_shift(case, e)
                        x.counts["left_aligned"] += 1 if k else 0
                        x.counts["shifted_bases"] += k
                if why is None:
                    lo, hi = RC.span(e.kind, where[0], where[1])
                    if not all(x.depth[e.contig][p] == 1 for p in range(lo, hi)):
                        why = "multiply_covered"
                if why is None:
                    assert (e.contig, where) not in x.kept, "the case spells one edit twice on one haplotype"
                    x.kept.add((e.contig, where))
                else:
                    x.counts[why] += 1
                    x.extra[i].append(where)
        x.touch = {c: bytearray(n) for c, n in lengths.items()}
        for contig, (pos, ref_len, bases) in x.kept:
            lo, hi = RC.span("SNV" if ref_len == 1 and len(bases) == 1 else "GAP", pos, ref_len)
            for p in range(lo, hi):
                x.touch[contig][p] = 1
        t.haps.append(x)
    return t


def record_span(rec):
    pos, ref_len, bases = J.stripped(rec)
    return RC.span(J.kind_of(rec[2], rec[3]), pos, ref_len)


# ------------------------------------------------------------------------------------------------ the checks
def check_run(name, left_align, out):
    """a, b, c (and d's leftmost rule) on the files of one run."""
    t = truth(name, left_align)
    case = t.case
    records = J.read_vcf(os.path.join(out, "small.vcf"))
    summary = json.load(open(os.path.join(out, "summary.json")))
    keys = [(case.order.index(r[0]), r[1], r[2], r[3]) for r in records]
    assert keys == sorted(set(keys)), "the records are not distinct or not in genome order"
    assert all(len(r[4]) == 2 and set(r[4]) <= set("01.") and "1" in r[4] for r in records)
    # ---- b: accounting
    assert [dict(h) for h in summary["haplotypes"]] == [x.counts for x in t.haps]
    for key, want in case.expect.items():
        if key in COUNTS:
            assert [x.counts[key] for x in t.haps] == want, key   # (the case holds what its name says)
    assert summary["records"] == len(records)
    for h, x in enumerate(t.haps):
        carried = [r for r in records if r[4][h] == "1"]
        # ---- c: the carried records are the kept truth edits
        assert set((r[0], J.stripped(r)) for r in carried) == x.kept and len(carried) == len(x.kept)
        # ---- a: rebuild
        by_contig = {}
        for r in carried:
            by_contig.setdefault(r[0], []).append((record_span(r), J.stripped(r)))
        assigned = without = 0
        for i in x.used:
            a = case.haps[h][i]
            reference = case.genome[a.contig]
            without += 0 if x.stretches[i] else 1
            own = []
            for lo, hi in x.stretches[i]:
                here = [e for (s_lo, s_hi), e in by_contig.get(a.contig, ()) if lo <= s_lo and s_hi <= hi]
                assigned += len(here)
                own += here
                edits = here + [c for c in (J.clipped(e, lo, hi) for e in x.extra[i]) if c is not None]
                assert J.rebuild(reference, lo, hi, edits) == J.aligned_bases(a, lo, hi).upper(), (name, h, a.name, lo, hi)
            # ---- d: leftmost
            if left_align and name in RC.LEFTMOST:
                end = a.start + J.ref_length(a.ops)
                every = own + [c for c in (J.clipped(e, a.start, end) for e in x.extra[i]) if c is not None]
                whole = J.aligned_bases(a, a.start, end).upper()
                assert J.rebuild(reference, a.start, end, every) == whole
                for k, e in enumerate(every[:len(own)]):
                    if e[1] == 1 and len(e[2]) == 1:
                        continue
                    moved = J.one_left(e, reference)
                    same = moved[0] > a.start and J.rebuild(reference, a.start, end, every[:k] + [moved] + every[k + 1:], strict=False) == whole
                    assert not same or e[0] - 1 in x.gap_ends[i], "not leftmost: %r of %s" % (e, a.name)
        assert assigned == len(carried), "a carried record outside every stretch of its haplotype, or in two"
        assert without == case.expect.get("no_stretch", [0, 0])[h]
    # ---- c: 0 and `.`
    for r in records:
        lo, hi = record_span(r)
        for h, x in enumerate(t.haps):
            if (r[0], J.stripped(r)) in x.kept:
                want = "1"
            else:
                inside = any(a <= lo and hi <= b for a, b in x.segments[r[0]])
                want = "0" if inside and not any(x.touch[r[0]][lo:hi]) else "."
            assert r[4][h] == want, (name, r, h, want)
    return records, summary


def check_named_expectations(name, left_align, records):
    """What single cases promise beyond the general checks."""
    case = RC.case(name)
    gt = {(r[0], r[1], J.kind_of(r[2], r[3])): "|".join(r[4]) for r in records}
    for key, want in case.expect.get("genotype", {}).get(left_align, {}).items():
        assert gt.get(key) == want, (key, gt.get(key), want)
    if name == "diploid":
        assert ("1|1" in [v for k, v in gt.items() if k[2] != "SNV" and 1900 < k[1] < 2300]) == left_align  # the repeats' indels
    for contig, pos in case.expect.get("zero_over_dropped", ()):
        assert gt[(contig, pos, "SNV")] == "0|1"      # (2) of the module's text
    if "over_abutment" in case.expect:
        contig, pos = case.expect["over_abutment"]
        assert gt[(contig, pos, "DEL")] == ".|1"      # (1) of the module's text
        d = truth(name, left_align).haps[0].depth[contig]
        assert all(d[p] == 1 for p in range(pos - 1, pos + 6))
    if "not_visited" in case.expect:
        hidden = [e for h, alns in enumerate(case.haps) for i, a in enumerate(alns) if a.name in case.expect["not_visited"] for e in RC.edits_of(case, h, i)]
        shown = set((r[0], J.stripped(r)) for r in records)
        own = set().union(*[x.kept for x in truth(name, left_align).haps])
        assert hidden and all((e.contig, RC.placed(case, e, left_align)) not in shown - own for e in hidden)


def snv_lines(text):
    return [l for l in text.splitlines() if not l.startswith("#") and len(l.split("\t")[3]) == len(l.split("\t")[4]) == 1]


def batch_limit(name):
    """A --batch_bases one below the cost (reference interval plus SEQ) of a haplotype's costliest record — of the haplotype
    where that is less: the record is above the limit and alone in its batch."""
    case = RC.case(name)
    return min(max(J.ref_length(a.ops) + len(a.seq) for a in h if RC.status(case, a) == "used") for h in case.haps) - 1


# ---- 4: svim-asm-small-compare
@functools.lru_cache(maxsize=None)
def truth_files(root, name, left_align):
    """(truth.vcf in another spelling, stretches.bed) of a case: the kept truth edits only."""
    t = truth(name, left_align)
    case = t.case
    per_hap, rows = [], []
    for h, x in enumerate(t.haps):
        out = []
        for i in x.used:
            a = case.haps[h][i]
            for lo, hi in x.stretches[i]:
                rows.append((a.contig, lo, hi))
                inside = [e for c, e in x.kept if c == a.contig and lo <= RC.span("SNV" if e[1] == 1 and len(e[2]) == 1 else "GAP", e[0], e[1])[0]
                          and RC.span("SNV" if e[1] == 1 and len(e[2]) == 1 else "GAP", e[0], e[1])[1] <= hi]
                out += [(a.contig,) + rec for rec in J.respelled(inside, case.genome[a.contig], lo, hi)]
        assert len(out) <= len(x.kept)
        per_hap.append(out)
    d = os.path.join(root, "truth")
    os.makedirs(d, exist_ok=True)
    stem = os.path.join(d, "%s.%s" % (name, "left" if left_align else "asis"))
    rows.sort(key=lambda r: (case.order.index(r[0]), r[1], r[2]))
    return J.write_truth_vcf(stem + ".vcf", list(case.order), t.lengths, per_hap), J.write_bed(stem + ".bed", rows)


def check_compare(root, backend, name, left_align, kind="sam"):
    out, _vcf, _summary = plain_run(root, backend, name, left_align, kind)
    base, bed = truth_files(root, name, left_align)
    got = os.path.join(root, backend, "cmp.%s.%s" % (name, "left" if left_align else "asis"))
    argv = [got, inputs(root, name, kind)[0], base, os.path.join(out, "small.vcf"), "--include_bed", bed, "--batch_bases", "3000" if name.startswith("random") else "60",
            "--cluster_distance", "600" if name == "repeats" else "50", "--max_cluster", "1000000"]
    assert smallcmp_cli.main(argv) == 0
    summary = json.load(open(os.path.join(got, "summary.json")))
    for side in ("base", "comp"):
        assert summary[side]["ref_mismatch"] == 0 and summary[side]["out_of_regions"] == 0 and summary[side]["too_large"] == 0, summary[side]
        assert summary[side]["compared"] == summary[side]["records"] > 0
    assert (summary["FN"], summary["FP"]) == (0, 0), {k: summary[k] for k in ("TP-base", "FN", "TP-comp", "FP", "clusters", "base", "comp")}
    assert summary["TP-base"] == summary["base"]["compared"] and summary["TP-comp"] == summary["comp"]["compared"]
    assert summary["base"]["conflict"] == summary["comp"]["conflict"] == 0
    return summary


# ------------------------------------------------------------------------------------------------ the tests
def test_every_case_builds_and_shows_what_its_name_says():
    assert len(RC.NAMES) == 15
    for name in RC.NAMES:
        case = RC.case(name)  # (the builders assert on their own arrays)
        assert list(case.order) != sorted(case.order) and len(case.order) == 3
        for c in case.order:
            seq = case.genome[c]
            assert 30000 <= len(seq) <= 50000 and "N" in seq.upper() and seq != seq.upper() and seq != seq.lower()
        for h in case.haps:
            for a in h:
                assert len(a.seq) == sum(n for op, n in a.ops if op in J.QRY_OPS) and a.start + J.ref_length(a.ops) <= len(case.genome[a.contig])
    assert max(J.ref_length(a.ops) for h in RC.case("tile-columns").haps for a in h) == 2 * RC.T + 5
    assert max(len(a.ops) for h in RC.case("op-per-column").haps for a in h) == 2 * RC.LC + 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("left_align", MODES, ids=("asis", "left"))
@pytest.mark.parametrize("name", RC.NAMES)
def test_rebuild(name, left_align, kind, rebuild_dir, stand_ins):
    out, vcf, _ = plain_run(rebuild_dir, "host", name, left_align, kind)
    records, summary = check_run(name, left_align, out)
    check_named_expectations(name, left_align, records)
    if left_align:  # d: the same SNV lines as without the option
        assert [l.split("\t")[:5] for l in snv_lines(vcf)] == [l.split("\t")[:5] for l in snv_lines(plain_run(rebuild_dir, "host", name, False, kind)[1])]
        assert any(h["left_aligned"] for h in summary["haplotypes"]) or not (name in RC.LEFTMOST or name.startswith("random"))
    if kind == "bam":  # the two kinds of input give the same bytes
        assert plain_run(rebuild_dir, "host", name, left_align, "sam")[1:] == plain_run(rebuild_dir, "host", name, left_align, "bam")[1:]


@pytest.mark.parametrize("name", RC.NAMES)
def test_several_batches_give_the_same_bytes(name, rebuild_dir, stand_ins, tmp_path):
    kind = KINDS[RC.NAMES.index(name) % 2]
    _, vcf, summary = plain_run(rebuild_dir, "host", name, True, kind)
    for calls in (host.CALLS, la.CALLS):
        for k in calls:
            calls[k] = 0
    out = str(tmp_path / "batches")
    assert small_cli.main(argv_of(rebuild_dir, name, kind, True, out, ["--batch_bases", str(batch_limit(name))])) == 0
    assert read_outputs(out) == (vcf, summary)
    assert host.CALLS["cigar_mismatch"] >= 3


@pytest.mark.parametrize("left_align", MODES, ids=("asis", "left"))
@pytest.mark.parametrize("name", RC.COMPARED)
def test_compare_closes_the_loop(name, left_align, rebuild_dir, stand_ins):
    summary = check_compare(rebuild_dir, "host", name, left_align)
    assert cmp_host.CALLS["variant_replay"] >= min(2, summary["clusters"]["replayed"])   # several replay batches
