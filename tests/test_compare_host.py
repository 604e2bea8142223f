"""svim-asm-compare where there is no GPU: the kernels answered by the oracle
(tests/helpers.OracleBackedContext), the matching by tests/match_restatement.py and the interval containment by plain
loops.  The summary's integers, the four VCFs byte for byte and matches.tsv must equal the restatement's
(tests/compare_restatement.py); so must, element for element, the distance matrices handed to match_greedy_batch — an
eligible cell the textbook distance, an ineligible one 0xFFFFFFFF on both sides.  tests/test_gpu_compare.py runs `check`
with the device in place of the stand-ins."""
import argparse
import json
import logging
import os

import numpy as np
import pytest

from svim_asm_amd import SVIM_COMPARE, compare_cli
from svim_asm_amd.fasta import FastaFile
from tests import compare_cases as K, compare_restatement as R, helpers, match_restatement

GOLD = K.GOLD
CASES = K.synthetic_cases()


def restated_match(self, dist, n_base, n_comp):
    mb, mc = match_restatement.match_batch(np.asarray(dist).ravel().tolist(), n_base, n_comp)
    return np.array(mb, np.uint32), np.array(mc, np.uint32)


def restated_cover_query(self, start_key, end_key, list_off, q_lo, q_hi):
    out = np.zeros((len(list_off) - 1, len(q_lo)), np.uint8)
    for l in range(len(list_off) - 1):
        for q in range(len(q_lo)):
            out[l, q] = any(int(start_key[i]) <= int(q_lo[q]) and int(end_key[i]) >= int(q_hi[q]) for i in range(int(list_off[l]), int(list_off[l + 1])))
    return out


class Recording(object):
    """A context that notes what goes into match_greedy_batch and how many distance jobs were asked for."""

    def __init__(self, ctx):
        self._ctx, self.matched, self.jobs = ctx, [], 0

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def match_greedy_batch(self, dist, n_base, n_comp):
        self.matched.append((np.array(dist, np.uint32).ravel().tolist(), [int(x) for x in n_base], [int(x) for x in n_comp]))
        return self._ctx.match_greedy_batch(dist, n_base, n_comp)

    def haplotype_distance_batch_mixed(self, pool, pieces, k_max):
        self.jobs += len(k_max)
        return self._ctx.haplotype_distance_batch_mixed(pool, pieces, k_max)


@pytest.fixture
def device(monkeypatch):
    monkeypatch.setattr(helpers.OracleBackedContext, "match_greedy_batch", restated_match, raising=False)
    monkeypatch.setattr(helpers.OracleBackedContext, "cover_query", restated_cover_query, raising=False)
    return helpers.oracle_backed_device(monkeypatch)


def check(ctx, base_path, comp_path, options, out_dir, bed=None, key=None, compiled_distance=None):
    """Run the comparison on `ctx` and hold everything it writes, and what it hands to the matching, to the restatement.
    Returns (summary, restatement's result, the recording context)."""
    rec = Recording(ctx)
    opts = argparse.Namespace(**options)
    reference = FastaFile(K.REF)
    try:
        summary = SVIM_COMPARE.compare(base_path, comp_path, reference, opts, str(out_dir), ctx=rec)
    finally:
        reference.close()
    base, comp, want, matrices = K.restated(base_path, comp_path, options, bed=bed, key=key, compiled_distance=compiled_distance)
    assert summary == json.load(open(os.path.join(str(out_dir), "summary.json")))
    # ---- integers; the ratios recomputed from them
    tp_b, fn, tp_c, fp = len(want["tp_base"]), len(want["fn"]), len(want["tp_comp"]), len(want["fp"])
    assert (summary["TP-base"], summary["FN"], summary["TP-comp"], summary["FP"]) == (tp_b, fn, tp_c, fp)
    assert summary["precision"] == (None if tp_c + fp == 0 else tp_c / (tp_c + fp))
    assert summary["recall"] == (None if tp_b + fn == 0 else tp_b / (tp_b + fn))
    p, r = summary["precision"], summary["recall"]
    assert summary["f1"] == (None if p is None or r is None or p + r == 0 else 2 * p * r / (p + r))
    for name in ("DEL", "INS"):
        t = summary["by_type"][name]
        n = {k: sum(1 for x in want[k] if x["class"] == name) for k in ("tp_base", "fn", "tp_comp", "fp")}
        assert (t["TP-base"], t["FN"], t["TP-comp"], t["FP"]) == (n["tp_base"], n["fn"], n["tp_comp"], n["fp"])
        assert t["precision"] == (None if n["tp_comp"] + n["fp"] == 0 else n["tp_comp"] / (n["tp_comp"] + n["fp"]))
        assert t["recall"] == (None if n["tp_base"] + n["fn"] == 0 else n["tp_base"] / (n["tp_base"] + n["fn"]))
    assert (summary["gt_compared"], summary["gt_concordant"]) == (want["gt_compared"], want["gt_concordant"])
    assert summary["gt_concordance"] == (None if not want["gt_compared"] else want["gt_concordant"] / want["gt_compared"])
    assert summary["base"] == want["base"] and summary["comp"] == want["comp"]
    assert summary["partitions_over_cap"] == want["partitions_over_cap"]
    # ---- the files, byte for byte
    for name, parsed, rows in (("tp-base.vcf", base, want["tp_base"]), ("fn.vcf", base, want["fn"]), ("tp-comp.vcf", comp, want["tp_comp"]),
                               ("fp.vcf", comp, want["fp"])):
        assert open(os.path.join(str(out_dir), name), "rb").read() == R.vcf_bytes(parsed, rows), name
    assert open(os.path.join(str(out_dir), "matches.tsv")).read() == R.matches_tsv(want)
    # ---- the matrices handed to the matching
    assert len(rec.matched) <= 1
    got = rec.matched[0] if rec.matched else ([], [], [])
    assert got[1] == [m[0] for m in matrices] and got[2] == [m[1] for m in matrices]
    assert got[0] == [d for m in matrices for d in m[2]]
    return summary, want, rec


def run_case(ctx, name, tmp_path, gz=False):
    case = CASES[name]
    base, comp, bed = K.write(case, tmp_path / "in", gz=gz)
    options = K.options_of(case)
    options["include_bed"] = bed
    return check(ctx, base, comp, options, tmp_path / "out", bed=case.get("bed"))


# ------------------------------------------------------------------------------------------------- golden files
def golden(ctx, base_name, comp_name, tmp_path, **extra):
    options = dict(K.DEFAULTS, **extra)
    return check(ctx, os.path.join(GOLD, base_name), os.path.join(GOLD, comp_name), options, tmp_path / "out",
                 key=(base_name, comp_name, tuple(sorted(extra.items()))))


def test_a_file_against_itself(device, tmp_path):
    summary, want, _ = golden(device, "diploid_default.vcf", "diploid_default.vcf", tmp_path, comp_min_sv_size=50)
    assert summary["FP"] == 0 and summary["FN"] == 0 and summary["TP-base"] == summary["base"]["compared"] > 50
    assert summary["precision"] == 1.0 and summary["recall"] == 1.0 and summary["f1"] == 1.0 and summary["gt_concordance"] == 1.0
    assert all(d == 0 for _, _, d in want["matches"])


@pytest.mark.parametrize("comp", ["diploid_tolerances.vcf", "haploid_default.vcf"])
def test_golden_call_sets_against_each_other(device, tmp_path, comp):
    summary, _, _ = golden(device, "diploid_default.vcf", comp, tmp_path)
    assert summary["TP-base"] > 20 and summary["TP-base"] == summary["TP-comp"]


# ------------------------------------------------------------------------------------------------- synthetic pairs
def test_same_deletion_at_two_offsets_in_a_tandem_repeat(device, tmp_path):
    summary, want, _ = run_case(device, "tandem_shift", tmp_path)
    assert (summary["TP-base"], summary["FN"], summary["FP"]) == (1, 0, 0) and want["matches"][0][2] == 0
    assert summary["gt_concordance"] == 0.0  # 1/1 against 0/1


def test_two_base_against_one_comp(device, tmp_path):
    summary, want, rec = run_case(device, "two_base_one_comp", tmp_path)
    assert (summary["TP-base"], summary["FN"], summary["TP-comp"], summary["FP"]) == (1, 1, 1, 0)
    assert [m[0]["id"] for m in want["matches"]] == ["b2"] and rec.matched[0][1:] == ([2], [1])


def test_genotypes_and_symbolic_against_resolved(device, tmp_path):
    summary, want, _ = run_case(device, "genotypes", tmp_path)
    assert summary["TP-base"] == 4 and summary["FP"] == 0
    assert (summary["gt_compared"], summary["gt_concordant"]) == (4, 3)  # only the het against the hom call differs
    text = open(tmp_path / "out" / "matches.tsv").read().splitlines()
    assert text[1].split("\t")[4:] == ["DEL", "0", "0/1", "1/1"] and text[2].split("\t")[4:] == ["INS", "6", "1/1", "1/1"]


def test_both_sides_of_the_limits(device, tmp_path):
    at, _, _ = run_case(device, "at_the_limit", tmp_path / "a")
    over, _, rec = run_case(device, "over_the_limit", tmp_path / "b")
    assert (at["TP-base"], at["FN"], at["FP"]) == (1, 0, 0) and (over["TP-base"], over["FN"], over["FP"]) == (0, 1, 1)
    assert rec.matched[0][0] == [match_restatement.NONE]
    rel, _, _ = run_case(device, "relative_limit", tmp_path / "c")
    off, _, _ = run_case(device, "relative_limit_off", tmp_path / "d")
    assert (rel["TP-base"], rel["FN"]) == (1, 1) and (off["TP-base"], off["FN"]) == (0, 2)


def test_a_size_difference_skips_the_job(device, tmp_path):
    """500 against 60 bases can never be within 200 edits: two of the four pairs get no distance job, and the matrix
    holds 0xFFFFFFFF there as the restatement's does after computing them."""
    summary, _, rec = run_case(device, "size_skip", tmp_path)
    assert rec.jobs == 2 and rec.matched[0][1:] == ([2], [2])
    assert sum(1 for d in rec.matched[0][0] if d == match_restatement.NONE) >= 2 and summary["TP-base"] == 2


def test_records_at_the_size_limits(device, tmp_path):
    summary, want, _ = run_case(device, "sizes", tmp_path)
    assert summary["base"]["size_filtered"] == 1 and summary["comp"]["size_filtered"] == 1
    # b49 is left out, c49 and c30 are compared and find nobody; the 30-base insertion is within 200 edits of the 50-base one
    assert [r["id"] for r in want["fn"]] == [] and sorted(r["id"] for r in want["fp"]) == ["c30", "c49"]
    assert [(b["id"], c["id"]) for b, c, _ in want["matches"]] == [("b50", "c50"), ("bi50", "ci30")]


def test_include_bed_is_one_line_never_the_union_of_two(device, tmp_path):
    summary, want, _ = run_case(device, "bed", tmp_path)
    assert [r["id"] for r in want["tp_base"]] == ["touch_lo", "touch_hi", "inside", "ins_on_the_seam", "ins_at_hi", "start_zero"]
    assert summary["base"]["out_of_regions"] == 5 and summary["base"]["compared"] == 6 and summary["FN"] == 0


def test_a_partition_over_the_cap_is_left_unmatched(device, tmp_path, caplog):
    with caplog.at_level(logging.WARNING):
        summary, _, rec = run_case(device, "over_cap", tmp_path / "a")
    warnings = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert warnings == ["Partition of 7 records (more than --compare_max_partition 6) left unmatched: DEL chr2:70030-70120"]
    assert summary["partitions_over_cap"] == 1 and summary["base"]["over_cap"] == 4 and summary["comp"]["over_cap"] == 3
    assert (summary["TP-base"], summary["FN"], summary["FP"]) == (1, 4, 3) and rec.matched[0][1:] == ([1], [1])
    under, _, _ = run_case(device, "under_cap", tmp_path / "b")
    assert under["partitions_over_cap"] == 0 and under["TP-base"] == 4 and under["FN"] == 1


def test_classes_that_are_counted_not_compared(device, tmp_path):
    summary, _, _ = run_case(device, "not_compared", tmp_path)
    b = summary["base"]
    assert (b["records"], b["compared"], b["complex"], b["other"], b["unresolved"], b["multiallelic"], b["not_carried"], b["filtered"]) == \
        (7, 1, 1, 1, 1, 1, 1, 1)
    assert (summary["TP-base"], summary["FP"]) == (1, 1)


def test_bgzf_inputs_give_the_same_files(device, tmp_path):
    plain, _, _ = run_case(device, "genotypes", tmp_path / "plain")
    packed, _, _ = run_case(device, "genotypes", tmp_path / "gz", gz=True)
    assert plain == packed
    for name in ("tp-base.vcf", "fn.vcf", "tp-comp.vcf", "fp.vcf", "matches.tsv"):
        assert open(tmp_path / "plain" / "out" / name, "rb").read() == open(tmp_path / "gz" / "out" / name, "rb").read()


def test_empty_sides(device, tmp_path):
    case = dict(base=[K.deletion("chr1", 5000, 5100, "b1")], comp=[])
    base, comp, _ = K.write(case, tmp_path / "in")
    summary, _, rec = check(device, base, comp, K.options_of(case), tmp_path / "out")
    assert (summary["TP-base"], summary["FN"], summary["FP"]) == (0, 1, 0) and summary["precision"] is None and summary["recall"] == 0.0
    assert summary["f1"] is None and summary["gt_concordance"] is None and not rec.matched


# ------------------------------------------------------------------------------------------------- the command
def test_command_writes_the_files_and_names_what_it_refuses(device, tmp_path, capsys, caplog):
    case = CASES["two_base_one_comp"]
    base, comp, _ = K.write(case, tmp_path / "in")
    out = tmp_path / "out"
    assert compare_cli.main([str(out), K.REF, base, comp]) == 0
    assert sorted(os.listdir(out)) == ["fn.vcf", "fp.vcf", "matches.tsv", "summary.json", "tp-base.vcf", "tp-comp.vcf"]
    assert json.load(open(out / "summary.json"))["TP-base"] == 1
    # argument errors: status 2 before any work
    for argv, what in (([str(tmp_path / "o2"), K.REF, base, str(tmp_path / "missing.vcf")], "no such file"),
                       ([str(tmp_path / "o2"), K.REF, base, comp, "--max_edit_distance", "-1"], "--max_edit_distance"),
                       ([str(tmp_path / "o2"), K.REF, base, comp, "--max_relative_distance", "1.5"], "--max_relative_distance"),
                       ([str(tmp_path / "o2"), K.REF, base, comp, "--compare_max_partition", "1"], "--compare_max_partition")):
        assert compare_cli.main(argv) == 2
        assert what in capsys.readouterr().err and not os.path.exists(tmp_path / "o2")
    # contigs that are not in the genome: status 1 and a message
    alien = tmp_path / "alien.vcf"
    alien.write_text(K.HEADER + "chrZ\t100\tx\tACGT\tA\t.\tPASS\t.\tGT\t1/1\n")
    with caplog.at_level(logging.ERROR):
        assert compare_cli.main([str(tmp_path / "o3"), K.REF, base, str(alien)]) == 1
    assert any("alien.vcf: line 4: the contig 'chrZ' is not in the genome's index" in r.getMessage() for r in caplog.records)
    with caplog.at_level(logging.ERROR):
        assert compare_cli.main([str(tmp_path / "o4"), K.REF, base, comp, "--comp_sample", "NOBODY"]) == 1
    assert any("no sample 'NOBODY'" in r.getMessage() for r in caplog.records)


# ------------------------------------------------------------------------------------------------- the BED itself
def test_bed_header_lines_and_contigs_that_begin_like_them(tmp_path):
    """`track ...` and `browser ...` lines of a BED are headers; a contig called track1 or browserX is a contig."""
    p = tmp_path / "r.bed"
    p.write_text("browser position chr1:1-100\ntrack name=x description=\"y\"\n# a comment\n\nchr1\t50\t60\ntrack1\t5\t9\nbrowserX\t0\t7\r\nchr1\t10\t20\n")
    lo, hi = SVIM_COMPARE.read_bed(str(p), ["track1", "browserX", "chr1"])
    assert lo.tolist() == [5, (1 << 32) | 0, (2 << 32) | 10, (2 << 32) | 50] and hi.tolist() == [9, (1 << 32) | 7, (2 << 32) | 20, (2 << 32) | 60]
    for bad, line in (("chr1\t9\n", 1), ("chrNo\t1\t2\n", 1), ("chr1\t1\t2\nchr1\t7\t3\n", 2), ("chr1\tx\t3\n", 1)):
        p.write_text(bad)
        with pytest.raises(ValueError, match="r.bed: line %d" % line):
            SVIM_COMPARE.read_bed(str(p), ["chr1"])


def test_an_empty_bed_holds_nothing(device, tmp_path):
    """A BED without lines: every record is out of the regions, nothing is compared and no kernel is asked anything."""
    case = CASES["two_base_one_comp"]
    base, comp, _ = K.write(case, tmp_path / "in")
    bed = tmp_path / "empty.bed"
    bed.write_text("track name=nothing\n")
    options = K.options_of(case)
    options["include_bed"] = str(bed)
    summary, _, rec = check(device, base, comp, options, tmp_path / "out", bed=[])
    assert (summary["TP-base"], summary["FN"], summary["FP"]) == (0, 0, 0) and not rec.matched and rec.jobs == 0
    assert summary["base"]["out_of_regions"] == 2 and summary["comp"]["out_of_regions"] == 1 and summary["recall"] is None
