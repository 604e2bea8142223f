"""svim-asm-small --left_align where there is no GPU: the command with the device answered as in
tests/test_small_host.py and svx_indel_shift by the loop of tests/shift_restatement.py — small.vcf byte for byte against
what tests/small_restatement.py writes for the alignments with every small gap MOVED IN THE CIGAR
(shift_restatement.rewrite), summary.json equal to that run's plus the two new counts.  tests/test_gpu_small_leftalign.py
holds the real kernels to the same expectation."""
import functools
import json
import os
import re
import tempfile

import numpy as np
import pytest

from svim_asm_amd import small_cli
from tests import helpers, paf_writer as pw, sam_text_writer as stw, shift_restatement as SH, small_restatement as SR
from tests import test_small_host as host
from tests.test_small_host import device  # noqa: F401  (the fixture that answers the other device calls)

CALLS = {"indel_shift": 0}
NEW_KEYS = ("left_aligned", "shifted_bases")
CHR1 = host.SEQS["chr1"]
# homopolymer runs of six bases or more on chr1 of the fixture genome, maximal and far from one another
RUNS = []
for _m in re.finditer(r"A{6,}|C{6,}|G{6,}|T{6,}", CHR1.upper()):
    if _m.start() > 1000 and (not RUNS or _m.start() > RUNS[-1][1] + 2000):
        RUNS.append((_m.start(), _m.end()))


def restated_indel_shift(self, bases, ref_off, ref_len, qry_off, qry_len, ref_start, aln, ref_pos, qry_pos, length, type, limit):
    CALLS["indel_shift"] += 1
    assert all(int(x) in (SH.INS, SH.DEL) for x in type) and all(int(n) > 0 for n in length)  # (what the entry point refuses)
    return np.array(SH.shift_batch(bases, ref_off, ref_len, qry_off, qry_len, ref_start, aln, ref_pos, qry_pos, length, type, limit), dtype=np.uint32)


@pytest.fixture
def shifting_device(monkeypatch, device):  # noqa: F811
    monkeypatch.setattr(helpers.OracleBackedContext, "indel_shift", restated_indel_shift, raising=False)
    CALLS["indel_shift"] = 0
    return device


def expectation_of(haplotypes, sample="Sample", min_sv_size=40):
    """(small.vcf text, summary, records, genotype texts) of the restatement on the rewritten alignments; the summary with
    the two new counts."""
    rewritten = [SH.rewrite(h, host.SEQS, min_sv_size) for h in haplotypes]
    with tempfile.TemporaryDirectory() as d:
        records, texts, summary = SR.write(d, [r for r, _ in rewritten], host.SEQS, host.NAMES, sample=sample, min_sv_size=min_sv_size)
        text = open(os.path.join(d, "small.vcf")).read()
    for counts, (_, moved) in zip(summary["haplotypes"], rewritten):
        counts["left_aligned"], counts["shifted_bases"] = len(moved), sum(moved)
    return text, summary, records, texts


@functools.lru_cache(maxsize=None)
def golden_left_aligned(haploid=False, sample="Sample"):
    return expectation_of([host.alignments(host.HAP1)] + ([] if haploid else [host.alignments(host.HAP2)]), sample=sample)


def check_outputs(out_dir, expected):
    assert sorted(os.listdir(out_dir)) == ["small.vcf", "summary.json"]
    assert open(os.path.join(out_dir, "small.vcf")).read() == expected[0]
    text = open(os.path.join(out_dir, "summary.json")).read()
    summary = json.loads(text)
    assert summary == expected[1]
    assert all(tuple(h) == SR.COUNTS + NEW_KEYS for h in summary["haplotypes"])  # (the new keys behind the existing ones)
    without = dict(summary, haplotypes=[{k: v for k, v in h.items() if k not in NEW_KEYS} for h in summary["haplotypes"]])
    assert json.dumps(without, indent=1) + "\n" == json.dumps(dict(expected[1], haplotypes=without["haplotypes"]), indent=1) + "\n"
    return summary


# ------------------------------------------------------------------------------ the fixture
def test_golden_diploid_left_aligned(tmp_path, shifting_device):
    expected = golden_left_aligned()
    assert small_cli.main([str(tmp_path / "out"), host.REF, host.HAP1, host.HAP2, "--left_align"]) == 0
    summary = check_outputs(str(tmp_path / "out"), expected)
    # the fixture's figures (tests/test_shift_restatement.py has them from the loop alone)
    assert [(h["left_aligned"], h["shifted_bases"], h["small_indels"]) for h in summary["haplotypes"]] == [(52, 66, 192), (44, 61, 202)]
    assert expected[0] != host.golden_expectation()[0]  # (the option changes the file)
    # the same SNVs as without the option: a passed column is a match before and after
    snv = lambda text: [l for l in text.splitlines() if not l.startswith("#") and len(l.split("\t")[3]) == len(l.split("\t")[4]) == 1]
    assert [l.split("\t")[:5] for l in snv(expected[0])] == [l.split("\t")[:5] for l in snv(host.golden_expectation()[0])]
    assert CALLS["indel_shift"] == 2 and host.CALLS["cigar_mismatch"] == 2  # one call per haplotype: one batch each


def test_golden_haploid_left_aligned(tmp_path, shifting_device):
    assert small_cli.main([str(tmp_path / "out"), host.REF, host.HAP1, "--sample", "only", "--left_align"]) == 0
    check_outputs(str(tmp_path / "out"), golden_left_aligned(haploid=True, sample="only"))


def test_golden_from_sam_and_paf_left_aligned(tmp_path, shifting_device):
    sam = stw.bam_as_sam(host.HAP1, str(tmp_path / "h1.sam"), so="unsorted", shuffle_seed=11)
    paf, query = pw.bam_as_paf(host.HAP2, str(tmp_path / "h2.paf"), str(tmp_path / "q2.fa"), shuffle_seed=12)
    assert small_cli.main([str(tmp_path / "out"), host.REF, sam, paf, "--query2", query, "--left_align"]) == 0
    check_outputs(str(tmp_path / "out"), golden_left_aligned())


def test_several_batches_left_aligned(tmp_path, shifting_device):
    assert small_cli.main([str(tmp_path / "out"), host.REF, host.HAP1, host.HAP2, "--batch_bases", "100000", "--left_align"]) == 0
    check_outputs(str(tmp_path / "out"), golden_left_aligned())
    assert 4 < CALLS["indel_shift"] <= host.CALLS["cigar_mismatch"]  # (a batch without small gaps makes no call)


def test_without_the_option_nothing_changes_and_the_entry_is_not_called(tmp_path, device, monkeypatch):  # noqa: F811
    def never(self, *args):
        raise AssertionError("indel_shift called without --left_align")
    monkeypatch.setattr(helpers.OracleBackedContext, "indel_shift", never, raising=False)
    assert small_cli.main([str(tmp_path / "out"), host.REF, host.HAP1, host.HAP2]) == 0
    host.check_outputs(str(tmp_path / "out"), host.golden_expectation())
    assert small_cli.main([str(tmp_path / "b"), host.REF, host.HAP1, host.HAP2, "--batch_bases", "100000"]) == 0
    host.check_outputs(str(tmp_path / "b"), host.golden_expectation())


def test_help_lists_the_option(capsys):
    with pytest.raises(SystemExit):
        small_cli.main(["--help"])
    assert "--left_align" in capsys.readouterr().out


# ------------------------------------------------------------------------------ made-up records in the fixture's repeats
def run_command(tmp_path, name, h1, h2, extra=()):
    sam1, sam2 = host.sam_of(str(tmp_path / (name + "1.sam")), h1), host.sam_of(str(tmp_path / (name + "2.sam")), h2)
    out = str(tmp_path / name)
    assert small_cli.main([out, host.REF, sam1, sam2] + list(extra)) == 0
    lines = [l.split("\t") for l in open(os.path.join(out, "small.vcf")).read().splitlines() if not l.startswith("#")]
    return out, [(int(l[1]), l[3], l[4], l[9]) for l in lines], json.load(open(os.path.join(out, "summary.json")))


def repeat_pair():
    """Both haplotypes delete one base of the run RUNS[0] and insert one more base of the run RUNS[1]: haplotype 1 places
    the gap at the run's right end, haplotype 2 in its middle."""
    (ds, de), (is_, ie) = RUNS[0], RUNS[1]
    base = CHR1[is_].upper()
    h1 = [host.build("chr1", ds - 100, [(0, de - 1 - (ds - 100)), (2, 1), (0, 100)]),
          host.build("chr1", is_ - 100, [(0, ie - (is_ - 100)), (1, base), (0, 100)])]
    h2 = [host.build("chr1", ds - 100, [(0, ds + 2 - (ds - 100)), (2, 1), (0, de - (ds + 3) + 100)]),
          host.build("chr1", is_ - 100, [(0, is_ + 3 - (is_ - 100)), (1, base), (0, ie - (is_ + 3) + 100)])]
    return h1, h2


def test_the_same_indel_placed_differently_becomes_one_record(tmp_path, shifting_device):
    assert len(RUNS) >= 4
    (ds, de), (is_, ie) = RUNS[0], RUNS[1]
    h1, h2 = repeat_pair()
    _, plain, _ = run_command(tmp_path, "plain", h1, h2)
    assert len(plain) == 4 and "1|1" not in [r[3] for r in plain]  # two records per indel
    assert sorted(r[0] for r in plain) == sorted([de - 1, ds + 2, ie, is_ + 3]) and CALLS["indel_shift"] == 0
    out, moved, summary = run_command(tmp_path, "moved", h1, h2, ["--left_align"])
    base = CHR1[is_].upper()
    anchor_d, anchor_i = CHR1[ds - 1].upper(), CHR1[is_ - 1].upper()
    assert moved == [(ds, anchor_d + CHR1[ds].upper(), anchor_d, "1|1"), (is_, anchor_i, anchor_i + base, "1|1")]  # leftmost, one record each
    assert [(h["left_aligned"], h["shifted_bases"]) for h in summary["haplotypes"]] == [(2, de - 1 - ds + ie - is_), (2, 2 + 3)]
    check_outputs(out, expectation_of([h1, h2]))


def test_a_snv_inside_the_repeat_stops_the_gap_there(tmp_path, shifting_device):
    s, e = RUNS[2]
    other = host.other(CHR1[s + 2])
    script = [(0, e - 1 - (s - 100)), (2, 1), (0, 100)]
    h1, h2 = [host.build("chr1", s - 100, script, {s + 2: other})], [host.build("chr1", s - 100, script)]
    out, records, summary = run_command(tmp_path, "snv", h1, h2, ["--left_align"])
    x = CHR1[s].upper()
    # haplotype 2's gap runs the repeat down; haplotype 1's stops behind its SNV's column, which becomes its anchor: two records
    assert records == [(s, CHR1[s - 1].upper() + x, CHR1[s - 1].upper(), "0|1"), (s + 3, x, other, "1|0"), (s + 3, x + x, x, "1|0")]
    assert [h["shifted_bases"] for h in summary["haplotypes"]] == [e - 1 - (s + 3), e - 1 - s]
    check_outputs(out, expectation_of([h1, h2]))


def test_two_gaps_one_aligned_column_apart_do_not_move(tmp_path, shifting_device):
    s, e = RUNS[3]
    # the run's first base deleted (the base in front differs: it cannot move), one column, the run's third base deleted
    h1 = [host.build("chr1", s - 100, [(0, 100), (2, 1), (0, 1), (2, 1), (0, e - (s + 3) + 100)])]
    h2 = [host.build("chr1", s - 100, [(0, e - s + 200)])]
    out, records, summary = run_command(tmp_path, "near", h1, h2, ["--left_align"])
    assert [r[0] for r in records] == [s, s + 2]
    assert summary["haplotypes"][0]["small_indels"] == 2 and summary["haplotypes"][0]["left_aligned"] == 0
    check_outputs(out, expectation_of([h1, h2]))


def test_a_large_op_stays_and_bounds_its_neighbour(tmp_path, shifting_device):
    s, e = RUNS[3]
    # --min_sv_size 2: the deletion of the run's second and third base is svim-asm's — it could move one column and does
    # not —, and the deletion of the fifth base, one column behind it, stays where it is
    h1 = [host.build("chr1", s - 100, [(0, 101), (2, 2), (0, 1), (2, 1), (0, e - (s + 5) + 100)])]
    h2 = [host.build("chr1", s - 100, [(0, e - s + 200)])]
    out, records, summary = run_command(tmp_path, "large", h1, h2, ["--left_align", "--min_sv_size", "2"])
    assert [r[0] for r in records] == [s + 4] and summary["haplotypes"][0]["left_aligned"] == 0
    check_outputs(out, expectation_of([h1, h2], min_sv_size=2))
    # without the large gap in front the same deletion runs the repeat down
    h1 = [host.build("chr1", s - 100, [(0, 104), (2, 1), (0, e - (s + 5) + 100)])]
    out, records, summary = run_command(tmp_path, "free", h1, h2, ["--left_align", "--min_sv_size", "2"])
    assert [r[0] for r in records] == [s] and summary["haplotypes"][0]["shifted_bases"] == 4
