"""svim-asm-small where there is no GPU: the command with the kernels answered by the oracle
(tests/helpers.OracleBackedContext), svx_cigar_mismatch by the loop of tests/mismatch_restatement.py and svx_cover_single
by the loops of tests/callable_restatement.py — small.vcf and summary.json byte for byte against the files
tests/small_restatement.py writes.  tests/test_gpu_small.py holds the real kernels to the same expectation."""
import functools
import json
import os

import numpy as np
import pytest

from svim_asm_amd import small_cli
from tests import callable_restatement as CR, helpers, merge_restatement as MR, mismatch_restatement as MM, paf_writer as pw
from tests import sam_text_writer as stw, small_restatement as SR, tabix_reader as TR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config1")
REF = os.path.join(GOLD, "ref.fa")
HAP1, HAP2 = os.path.join(GOLD, "hap1.bam"), os.path.join(GOLD, "hap2.bam")
SEQS = MR.read_fasta(REF)
NAMES = list(SEQS)
CALLS = {"cigar_mismatch": 0, "cover_single": 0}


def restated_cigar_mismatch(self, cigar, aln_off, ref_start, bases, ref_off, ref_len, qry_off, qry_len, cap=None, n_ops=None):
    CALLS["cigar_mismatch"] += 1
    assert n_ops is None  # (no pool in HBM where there is no device)
    assert all(int(s) >= 0 for s in ref_start)  # (what the entry point refuses)
    out = MM.mismatch_batch(cigar, aln_off, ref_start, bases, ref_off, ref_len, qry_off, qry_len)
    return {k: np.array(v, dtype=np.uint8 if k.endswith("base") else np.uint32) for k, v in out.items()}


def restated_cover_single(self, start_key, end_key, list_off):
    CALLS["cover_single"] += 1
    off = [int(x) for x in list_off]
    pairs = list(zip([int(x) for x in start_key], [int(x) for x in end_key]))
    lo, hi, seg_off = CR.flat(CR.single([pairs[off[l]:off[l + 1]] for l in range(len(off) - 1)]))
    return np.array(lo, dtype=np.uint64), np.array(hi, dtype=np.uint64), np.array(seg_off, dtype=np.uint64)


@pytest.fixture
def device(monkeypatch):
    monkeypatch.setattr(helpers.OracleBackedContext, "cigar_mismatch", restated_cigar_mismatch, raising=False)
    monkeypatch.setattr(helpers.OracleBackedContext, "cover_single", restated_cover_single, raising=False)
    monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", "0")
    for k in CALLS:
        CALLS[k] = 0
    return helpers.oracle_backed_device(monkeypatch)


@functools.lru_cache(maxsize=None)
def alignments(path):
    return SR.alignments_of(path)


@functools.lru_cache(maxsize=None)
def golden_expectation(haploid=False, sample="Sample"):
    """(small.vcf text, summary.json text, summary) of the fixture by the restatement."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        haps = [alignments(HAP1)] + ([] if haploid else [alignments(HAP2)])
        _, _, summary = SR.write(d, haps, SEQS, NAMES, sample=sample)
        return open(os.path.join(d, "small.vcf")).read(), open(os.path.join(d, "summary.json")).read(), summary


def check_outputs(out_dir, expected):
    assert sorted(os.listdir(out_dir)) == ["small.vcf", "summary.json"]
    assert open(os.path.join(out_dir, "small.vcf")).read() == expected[0]
    assert open(os.path.join(out_dir, "summary.json")).read() == expected[1]


# ------------------------------------------------------------------------------ the fixture
def test_golden_diploid_equals_the_restatement(tmp_path, device):
    expected = golden_expectation()
    assert small_cli.main([str(tmp_path / "out"), REF, HAP1, HAP2]) == 0
    check_outputs(str(tmp_path / "out"), expected)
    summary = expected[2]
    # the issue's counts of the fixture, by a plain loop over the pure-Python reader
    assert [h["mismatches"] for h in summary["haplotypes"]] == [325, 340]
    assert [h["small_indels"] for h in summary["haplotypes"]] == [192, 202]
    assert [h["records_used"] for h in summary["haplotypes"]] == [34, 38]
    assert summary["records"] == sum(summary["by_type"].values()) == sum(summary["by_genotype"].values()) > 500
    assert all(summary["by_type"][k] > 0 for k in ("SNV", "INS", "DEL"))
    # (the fixture's haplotypes were mutated independently: no small variant is shared, 1|1 does not occur)
    assert {"1|0", "0|1", "1|.", ".|1"} == set(summary["by_genotype"])
    # one mismatch call per haplotype (one batch each), ONE single-coverage call for both
    assert CALLS == {"cigar_mismatch": 2, "cover_single": 1}


def test_golden_haploid(tmp_path, device):
    expected = golden_expectation(haploid=True, sample="only")
    assert small_cli.main([str(tmp_path / "out"), REF, HAP1, "--sample", "only"]) == 0
    check_outputs(str(tmp_path / "out"), expected)
    assert set(expected[2]["by_genotype"]) == {"1"}
    assert CALLS == {"cigar_mismatch": 1, "cover_single": 1}


def test_golden_from_sam_and_paf(tmp_path, device):
    sam = stw.bam_as_sam(HAP1, str(tmp_path / "h1.sam"), so="unsorted", shuffle_seed=11)
    paf, query = pw.bam_as_paf(HAP2, str(tmp_path / "h2.paf"), str(tmp_path / "q2.fa"), shuffle_seed=12)
    assert small_cli.main([str(tmp_path / "out"), REF, sam, paf, "--query2", query]) == 0
    check_outputs(str(tmp_path / "out"), golden_expectation())
    assert CALLS["cover_single"] == 1


def test_several_batches_give_the_same_files(tmp_path, device):
    assert small_cli.main([str(tmp_path / "out"), REF, HAP1, HAP2, "--batch_bases", "100000"]) == 0
    check_outputs(str(tmp_path / "out"), golden_expectation())
    assert CALLS["cigar_mismatch"] > 4 and CALLS["cover_single"] == 1


def test_bgzip_output_reads_back(tmp_path, device):
    assert small_cli.main([str(tmp_path / "out"), REF, HAP1, HAP2, "--bgzip_output"]) == 0
    out = str(tmp_path / "out")
    assert sorted(os.listdir(out)) == ["small.vcf.gz", "small.vcf.gz.tbi", "summary.json"]
    text = golden_expectation()[0].encode()
    blob = open(os.path.join(out, "small.vcf.gz"), "rb").read()
    TR.check_bgzf(blob, text)
    reader = TR.Reader(blob, open(os.path.join(out, "small.vcf.gz.tbi"), "rb").read())
    for name, beg, end in (("chr1", 0, 1 << 29), ("chr2", 100000, 300000), ("chr10", 0, 5000)):
        assert reader.query(name, beg, end) == TR.brute(text, name, beg, end)
    assert len(reader.query("chr1", 0, 1 << 29)) > 10


# ------------------------------------------------------------------------------ made-up records
def build(contig, start, script, snvs=()):
    """An alignment (contig, start, ops, SEQ) from a script of (op, length or bases): M copies the reference (with the bases
    of `snvs`, {reference position: base}), I and S take the given bases, D and N skip."""
    ref, snvs = SEQS[contig], dict(snvs)
    ops, seq, r = [], [], start
    for op, arg in script:
        if op in (1, 4):
            ops.append((op, len(arg)))
            seq.append(arg)
        else:
            ops.append((op, arg))
            if op == 0:
                seq.append("".join(snvs.get(p, ref[p]) for p in range(r, r + arg)))
            r += arg
    return contig, start, ops, "".join(seq)


def sam_of(path, alignments, no_sequence=()):
    lines = []
    for k, (contig, start, ops, seq) in enumerate(alignments):
        cigar = stw.cigar_string([(n << 4) | op for op, n in ops])
        lines.append(stw.record_line("q%d" % k, 0, contig, start, 60, cigar, None if k in no_sequence else seq))
    return stw.write_sam(path, NAMES, [len(SEQS[n]) for n in NAMES], lines)


def other(base):
    return {"A": "C", "C": "G", "G": "T", "T": "A"}[base.upper()]


def made_up():
    """Two haplotypes on chr1: every drop reason on haplotype 1; on haplotype 2 a clean alignment over haplotype 1's first
    events (0), an allele that overlaps one of them (. on both sides), and nothing over the rest (.)."""
    ref = SEQS["chr1"]
    snv = {1040: other(ref[1040]), 1060: other(ref[1060]), 1300: other(ref[1300])}
    h1 = [build("chr1", 1000, [(4, "ACG"), (0, 100), (2, 3), (0, 100), (1, "ACGTA"), (0, 200)], snv),     # SNVs, a DEL, an INS
          build("chr1", 3000, [(4, "AC"), (1, "TTT"), (0, 100)]),                                          # no_anchor
          build("chr1", 4000, [(0, 50), (1, "ACNGT"), (0, 50)]),                                           # ambiguous_base
          build("chr1", 5000, [(0, 300)], {5250: other(ref[5250]), 5010: other(ref[5010])}),               # 5250: multiply_covered
          build("chr1", 5200, [(0, 300)]),
          build("chr1", 7000, [(0, 100)], {7050: other(ref[7050])}),                                       # no_sequence
          build("chr1", 8000, [(0, 50), (3, 20), (0, 50)], {8010: other(ref[8010])}),                      # spliced
          build("chr1", 9000, [(0, 100)], {9050: other(ref[9050])})]                                       # haplotype 2 is not there
    h2 = [build("chr1", 900, [(0, 398), (2, 5), (0, 300)], {1060: snv[1060]}),  # the SNV at 1060 too; reference over 1040 and the indels; a DEL [1298, 1303) over the SNV at 1300
          build("chr1", 4900, [(0, 200)])]
    return h1, h2


def test_made_up_records(tmp_path, device):
    h1, h2 = made_up()
    sam1, sam2 = sam_of(str(tmp_path / "h1.sam"), h1, no_sequence=(5,)), sam_of(str(tmp_path / "h2.sam"), h2)
    h1[5] = h1[5][:3] + ("",)
    records, texts, summary = SR.write(str(tmp_path / "expected"), [h1, h2], SEQS, NAMES)
    assert small_cli.main([str(tmp_path / "out"), REF, sam1, sam2]) == 0
    for name in ("small.vcf", "summary.json"):
        assert open(str(tmp_path / "out" / name)).read() == open(str(tmp_path / "expected" / name)).read()
    c = summary["haplotypes"][0]
    assert (c["no_sequence"], c["spliced"], c["no_anchor"], c["ambiguous_base"]) == (1, 1, 1, 1) and c["multiply_covered"] == 1
    gt = {(r[1], r[4]): t for r, t in zip(records, texts)}
    ref = SEQS["chr1"]
    assert gt[(1041, "SNV")] == "1|0"                       # haplotype 2 lies over it with the reference's base
    assert gt[(1061, "SNV")] == "1|1"                       # both carry it
    assert gt[(1100, "DEL")] == "1|0" and gt[(1203, "INS")] == "1|0"
    assert gt[(1301, "SNV")] == "1|." and gt[(1298, "DEL")] == ".|1"  # overlapping alleles: neither is the other's reference
    assert gt[(5011, "SNV")] == "1|0"
    assert (5251, "SNV") not in gt and (7051, "SNV") not in gt and (8011, "SNV") not in gt
    assert gt[(9051, "SNV")] == "1|."                       # no alignment of haplotype 2 there
    assert [r for r in records if r[1] == 1100][0][2:4] == (ref[1099:1103].upper(), ref[1099].upper())
    assert [r for r in records if r[1] == 1203][0][2:4] == (ref[1202].upper(), ref[1202].upper() + "ACGTA")


# ------------------------------------------------------------------------------ refusals and exit statuses
def test_argument_errors_exit_2_before_any_work(tmp_path, capsys):
    out = str(tmp_path / "out")
    for extra in (["--min_sv_size", "0"], ["--batch_bases", "0"], ["--min_mapq", "-1"], ["--sample", "a\tb"]):
        assert small_cli.main([out, REF, HAP1] + extra) == 2
    assert small_cli.main([out, REF, str(tmp_path / "none.bam")]) == 2
    assert small_cli.main([out, REF, HAP1, "--query2", REF]) == 2
    assert "svim-asm-small:" in capsys.readouterr().err and not os.path.exists(out)


def test_unusable_genome_exit_1(tmp_path, device, caplog):
    out = str(tmp_path / "out")
    assert small_cli.main([out, str(tmp_path / "none.fa"), HAP1]) == 1
    small = str(tmp_path / "small.fa")  # a genome without one of the alignments' contigs
    pw.write_fasta(small, ["chr1"], [SEQS["chr1"]])
    assert small_cli.main([out, small, HAP1]) == 1
    assert any("genome does not have" in r.getMessage() for r in caplog.records)
    assert not os.path.exists(os.path.join(out, "small.vcf"))


def test_the_command_line_tool_exists():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "svim-asm-small")
    assert os.access(path, os.X_OK) and "small_cli" in open(path).read()
