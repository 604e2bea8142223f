"""svim-asm-genotype where there is no GPU: the command with the kernels answered by the oracle
(tests/helpers.OracleBackedContext) and svx_cover_locate / svx_cigar_lift by the plain loops of tests/lift_restatement.py
— every GT, DR and DA, genotypes.vcf byte for byte and the counts of summary.json against tests/genotype_restatement.py.
tests/test_gpu_genotype.py holds the real kernels to the same expectation."""
import functools
import json
import os
import random

import numpy as np
import pytest

from svim_asm_amd import SVIM_GENOTYPE, bamio, genotype_cli, vcfin
from tests import genotype_restatement as G, helpers, lift_restatement as LR, merge_restatement as MR, paf_writer as pw, sam_text_writer as stw

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config1")
REF = os.path.join(GOLD, "ref.fa")
HAP1, HAP2 = os.path.join(GOLD, "hap1.bam"), os.path.join(GOLD, "hap2.bam")
SITES = os.path.join(GOLD, "diploid_default.vcf")
SEQS = MR.read_fasta(REF)
NAMES = list(SEQS)
CALLS = {"cover_locate": 0, "cigar_lift": 0, "mixed": 0, "slices": 0}


def restated_cover_locate(self, start_key, end_key, list_off, q_lo, q_hi):
    CALLS["cover_locate"] += 1
    off = [int(x) for x in list_off]
    pairs = list(zip([int(x) for x in start_key], [int(x) for x in end_key]))
    lists = [pairs[off[l]:off[l + 1]] for l in range(len(off) - 1)]
    queries = list(zip([int(x) for x in q_lo], [int(x) for x in q_hi]))
    return np.array(LR.locate(lists, queries), dtype=np.uint32).reshape(len(lists), len(queries))


def restated_cigar_lift(self, cigar, aln_off, ref_start, q_aln, q_ref, n_ops=None):
    CALLS["cigar_lift"] += 1
    assert n_ops is None  # (no pool in HBM where there is no device)
    query, state = LR.lift_batch(cigar, aln_off, ref_start, q_aln, q_ref)
    return np.array(query, dtype=np.uint32), np.array(state, dtype=np.uint8)


@pytest.fixture
def device(monkeypatch):
    monkeypatch.setattr(helpers.OracleBackedContext, "cover_locate", restated_cover_locate, raising=False)
    monkeypatch.setattr(helpers.OracleBackedContext, "cigar_lift", restated_cigar_lift, raising=False)
    mixed = helpers.OracleBackedContext.haplotype_distance_batch_mixed
    slices = bamio.AlignmentFile.sequence_slices_raw

    def counted_mixed(self, *a, **kw):
        CALLS["mixed"] += 1
        return mixed(self, *a, **kw)

    def counted_slices(self, *a, **kw):
        CALLS["slices"] += 1
        return slices(self, *a, **kw)
    monkeypatch.setattr(helpers.OracleBackedContext, "haplotype_distance_batch_mixed", counted_mixed)
    monkeypatch.setattr(bamio.AlignmentFile, "sequence_slices_raw", counted_slices)
    for k in CALLS:
        CALLS[k] = 0
    return helpers.oracle_backed_device(monkeypatch)


@functools.lru_cache(maxsize=None)
def alignments(path):
    return G.alignments_of(path, NAMES)


@functools.lru_cache(maxsize=None)
def golden_expectation(haploid=False):
    sites = G.sites_of(SITES)
    haps = [alignments(HAP1)] + ([] if haploid else [alignments(HAP2)])
    return sites, G.genotypes(sites, haps, SEQS)


def check_outputs(out_dir, sites_path, sites, results, n_hap, n_records, sample="Sample"):
    assert sorted(os.listdir(out_dir)) == ["genotypes.vcf", "summary.json"]
    text = open(os.path.join(out_dir, "genotypes.vcf")).read()
    got = [l.split("\t") for l in text.splitlines() if not l.startswith("#")]
    assert len(got) == len(sites)
    for rec, site, calls in zip(got, sites, results):
        assert rec[:8] == site[0][:8] and rec[8] == "GT:DR:DA" and rec[9] == G.sample_text(calls), (rec[:3], rec[9], G.sample_text(calls))
    assert text == G.expected_vcf(sites_path, sites, results, sample)
    summary = json.load(open(os.path.join(out_dir, "summary.json")))
    assert summary["records"] == n_records and summary["genotyped"] == len(sites)
    assert summary["haplotypes"] == G.expected_haplotype_counts(results, n_hap)
    return summary


def n_data_lines(path):
    return sum(1 for l in open(path) if l.strip() and not l.startswith("#"))


# ------------------------------------------------------------------------------ the fixture
def test_golden_diploid_equals_the_restatement(tmp_path, device):
    sites, results = golden_expectation()
    assert len(sites) > 40 and {"DEL", "INS"} == {s[1] for s in sites}
    assert genotype_cli.main([str(tmp_path / "out"), REF, SITES, HAP1, HAP2]) == 0
    summary = check_outputs(str(tmp_path / "out"), SITES, sites, results, 2, n_data_lines(SITES))
    # ONE call each of the locate and the distances, one lift and one slice call per haplotype
    assert CALLS == {"cover_locate": 1, "cigar_lift": 2, "mixed": 1, "slices": 2}
    texts = {"/".join(c[0] for c in calls) for calls in results}
    assert {"1/1", "1/0", "0/1"} <= texts
    # the classes that are not genotyped, and the records below --min_sv_size
    recs = vcfin.read_sites(SITES, NAMES, [len(SEQS[n]) for n in NAMES])
    assert summary["not_genotyped"] == {k: recs.counts[k] for k in ("multiallelic", "complex", "unresolved", "other", "filtered")}
    assert sum(summary["not_genotyped"].values()) + summary["genotyped"] + summary["size_filtered"] == summary["records"]
    assert summary["size_filtered"] == len(G.sites_of(SITES, min_size=0)) - len(sites) > 0
    assert not os.path.exists(tmp_path / "out" / "genotypes.vcf.tmp")


def test_golden_haploid(tmp_path, device):
    sites, results = golden_expectation(haploid=True)
    assert genotype_cli.main([str(tmp_path / "out"), REF, SITES, HAP1, "--sample", "only"]) == 0
    check_outputs(str(tmp_path / "out"), SITES, sites, results, 1, n_data_lines(SITES), sample="only")
    assert all("/" not in G.sample_text(c).split(":")[0] for c in results)
    assert CALLS == {"cover_locate": 1, "cigar_lift": 1, "mixed": 1, "slices": 1}


def test_golden_from_sam_and_paf(tmp_path, device):
    sites, results = golden_expectation()
    sam = stw.bam_as_sam(HAP1, str(tmp_path / "h1.sam"), so="unsorted", shuffle_seed=11)
    paf, query = pw.bam_as_paf(HAP2, str(tmp_path / "h2.paf"), str(tmp_path / "q2.fa"), shuffle_seed=12)
    assert genotype_cli.main([str(tmp_path / "out"), REF, SITES, sam, paf, "--query2", query]) == 0
    check_outputs(str(tmp_path / "out"), SITES, sites, results, 2, n_data_lines(SITES))


# ------------------------------------------------------------------------------ concordance with PAIR
# records whose genotype here differs from the GT PAIR wrote into diploid_default.vcf, as (ID, PAIR's, ours): explained
# one by one in DESIGN.md §3.17
DISCORDANT = [("svim_asm.INS.2", "1/1", "0/0"),    # PAIR's allele lies between two split alignments; the long alignment over it is reference
              ("svim_asm.DEL.10", "1/1", "./."),   # likewise split; haplotype 1's long alignment holds DEL.11 inside the window, none of haplotype 2 spans
              ("svim_asm.DEL.11", "1/0", "1/."),   # no alignment of haplotype 2 spans the window
              ("svim_asm.DEL.13", "1/1", "./."),   # split; haplotype 2's spanning alignment holds INS.10 inside the window, none of haplotype 1 spans
              ("svim_asm.DEL.41", "1/0", "1/1")]   # haplotype 2 holds another allele exactly at the limit (d_alt = 200)


def test_concordance_with_pair_is_pinned():
    sites, results = golden_expectation()
    discordant = []
    for site, calls in zip(sites, results):
        ours = "/".join(c[0] for c in calls)
        if ours != site[0][9].split(":")[0]:
            discordant.append((site[0][2], site[0][9].split(":")[0], ours))
    assert discordant == DISCORDANT


# ------------------------------------------------------------------------------ made-up sites
def made_up_vcf(path):
    """The header of the fixture and hand-made records: real sites with other genotype columns, a made-up deletion 200 bp
    behind a real one, an insertion with random bases, sites at both ends of a contig, a <DEL>."""
    rng = random.Random(5)
    real = G.sites_of(SITES)
    dels = [s for s in real if s[1] == "DEL" and s[0][9].startswith(("1/0", "0/1")) and 100 < s[4] - s[3] < 400]
    inss = [s for s in real if s[1] == "INS" and len(s[5]) > 500]  # (random bases of that length lie beyond the limit of 200)
    lines = [l for l in open(SITES) if l.startswith("#")]
    records = []

    def add(contig, pos1, ref, alt, info="SVTYPE=X", sample="GT\t0/0"):
        records.append("%s\t%d\tmade.%d\t%s\t%s\t.\tPASS\t%s\t%s\n" % (contig, pos1, len(records), ref, alt, info, sample))
    for s, sample in zip(dels[:3], ("GT\t0/0", "GT\t./.", "GT:CN\t0/0:1")):
        records.append("\t".join(s[0][:8] + sample.split("\t")) + "\n")
    d = dels[0]
    seq = SEQS[d[2]]
    at = d[4] + 200
    add(d[2], at + 1, seq[at:at + 61], seq[at])                                # [at + 1, at + 61): nobody carries it
    i = inss[0]
    anchor = SEQS[i[2]][i[3] - 1]
    add(i[2], i[3], anchor, anchor + "".join(rng.choice("ACGT") for _ in i[5]))  # the real insertion's place, other bases
    for contig in ("chr2", "chr10"):
        seq = SEQS[contig]
        add(contig, 11, seq[10:71], seq[10])                                     # window clamped at 0
        add(contig, len(seq) - 70, seq[len(seq) - 71:len(seq) - 10], seq[len(seq) - 71])   # ... and at the contig's end
    d = dels[1]
    add(d[2], d[3], SEQS[d[2]][d[3] - 1], "<DEL>", "SVTYPE=DEL;END=%d;SVLEN=%d" % (d[4], d[3] - d[4]), "GT\t1/1")
    with open(path, "w") as fh:
        fh.writelines(lines + records)
    return path


def test_made_up_sites(tmp_path, device):
    path = made_up_vcf(str(tmp_path / "sites.vcf"))
    sites = G.sites_of(path)
    assert len(sites) == n_data_lines(path) == 10
    haps = [alignments(HAP1), alignments(HAP2)]
    results = G.genotypes(sites, haps, SEQS)
    assert genotype_cli.main([str(tmp_path / "out"), REF, path, HAP1, HAP2]) == 0
    check_outputs(str(tmp_path / "out"), path, sites, results, 2, 10)
    gts = ["/".join(c[0] for c in calls) for calls in results]
    # 0/0 and ./. columns change nothing: the three real sites read as in the fixture — and read_vcf drops them
    real = {tuple(s[0][:5]): "/".join(c[0] for c in calls) for s, calls in zip(*golden_expectation())}
    assert gts[:3] == [real[tuple(s[0][:5])] for s in sites[:3]] and all(g in ("1/0", "0/1") for g in gts[:3])
    lengths = [len(SEQS[n]) for n in NAMES]
    assert vcfin.read_vcf(path, NAMES, lengths).counts["not_carried"] == 9  # (all but the <DEL>, which says 1/1)
    assert vcfin.read_sites(path, NAMES, lengths).counts["not_carried"] == 0
    # the made-up deletion beside a real one: reference on a haplotype that spans it
    assert "0" in gts[3].split("/") and "1" not in gts[3].split("/")
    # the random insertion: whatever the restatement says, never the alternative allele
    assert set(gts[4].split("/")) <= {"0", "."} and all(c[1] in (None, "other_allele", "not_spanned") for c in results[4])
    # clamped windows
    for k in (5, 7):
        assert max(0, sites[k][3] - 100) == 0
    for k in (6, 8):
        assert sites[k][4] + 100 > len(SEQS[sites[k][2]])
    # the <DEL>: the sequence-resolved record's genotype
    assert sites[9][1] == "DEL" and gts[9] == gts[1]


def test_site_windows_are_clamped():
    lo, hi = SVIM_GENOTYPE.site_windows(np.array([0, 0, 1]), np.array([10, 950, 40]), np.array([70, 990, 40]), np.array([1000, 50]), 100)
    assert lo.tolist() == [0, 850, 0] and hi.tolist() == [170, 1000, 50]


def test_a_site_without_its_alignments_is_not_spanned(tmp_path, device):
    sites, results = golden_expectation(haploid=True)
    k = next(i for i, c in enumerate(results) if c[0][0] == "1" and sites[i][1] == "DEL")
    _cols, _kind, contig, s, e, _seq = sites[k]
    gone = [(a[0], a[1]) for a in alignments(HAP1) if a[0] == contig and a[1] <= s - 100 and a[2] >= e + 100]
    assert gone
    bam = bamio.AlignmentFile(HAP1, reader="python")
    lines = [l for l in stw.records_of_bam(bam) if (l.split("\t")[2], int(l.split("\t")[3]) - 1) not in gone]
    sam = str(tmp_path / "cut.sam")
    stw.write_sam(sam, bam.references, bam.lengths, lines)
    left = [a for a in alignments(HAP1) if (a[0], a[1]) not in gone]
    expected = G.genotypes(sites, [left], SEQS)
    assert expected[k][0][:2] == (".", "not_spanned")
    assert genotype_cli.main([str(tmp_path / "out"), REF, SITES, sam]) == 0
    summary = check_outputs(str(tmp_path / "out"), SITES, sites, expected, 1, n_data_lines(SITES))
    assert summary["haplotypes"][0]["not_spanned"] >= 1


# ------------------------------------------------------------------------------ refusals and exit statuses
def test_argument_errors_exit_2_before_any_work(tmp_path, capsys):
    out = str(tmp_path / "out")
    for extra in (["--flank", "-1"], ["--max_relative_distance", "1.5"], ["--min_sv_size", "-3"], ["--sample", "a\tb"]):
        assert genotype_cli.main([out, REF, SITES, HAP1] + extra) == 2
    assert genotype_cli.main([out, REF, str(tmp_path / "none.vcf"), HAP1]) == 2
    assert genotype_cli.main([out, REF, SITES, str(tmp_path / "none.bam")]) == 2
    assert genotype_cli.main([out, REF, SITES, HAP1, "--query2", REF]) == 2
    assert "svim-asm-genotype:" in capsys.readouterr().err and not os.path.exists(out)


def test_unusable_genome_or_vcf_exit_1(tmp_path, device, caplog):
    out = str(tmp_path / "out")
    assert genotype_cli.main([out, str(tmp_path / "none.fa"), SITES, HAP1]) == 1
    other = str(tmp_path / "other.vcf")
    with open(other, "w") as fh:
        fh.writelines([l for l in open(SITES) if l.startswith("#")] + ["chrNone\t5\t.\tACGT\tA\t.\tPASS\t.\n"])
    assert genotype_cli.main([out, REF, other, HAP1]) == 1
    assert any("chrNone" in r.getMessage() for r in caplog.records)
    broken = str(tmp_path / "broken.vcf")
    open(broken, "w").write("chr1\t5\t.\tACGT\tA\t.\tPASS\t.\n")
    assert genotype_cli.main([out, REF, broken, HAP1]) == 1
    # a genome without one of the alignments' contigs
    small = str(tmp_path / "small.fa")
    pw.write_fasta(small, ["chr1"], [SEQS["chr1"]])
    only1 = str(tmp_path / "chr1.vcf")
    with open(only1, "w") as fh:
        fh.writelines(l for l in open(SITES) if l.startswith("#") or l.startswith("chr1\t"))
    assert genotype_cli.main([out, small, only1, HAP1]) == 1
    assert any("genome does not have" in r.getMessage() for r in caplog.records)
    assert not os.path.exists(os.path.join(out, "genotypes.vcf"))
