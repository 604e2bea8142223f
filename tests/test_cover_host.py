"""Non-carrier genotyping of the cohort merge where there is no GPU: --keep_coverage and its file,
svim-asm-merge --genotype_non_carriers with the kernels answered by the oracle (tests/helpers.OracleBackedContext) and
svx_cover_query by the plain loops of tests/cover_restatement.py — every genotype column, NS, AC and AN of every record
against the loop restatement.  tests/test_gpu_cover.py holds the real kernel to the same restatement."""
import logging
import os

import numpy as np
import pytest

from svim_asm_amd import SVCandidate, SVIM_COLLECT, SVIM_MERGE, bamio
from svim_asm_amd.fasta import FastaFile
from svim_asm_amd.table import CandidateTable
from tests import cover_cases as K, cover_restatement as R, helpers, merge_restatement as MR, paf_writer as pw, sam_text_writer as stw

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config1")
REF = os.path.join(GOLD, "ref.fa")
HAP1, HAP2 = os.path.join(GOLD, "hap1.bam"), os.path.join(GOLD, "hap2.bam")
SEQS = MR.read_fasta(REF)
NAMES = list(SEQS)
LENGTH = {n: len(SEQS[n]) for n in NAMES}
BAM = helpers.FakeBam(NAMES, [LENGTH[n] for n in NAMES], [])
REF_OPS = (0, 2, 3, 7, 8)  # M D N = X


def restated_cover_query(self, start_key, end_key, list_off, q_lo, q_hi):
    """Context.cover_query answered by the loops of tests/cover_restatement.py."""
    restated_cover_query.calls += 1
    off = [int(x) for x in list_off]
    pairs = list(zip([int(x) for x in start_key], [int(x) for x in end_key]))
    lists = [pairs[off[l]:off[l + 1]] for l in range(len(off) - 1)]
    queries = list(zip([int(x) for x in q_lo], [int(x) for x in q_hi]))
    return np.array(R.cover(lists, queries), dtype=np.uint8).reshape(len(lists), len(queries))


restated_cover_query.calls = 0


@pytest.fixture
def device(monkeypatch):
    monkeypatch.setattr(helpers.OracleBackedContext, "cover_query", restated_cover_query, raising=False)
    return helpers.oracle_backed_device(monkeypatch)


def python_intervals(path, min_mapq=20):
    """(tid, start, end) of the records COLLECT's loop visits, from the pure-Python reader and a walk of the CIGAR."""
    f = bamio.AlignmentFile(path, reader="python")
    out = []
    for contig in f.references:
        for a in f.fetch(contig=contig):
            if a.is_unmapped or a.is_secondary or a.mapping_quality < min_mapq:
                continue
            ref_len = sum(n for op, n in a.cigartuples if op in REF_OPS)
            if ref_len:
                out.append((a.reference_id, a.reference_start, a.reference_start + ref_len))
    assert out == sorted(out, key=lambda t: t[:2])
    return out


def as_tuples(triple):
    return list(zip(*[np.asarray(a).tolist() for a in triple]))


def run(argv):
    from svim_asm_amd import cli
    return cli.main(argv)


def listing(d):
    return sorted(n for n in os.listdir(d) if not n.endswith(".log"))


def undated(path):
    return [l for l in open(path) if not l.startswith("##fileDate=")]


# ------------------------------------------------------------------------------ the file
def test_coverage_file_round_trips():
    lists = [(np.array([0, 0, 2]), np.array([5, 5, 1 << 31]), np.array([90, 60, (1 << 31) + 7])),
             (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))]
    cov = SVIM_MERGE.Coverage(NAMES, [LENGTH[n] for n in NAMES], lists)
    blob = cov.to_wire()
    assert blob.startswith(SVIM_MERGE.COVERAGE_MAGIC) and b"pickle" not in blob
    back = SVIM_MERGE.Coverage.from_wire(blob)
    assert back.contigs == NAMES and back.contig_len.tolist() == [LENGTH[n] for n in NAMES]
    assert [as_tuples(t) for t in back.lists] == [as_tuples(t) for t in lists]
    assert back.to_wire() == blob
    one = SVIM_MERGE.Coverage.from_wire(SVIM_MERGE.Coverage(NAMES, [1, 2, 3], lists[:1]).to_wire())
    assert len(one.lists) == 1 and as_tuples(one.lists[0]) == as_tuples(lists[0])
    wrong_version = bytearray(blob)
    wrong_version[8] = 9
    with pytest.raises(ValueError, match="version 9"):
        SVIM_MERGE.Coverage.from_wire(bytes(wrong_version))


def test_read_coverage_names_the_path_and_the_option(tmp_path):
    path = str(tmp_path / "coverage.svxt")
    with pytest.raises(ValueError) as e:
        SVIM_MERGE.read_coverage(str(tmp_path))
    assert path in str(e.value) and "--keep_coverage" in str(e.value)
    whole = SVIM_MERGE.Coverage(NAMES, [LENGTH[n] for n in NAMES], [(np.arange(50) % 3, np.arange(50), np.arange(50) + 9)]).to_wire()
    for blob in (whole[:len(whole) // 2], whole[:10], b"",
                 CandidateTable.from_objects([SVCandidate.CandidateDeletion("chr1", 5, 90, ["r"], BAM, "1/1")], BAM).to_wire()):
        open(path, "wb").write(blob)
        with pytest.raises(ValueError) as e:
            SVIM_MERGE.read_coverage(str(tmp_path))
        assert path in str(e.value) and "--keep_coverage" in str(e.value)
    open(path, "wb").write(whole)
    assert len(SVIM_MERGE.read_coverage(str(tmp_path)).lists[0][0]) == 50


# ------------------------------------------------------------------------------ --keep_coverage
def test_keep_coverage_writes_the_intervals_of_the_records_collect_visits(tmp_path, device):
    run(["diploid", str(tmp_path / "plain"), HAP1, HAP2, REF])
    run(["diploid", str(tmp_path / "kept"), HAP1, HAP2, REF, "--keep_candidates", "--keep_coverage"])
    run(["diploid", str(tmp_path / "table"), HAP1, HAP2, REF, "--keep_candidates"])
    assert listing(tmp_path / "plain") == ["variants.vcf"]
    assert listing(tmp_path / "table") == ["candidates.svxt", "variants.vcf"]
    assert listing(tmp_path / "kept") == ["candidates.svxt", "coverage.svxt", "variants.vcf"]
    assert undated(tmp_path / "kept" / "variants.vcf") == undated(tmp_path / "plain" / "variants.vcf")
    assert open(tmp_path / "kept" / "candidates.svxt", "rb").read() == open(tmp_path / "table" / "candidates.svxt", "rb").read()
    cov = SVIM_MERGE.read_coverage(str(tmp_path / "kept"))
    f = bamio.AlignmentFile(HAP1, reader="python")
    assert cov.contigs == list(f.references) and cov.contig_len.tolist() == list(f.lengths)
    assert [as_tuples(t) for t in cov.lists] == [python_intervals(HAP1), python_intervals(HAP2)]
    assert len(cov.lists[0][0]) > 30 and len(cov.lists[1][0]) > 30
    # the filter is the loop's: a stricter --min_mapq keeps fewer or the same, never others
    run(["haploid", str(tmp_path / "strict"), HAP2, REF, "--keep_coverage", "--min_mapq", "61"])
    assert listing(tmp_path / "strict") == ["coverage.svxt", "variants.vcf"]
    strict = SVIM_MERGE.read_coverage(str(tmp_path / "strict"))
    assert len(strict.lists) == 1 and as_tuples(strict.lists[0]) == python_intervals(HAP2, 61)


def test_keep_coverage_from_sam_and_paf_input(tmp_path, device):
    sam = stw.bam_as_sam(HAP1, str(tmp_path / "h1.sam"), so="unsorted", shuffle_seed=11)
    paf, query = pw.bam_as_paf(HAP2, str(tmp_path / "h2.paf"), str(tmp_path / "q2.fa"), shuffle_seed=12)
    run(["diploid", str(tmp_path / "wd"), sam, paf, REF, "--query2", query, "--keep_coverage"])
    assert listing(tmp_path / "wd") == ["coverage.svxt", "variants.vcf"]
    cov = SVIM_MERGE.read_coverage(str(tmp_path / "wd"))
    assert [as_tuples(t) for t in cov.lists] == [python_intervals(HAP1), python_intervals(HAP2)]


def test_coverage_of_the_golden_sam_fixture(device):
    """tests/golden/chimeric_read_errors.sam (samtools' text of a queryname-ordered file): the reader presents the records
    by contig and coordinate, the intervals are those of the kept lines."""
    path = os.path.join(os.path.dirname(GOLD), "chimeric_read_errors.sam")
    header = [l.split("\t")[1][3:] for l in open(path) if l.startswith("@SQ")]
    expected = []
    for no, line in enumerate(l for l in open(path) if not l.startswith("@")):
        f = line.rstrip("\n").split("\t")
        flag, mapq = int(f[1]), int(f[4])
        if flag & 0x4 or flag & 0x100 or mapq < 20 or f[2] == "*" or f[5] == "*":
            continue
        ref_len, n = 0, ""
        for ch in f[5]:
            if ch.isdigit():
                n += ch
            else:
                ref_len += int(n) if ch in "MDN=X" else 0
                n = ""
        if ref_len:
            expected.append((header.index(f[2]), int(f[3]) - 1, int(f[3]) - 1 + ref_len, no))
    expected = [t[:3] for t in sorted(expected, key=lambda t: (t[0], t[1], t[3]))]
    assert len(expected) >= 2
    f = bamio.AlignmentFile(path)
    (table,) = SVIM_COLLECT.collect_tables([f], helpers.options(keep_coverage=True), ctx=device)
    assert as_tuples(table.coverage) == expected
    (table,) = SVIM_COLLECT.collect_tables([bamio.AlignmentFile(path)], helpers.options(), ctx=device)
    assert not hasattr(table, "coverage")


def test_a_sharded_run_refuses_keep_coverage_by_name(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    assert run(["diploid", str(tmp_path / "wd"), HAP1, HAP2, REF, "--keep_coverage"]) == 2
    assert "--keep_coverage" in capsys.readouterr().err and not os.path.exists(tmp_path / "wd")


# ------------------------------------------------------------------------------ the merge
def records_of(path):
    return [l.rstrip("\n").split("\t") for l in open(path) if not l.startswith("#")]


def line_records(merged, sample_names, tmp, monkeypatch):
    """Which record each body line of the cohort VCF belongs to: the writer run with the record's index as the text of
    the first sample column."""
    o = helpers.options(working_dir=str(tmp))
    os.makedirs(str(tmp), exist_ok=True)

    def labels(G, C=None):
        out = []
        for lines in ([("R%d" % r).encode() for r in range(len(G))], [b""] * len(G)):
            off = np.zeros(len(lines) + 1, np.int64)
            np.cumsum([len(x) for x in lines], out=off[1:])
            out.append((b"".join(lines), off))
        return tuple(out)
    with monkeypatch.context() as m:
        m.setattr(SVIM_MERGE, "_cohort_texts", labels)
        path = SVIM_MERGE.write_cohort_vcf(merged, np.zeros((len(merged), 1), np.uint8), sample_names[:1], "1.0.3",
                                           o.types.split(","), FastaFile(REF), o)
    return [int(rec[9][1:]) for rec in records_of(path)]


def named(intervals, contigs):
    return [(contigs[t], s, e) for t, s, e in intervals]


def expected_texts(merged, G, haplotypes, margin):
    """[record][sample] by the loop restatement; haplotypes: per sample a list of interval lists (named contigs)."""
    out = []
    for c, row in zip(merged.objects(), G.tolist()):
        wins = R.windows(c, margin, LENGTH)
        out.append([R.sample_text(SVIM_MERGE.GT_TEXT[g], wins, haps) for g, haps in zip(row, haplotypes)])
    return out


def check_cohort_vcf(path, plain_path, merged, texts, line_rec):
    """Every line: the plain file's up to INFO's suffix, the restatement's columns and counts."""
    recs, plain = records_of(path), records_of(plain_path)
    assert len(recs) == len(plain) == len(line_rec) > 0
    for rec, one, r in zip(recs, plain, line_rec):
        assert rec[:7] == one[:7] and rec[8] == one[8] == "GT"
        assert rec[7].split(";NS=")[0] == one[7].split(";NS=")[0]
        assert rec[9:] == texts[r], (r, rec[:3])
        info = dict(kv.split("=") for kv in rec[7].split(";") if "=" in kv)
        assert (int(info["NS"]), int(info["AC"]), int(info["AN"])) == R.counts(texts[r]), (r, rec[:3])
        old = dict(kv.split("=") for kv in one[7].split(";") if "=" in kv)
        assert info["AC"] == old["AC"]


@pytest.fixture
def cohort(tmp_path, device):
    """s1 = (hap1, hap2), s2 = (hap2, hap1), s3 = haploid on hap1 alone, each with its table and its coverage."""
    dirs = [str(tmp_path / n) for n in ("s1", "s2", "s3")]
    run(["diploid", dirs[0], HAP1, HAP2, REF, "--keep_candidates", "--keep_coverage"])
    run(["diploid", dirs[1], HAP2, HAP1, REF, "--keep_candidates", "--keep_coverage"])
    run(["haploid", dirs[2], HAP1, REF, "--keep_candidates", "--keep_coverage"])
    return dirs


def test_merge_genotypes_non_carriers_as_the_restatement_does(tmp_path, cohort, device, monkeypatch):
    from svim_asm_amd import merge_cli
    names = ["s1", "s2", "s3"]
    h1, h2 = python_intervals(HAP1), python_intervals(HAP2)
    contigs = list(bamio.AlignmentFile(HAP1, reader="python").references)
    tables = [SVIM_MERGE.read_candidates(d) for d in cohort]
    o = helpers.options()
    merged, G = SVIM_MERGE.merge_tables(tables, names, FastaFile(REF), o, ctx=device)
    line_rec = line_records(merged, names, tmp_path / "labels", monkeypatch)
    # ---- without the option: today's file
    assert merge_cli.main([str(tmp_path / "plain"), REF] + cohort) == 0
    assert restated_cover_query.calls == 0
    plain = str(tmp_path / "plain" / "cohort.vcf")
    assert all(set(r[9:]) <= {"./.", "1/0", "0/1", "1/1"} for r in records_of(plain))
    assert sum(l.startswith("##INFO=<ID=AN,") and "haplotypes of the samples with the variant" in l for l in open(plain)) == 1
    # ---- with it
    assert merge_cli.main([str(tmp_path / "gt"), REF] + cohort + ["--genotype_non_carriers"]) == 0
    assert restated_cover_query.calls == 1  # every window of every record against every list: ONE call
    haplotypes = [[named(h1, contigs), named(h2, contigs)], [named(h2, contigs), named(h1, contigs)], [named(h1, contigs)]]
    texts = expected_texts(merged, G, haplotypes, 1000)
    path = str(tmp_path / "gt" / "cohort.vcf")
    check_cohort_vcf(path, plain, merged, texts, line_rec)
    s3 = [t[2] for t in texts]
    assert "0/0" in s3 and all(t in ("0/0", "./.", "1/1") for t in s3)
    assert [l for l in undated(path) if l.startswith("##") and "ID=NS" not in l and "ID=AC" not in l and "ID=AN" not in l] == \
        [l for l in undated(plain) if l.startswith("##") and "ID=NS" not in l and "ID=AC" not in l and "ID=AN" not in l]
    assert sum(l.startswith("##INFO=<ID=AN,") and "called alleles" in l for l in open(path)) == 1
    # a carrier keeps what it had, the 0 of a 1/0 included
    for row, text in zip(G.tolist(), texts):
        for g, t in zip(row, text):
            assert g == 0 or t == SVIM_MERGE.GT_TEXT[g]
    # ---- a margin of its own
    assert merge_cli.main([str(tmp_path / "gt5"), REF] + cohort + ["--genotype_non_carriers", "--genotype_margin", "5"]) == 0
    check_cohort_vcf(str(tmp_path / "gt5" / "cohort.vcf"), plain, merged, expected_texts(merged, G, haplotypes, 5), line_rec)
    # ---- s3 without the alignments over one record it was 0/0 at
    r = s3.index("0/0")
    wins = R.windows(merged.objects()[r], 1000, LENGTH)
    left = [iv for iv in named(h1, contigs) if not any(iv[0] == c and iv[1] <= lo and iv[2] >= hi for c, lo, hi in wins)]
    assert 0 < len(left) < len(h1)
    tid = {n: i for i, n in enumerate(contigs)}
    cov = SVIM_MERGE.read_coverage(cohort[2])
    SVIM_MERGE.keep_coverage(cov.contigs, cov.contig_len, [tuple(np.array([(tid[c], s, e) for c, s, e in left]).T)], cohort[2])
    assert merge_cli.main([str(tmp_path / "cut"), REF] + cohort + ["--genotype_non_carriers"]) == 0
    cut = expected_texts(merged, G, haplotypes[:2] + [[left]], 1000)
    assert cut[r][2] == "./." and cut != texts
    check_cohort_vcf(str(tmp_path / "cut" / "cohort.vcf"), plain, merged, cut, line_rec)
    # ---- bgzip output: the same text
    import gzip
    monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", "0")
    assert merge_cli.main([str(tmp_path / "gz"), REF] + cohort + ["--genotype_non_carriers", "--bgzip_output"]) == 0
    text = gzip.decompress(open(tmp_path / "gz" / "cohort.vcf.gz", "rb").read()).decode()
    assert [l for l in text.splitlines(True) if not l.startswith("##fileDate=")] == undated(str(tmp_path / "cut" / "cohort.vcf"))


def test_merge_names_a_missing_coverage_file(tmp_path, cohort, device, caplog):
    from svim_asm_amd import merge_cli
    os.remove(os.path.join(cohort[1], "coverage.svxt"))
    with caplog.at_level(logging.ERROR):
        assert merge_cli.main([str(tmp_path / "out"), REF] + cohort + ["--genotype_non_carriers"]) == 1
    errors = [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR]
    assert len(errors) == 1 and os.path.join(cohort[1], "coverage.svxt") in errors[0] and "--keep_coverage" in errors[0]
    assert not os.path.exists(tmp_path / "out" / "cohort.vcf")


def test_cohort_command_passes_the_option_on(tmp_path, device, monkeypatch):
    """svim-asm-cohort --merge OUT --genotype_non_carriers (single process): --keep_coverage for every sample, the merge
    with the option; and the argument list of the merge child of --gpus N."""
    from svim_asm_amd import cli, cohort as cohort_cmd
    monkeypatch.setattr(cli, "_warm_device", lambda device: None)
    manifest = tmp_path / "cohort.tsv"
    manifest.write_text("%s %s %s\n%s %s %s\n" % (tmp_path / "s1", HAP1, HAP2, tmp_path / "s2", HAP2, HAP1))
    assert cohort_cmd.main(["diploid", str(manifest), REF, "--merge", str(tmp_path / "all"), "--genotype_non_carriers"]) == 0
    for s in ("s1", "s2"):
        assert listing(tmp_path / s) == ["candidates.svxt", "coverage.svxt", "variants.vcf"]
    assert sum(l.startswith("##INFO=<ID=AN,") and "called alleles" in l for l in open(tmp_path / "all" / "cohort.vcf")) == 1
    assert cohort_cmd.main(["diploid", str(manifest), REF, "--genotype_non_carriers"]) == 2  # (an option of the merge)
    rest, extra = cohort_cmd._take_genotype(["--min_mapq", "30", "--genotype_margin", "70", "--genotype_non_carriers"])
    assert rest == ["--min_mapq", "30", "--keep_coverage"] and extra == ["--genotype_non_carriers", "--genotype_margin", "70"]
    argv = cohort_cmd._merge_command("diploid", "OUT", REF, ["a", "b"], 3, rest, extra)
    assert argv[-3:] == extra and "--keep_coverage" not in argv and argv[argv.index("--device") + 1] == "3"
    assert cohort_cmd._take_genotype(["--verbose"]) == (["--verbose"], [])


# ------------------------------------------------------------------------------ hand-built records
def coverage(*lists):
    tid = {n: i for i, n in enumerate(NAMES)}
    cols = [tuple(np.array([(tid[c], s, e) for c, s, e in l], dtype=np.int64).reshape(-1, 3).T) for l in lists]
    return SVIM_MERGE.Coverage(NAMES, [LENGTH[n] for n in NAMES], cols)


def codes(cands, covs, **opts):
    merged = CandidateTable.from_objects(cands, BAM)
    C = SVIM_MERGE.genotype_non_carriers(merged, covs, helpers.options(**opts), helpers.OracleBackedContext())
    exp = [[sum(bit << k for k, bit in enumerate(int(R.haplotype_is_reference(R.windows(c, opts.get("genotype_margin", 1000), LENGTH),
                                                                               [(NAMES[t], s, e) for t, s, e in as_tuples(h)]))
                                                  for h in (cov.lists[0], cov.lists[-1]))) for cov in covs] for c in cands]
    assert C.tolist() == exp and C.dtype == np.uint8
    return C.tolist()


def test_a_breakend_needs_both_ends_and_takes_them_from_different_alignments(device):
    bnd = SVCandidate.CandidateBreakend("chr1", 60000, "fwd", "chr2", 7000, "fwd", ["r"], BAM, "1/1")
    one_end = coverage([("chr1", 50000, 70000)], [("chr2", 0, 9000)])
    both = coverage([("chr1", 50000, 70000), ("chr2", 6000, 8000)], [("chr1", 59000, 61000), ("chr1", 61000, 90000), ("chr2", 1, 8001)])
    abut = coverage([("chr1", 50000, 60500), ("chr1", 60500, 70000), ("chr2", 0, 100000)])
    assert codes([bnd], [one_end, both, abut]) == [[0, 3, 0]]
    # haplotype 2 of the second sample: [59000, 61000] exactly, and one base short on either side
    assert codes([bnd], [coverage([("chr1", 0, 1)], [("chr1", 59001, 61000), ("chr2", 0, 9000)]),
                         coverage([("chr1", 0, 1)], [("chr1", 59000, 60999), ("chr2", 0, 9000)])]) == [[0, 0]]


def test_contig_mismatch_between_table_and_coverage_is_refused(device):
    merged = CandidateTable.from_objects([SVCandidate.CandidateDeletion("chr1", 5000, 5050, ["r"], BAM, "1/1")], BAM)
    good = coverage([("chr1", 0, 9000)])
    other = SVIM_MERGE.Coverage(NAMES, [LENGTH[n] - (n == "chr2") for n in NAMES], good.lists)
    o = helpers.options()
    with pytest.raises(ValueError, match="sample second .* contig 2 is chr2 .100000 bp. in the tables and chr2 .99999 bp. in its coverage"):
        SVIM_MERGE.genotype_non_carriers(merged, [good, other], o, helpers.OracleBackedContext(), sample_names=["first", "second"])
    renamed = SVIM_MERGE.Coverage(["chr1", "chrTen", "chr2"], [LENGTH[n] for n in NAMES], good.lists)
    with pytest.raises(ValueError, match="contig 1 is chr10 .150000 bp. in the tables and chrTen .150000 bp. in its coverage"):
        SVIM_MERGE.genotype_non_carriers(merged, [renamed], o, helpers.OracleBackedContext())


def test_windows_are_clamped_to_the_contig(device):
    end = LENGTH["chr2"]
    cands = [SVCandidate.CandidateDeletion("chr1", 300, 420, ["r"], BAM, "1/1"),
             SVCandidate.CandidateInsertion("chr2", end - 200, end - 140, ["r"], "A" * 60, BAM, "1/1"),
             SVCandidate.CandidateDuplicationTandem("chr2", end - 500, end - 100, 2, True, ["r"], BAM, "1/1"),
             SVCandidate.CandidateDuplicationInterspersed("chr1", 120000, 120200, "chr10", 150, 350, ["r"], BAM, False, "1/1"),
             SVCandidate.CandidateInversion("chr10", 20000, 20400, ["r"], True, BAM, "1/1")]
    merged = CandidateTable.from_objects(cands, BAM)
    rec, contig, lo, hi = SVIM_MERGE.record_windows(merged, 1000)
    got = [(NAMES[c], a, b) for c, a, b in zip(contig.tolist(), lo.tolist(), hi.tolist())]
    assert got == [w for c in cands for w in R.windows(c, 1000, LENGTH)] and rec.tolist() == list(range(5))
    assert got[0] == ("chr1", 0, 1420) and got[1] == ("chr2", end - 1200, end) and got[2] == ("chr2", end - 1500, end)
    assert got[3] == ("chr10", 0, 1150) and got[4] == ("chr10", 19000, 21400)
    whole = coverage([(n, 0, LENGTH[n]) for n in NAMES])
    short = coverage([("chr1", 1, LENGTH["chr1"]), ("chr2", 0, end - 1), ("chr10", 0, 1149)], [(n, 0, LENGTH[n]) for n in NAMES])
    assert codes(cands, [whole, short]) == [[3, 2], [3, 2], [3, 2], [3, 2], [3, 2]]
    # margin 0: the record itself
    assert codes(cands[:1], [coverage([("chr1", 300, 420)]), coverage([("chr1", 301, 420)])], genotype_margin=0) == [[3, 0]]
    # no record, no sample
    assert SVIM_MERGE.genotype_non_carriers(CandidateTable.from_objects([], BAM), [whole], helpers.options(),
                                            helpers.OracleBackedContext()).shape == (0, 1)


# ------------------------------------------------------------------------------ the device's cases and the probe's host version
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_the_device_cases_are_valid_balanced_and_one_prefix_maximum_answers_them(name):
    """tests/test_gpu_cover.py runs these on the device; here the conditions on the inputs, and the argument of
    svx_cover_query on the host: tools/cover_probe.py's searchsorted + maximum.accumulate gives the restatement's answers."""
    from tools import cover_probe
    lists, queries = K.CASES[name]()
    K.check_inputs(lists, queries)
    expected = K.answers(name)
    assert K.is_balanced(expected)
    start = np.array([s for ivs in lists for s, _ in ivs], dtype=np.uint64)
    end = np.array([e for ivs in lists for _, e in ivs], dtype=np.uint64)
    off = np.cumsum([0] + [len(ivs) for ivs in lists]).astype(np.uint64)
    lo, hi = (np.array([q[k] for q in queries], dtype=np.uint64) for k in (0, 1))
    assert cover_probe.on_host(start, end, off, lo, hi).tolist() == expected


def test_the_probes_batch_is_a_valid_one():
    from tools import cover_probe
    start, end, off, lo, hi = cover_probe.synthetic_batch(6, 500, 300)
    assert off.tolist() == [500 * k for k in range(7)] and len(start) == len(end) == 3000 and len(lo) == len(hi) == 300
    for l in range(6):
        s, e = start[500 * l:500 * (l + 1)], end[500 * l:500 * (l + 1)]
        assert bool((s[1:] >= s[:-1]).all()) and bool(((s >> np.uint64(32)) == (e >> np.uint64(32))).all()) and bool((e >= s).all())
    assert bool((lo <= hi).all()) and bool(((lo >> np.uint64(32)) == (hi >> np.uint64(32))).all())
    share = float(cover_probe.on_host(start, end, off, lo, hi).mean())
    assert 0.1 < share < 0.9
