"""The cohort merge (svim_asm_amd/SVIM_MERGE.py) where there is no GPU: the kernels answered by the oracle
(tests/helpers.OracleBackedContext), every merged table and genotype matrix held against the plain-Python restatement
(tests/merge_restatement.py); the multi-sample VCF writer; --keep_candidates.  The cohort-sized partitions of
tests/merge_cases.py: every type at 11, 17 and 33 distinct alleles, the cohort with every type and partition size at
once, the chunked distance path, and the condensed vectors handed to the linkage call; the cases that only run on the
device (tests/test_gpu_merge.py) are held to their non-triviality condition here."""
import gzip
import logging
import os

import numpy as np
import pytest

from svim_asm_amd import SVCandidate, SVIM_COMBINE, SVIM_MERGE
from svim_asm_amd.fasta import FastaFile
from svim_asm_amd.table import CandidateTable
from tests import helpers, merge_cases as M, merge_restatement as R, tabix_reader

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config1")
REF = os.path.join(GOLD, "ref.fa")
SEQS = R.read_fasta(REF)
NAMES = list(SEQS)
BAM = helpers.FakeBam(NAMES, [len(SEQS[n]) for n in NAMES], [])
SAMPLES = ["s0", "s1", "s2", "s3"]


def DEL(start, size=50, gt="1/1", contig="chr1"):
    return SVCandidate.CandidateDeletion(contig, start, start + size, ["r"], BAM, gt)


def INS(pos, seq, gt="1/1", contig="chr1"):
    return SVCandidate.CandidateInsertion(contig, pos, pos + len(seq), ["r"], seq, BAM, gt)


def BND(pos, dest, sdir="fwd", ddir="fwd", gt="1/1"):
    return SVCandidate.CandidateBreakend("chr1", pos, sdir, "chr2", dest, ddir, ["r"], BAM, gt)


def del_distance(a, b):
    return R.edit_distance(*R.haplotypes(DEL(a), DEL(b), SEQS))


def hand_built_cohort():
    """Four samples with every kind of locus at once (also the case tests/test_gpu_merge.py runs on the real context)."""
    seq = "ACGTTGCAAGGCTTAACCGGTTAGCATCGATCGGATCCATGCAAGTCTAGGCTAAGCTT"
    other = seq[:20] + "CCC" + seq[23:]
    return [
        [DEL(5000, gt="1/0"), DEL(5003, gt="0/1"), INS(30000, seq), BND(60000, 7000), DEL(90000), DEL(150000, 60),
         SVCandidate.CandidateInversion("chr10", 20000, 20400, ["r"], True, BAM, "1/1")],
        [DEL(5000), INS(30000, other, "1/0"), BND(60030, 7040, gt="0/1"), DEL(90040), DEL(90400, 80),
         SVCandidate.CandidateDuplicationTandem("chr2", 40000, 40120, 2, True, ["r"], BAM, "1/0")],
        [DEL(5003, gt="1/0"), INS(30000, seq, "0/1"), BND(60010, 7000, "rev", "fwd"), DEL(90080), DEL(91390, 45),
         SVCandidate.CandidateInversion("chr10", 20004, 20400, ["r"], False, BAM, "0/1"),
         SVCandidate.CandidateDuplicationTandem("chr2", 40000, 40120, 3, True, ["r"], BAM, "1/1")],
        [DEL(5000, gt="0/1"), DEL(150000, 60, "1/0"), DEL(90120), DEL(90160), DEL(90200),
         SVCandidate.CandidateDuplicationInterspersed("chr1", 120000, 120200, "chr2", 50000, 50200, ["r"], BAM, False, "1/1")],
    ]


def both(samples, ctx=None, **opts):
    """merge_tables on the oracle-backed context (or `ctx`) == the restatement; returns the records."""
    o = helpers.options(**opts)
    tables = [CandidateTable.from_objects(s, BAM) for s in samples]
    merged, G = SVIM_MERGE.merge_tables(tables, SAMPLES[:len(samples)], FastaFile(REF), o, ctx=ctx or helpers.OracleBackedContext())
    assert G.shape == (len(merged), len(samples))
    got = [(R.allele_key(c), [SVIM_MERGE.GT_TEXT[g] for g in row]) for c, row in zip(merged.objects(), G.tolist())]
    exp, _ = R.merge(samples, SEQS, o.partition_max_distance, o.max_edit_distance, getattr(o, "merge_max_partition", 1024))
    assert got == exp
    return got


def test_identical_alleles_in_all_samples_are_one_record():
    got = both([[DEL(5000, gt=g)] for g in ("1/1", "1/0", "0/1", "1/1")])
    assert got == [(("DEL", "chr1", 5000, 5050), ["1/1", "1/0", "0/1", "1/1"])]


def test_alleles_within_the_threshold_are_one_record_of_the_better_supported():
    d = del_distance(5000, 5003)
    assert 0 < d <= 200
    got = both([[DEL(5003)], [DEL(5000, gt="1/0")], [DEL(5000, gt="0/1")], [DEL(5000)]])
    assert got == [(("DEL", "chr1", 5000, 5050), ["1/1", "1/0", "0/1", "1/1"])]
    # two haplotypes against one: the later allele in partition order wins on support
    got = both([[DEL(5000, gt="1/0")], [DEL(5003)], [], []])
    assert got == [(("DEL", "chr1", 5003, 5053), ["1/0", "1/1", "./.", "./."])]


def test_a_tie_goes_to_the_earliest_in_partition_order():
    got = both([[DEL(5003, gt="1/0")], [DEL(5000, gt="0/1")], [], []])
    assert got == [(("DEL", "chr1", 5000, 5050), ["1/0", "0/1", "./.", "./."])]


def test_alleles_just_over_the_threshold_are_two_records():
    d = del_distance(5000, 5003)
    samples = [[DEL(5000)], [DEL(5003, gt="1/0")], [DEL(5000, gt="0/1")], []]
    assert len(both(samples, max_edit_distance=d)) == 1
    got = both(samples, max_edit_distance=d - 1)
    assert got == [(("DEL", "chr1", 5000, 5050), ["1/1", "./.", "0/1", "./."]),
                   (("DEL", "chr1", 5003, 5053), ["./.", "1/0", "./.", "./."])]


def test_two_rows_of_one_sample_in_one_cluster_make_it_homozygous():
    got = both([[DEL(5000, gt="1/0"), DEL(5003, gt="0/1")], [DEL(5003, gt="0/1")], [], []])
    assert got == [(("DEL", "chr1", 5003, 5053), ["1/1", "0/1", "./.", "./."])]


def twelve():
    """Twelve distinct deletions 40 bp apart: one partition."""
    return [[DEL(90000 + 40 * (4 * k + s), gt=("1/1", "1/0", "0/1")[(k + s) % 3]) for k in range(3)] for s in range(4)]


def test_a_partition_of_twelve_is_clustered_not_dropped():
    got = both(twelve(), max_edit_distance=90)
    assert 1 < len(got) < 12
    assert sum(g != "./." for _, row in got for g in row) >= 12
    assert len(both(twelve(), max_edit_distance=2000)) == 1


def test_a_partition_over_the_cap_comes_out_unclustered_with_a_warning(caplog):
    with caplog.at_level(logging.WARNING):
        got = both(twelve(), max_edit_distance=2000, merge_max_partition=5)
    assert len(got) == 12
    warnings = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "DEL" in warnings[0] and "chr1" in warnings[0]
    assert str(90025) in warnings[0] and str(90000 + 40 * 11 + 25) in warnings[0]


def test_breakends_pair_on_equal_directions_only():
    got = both([[BND(60000, 7000)], [BND(60030, 7040, gt="0/1")], [BND(60010, 7000, "rev", "fwd")], [BND(61500, 7000)]])
    assert [row for _, row in got] == [["1/1", "0/1", "./.", "./."], ["./.", "./.", "1/1", "./."], ["./.", "./.", "./.", "1/1"]]


def test_insertions_equal_in_coordinates_but_not_in_bytes_stay_distinct_alleles():
    seq = "ACGTTGCAAGGCTTAACCGGTTAGCATCGATCGGATCCATGCAAGTCTAGGCTAAGCTT"
    other = seq[:20] + "CCC" + seq[23:]
    samples = [[INS(30000, seq, "1/0")], [INS(30000, other)], [INS(30000, seq, "0/1")], [INS(30000, other, "1/0")]]
    got = both(samples, max_edit_distance=1)
    assert got == [(("INS", "chr1", 30000, 30000 + len(seq), seq), ["1/0", "./.", "0/1", "./."]),
                   (("INS", "chr1", 30000, 30000 + len(seq), other), ["./.", "1/1", "./.", "1/0"])]
    got = both(samples)  # within the threshold: one record, of the allele on three haplotypes
    assert got == [(("INS", "chr1", 30000, 30000 + len(seq), other), ["1/0", "1/1", "0/1", "1/0"])]


def test_the_hand_built_cohort():
    got = both(hand_built_cohort())
    assert len({k[0] for k, _ in got}) == 6  # every type


def test_contig_mismatch_is_refused():
    t = [CandidateTable.from_objects([DEL(5000)], BAM) for _ in range(3)]
    shorter = helpers.FakeBam(NAMES, [len(SEQS[n]) - (n == "chr2") for n in NAMES], [])
    t.append(CandidateTable.from_objects([], shorter))
    with pytest.raises(ValueError, match="contig 2 is chr2 .100000 bp. in the first and chr2 .99999 bp."):
        SVIM_MERGE.merge_tables(t, SAMPLES, FastaFile(REF), helpers.options(), ctx=helpers.OracleBackedContext())


def test_empty_samples():
    assert both([[], [], [], []]) == []
    assert both([[], [DEL(5000)], [], []]) == [(("DEL", "chr1", 5000, 5050), ["./.", "1/1", "./.", "./."])]


# ------------------------------------------------------------------------------ cohort-sized partitions
def test_the_compiled_edit_distances_equal_the_textbook_one():
    """The large cases' expected answers use the oracle's C full DP (and, for the wide cohort, its band-doubling DP) in
    place of the restatement's textbook rows: the three agree on haplotype pairs of every type from the builders."""
    from oracle import orc
    pairs = []
    for typ in ("DEL", "INS", "INV", "DUP_TAN", "DUP_INT"):
        objs = [make("1/1") for make in M.BUILDERS[typ](33)]
        pairs += [R.haplotypes(objs[i], objs[j], SEQS) for i, j in ((0, 1), (0, 32), (3, 17), (5, 6), (9, 30), (11, 12), (16, 31),
                                                                   (20, 21), (2, 29), (7, 25), (13, 14), (18, 27), (4, 4))]
    assert len(pairs) >= 60 and 600 < max(len(a) for a, _ in pairs) <= 700
    assert any(a != a.upper() for a, _ in pairs) and any("N" in a for a, _ in pairs)  # inserted bytes keep their case
    for a, b in pairs:
        d = R.edit_distance(a, b)
        assert orc.edit_distance(a.encode("latin-1"), b.encode("latin-1")) == d
        assert orc.edit_distance_banded(a.encode("latin-1"), b.encode("latin-1")) == d
    assert len({R.edit_distance(a, b) for a, b in pairs}) > 20


@pytest.mark.parametrize("n", [11, 17, 33])
@pytest.mark.parametrize("typ", M.TYPES)
def test_one_partition_of_every_type_beyond_ten_members(typ, n):
    assert M.is_non_trivial((typ, n))
    got, proxy = M.check((typ, n), helpers.OracleBackedContext())
    assert [sizes.tolist() for _, sizes, _ in proxy.linkage] == [[n]]
    assert proxy.distance_jobs == ([] if typ == "BND" else [n * (n - 1) // 2])


DEVICE_ONLY = [("DEL", 65), ("DEL", 128), ("DEL", 129), ("INS", 65), ("INS", 129), ("BND", 129), "wide"]


@pytest.mark.parametrize("case", DEVICE_ONLY, ids=str)
def test_the_cases_that_only_run_on_the_device_are_non_trivial(case):
    """tests/test_gpu_merge.py runs these against the restatement; here only the condition on the inputs: at the case's
    max_edit_distance the restatement makes more than one and fewer than n records and a cluster of three or more."""
    assert M.is_non_trivial(case)
    (typ, keys, cond), = M.expected(case)[1]
    assert len(keys) == (17 if case == "wide" else case[1])
    if typ == "BND":  # span-position distances on either side of 0.3 beside the direction-mismatch sentinel
        assert any(d < 0.3 for d in cond) and any(0.3 < d < 1 for d in cond) and 99999.0 in cond
    if case == "wide":
        a, b = R.haplotypes(DEL(100000, 40), DEL(100000 + 16 * 600, 40), SEQS)
        assert len(a) > 9500


def test_every_type_and_partition_size_in_one_call():
    assert M.is_non_trivial("everything")
    got, proxy = M.check("everything", helpers.OracleBackedContext())
    assert len({k[0] for k, _ in got}) == 6
    (_, edit_sizes, _), (_, bnd_sizes, cut) = proxy.linkage
    assert sorted(edit_sizes.tolist() + bnd_sizes.tolist()) == sorted(n for _, sizes in M.EVERYTHING for n in sizes if n > 1)
    assert cut == 0.3 and {10, 11, 15, 16, 17, 33, 65, 129} <= set(edit_sizes.tolist())
    # a fifth of the alleles is carried by more than one sample
    assert sum(sum(g != "./." for g in row) > 1 for _, row in got) >= 10


def _non_empty_chunks(jobs_per_partition, n_chunks):
    """Chunks of whole partitions: chunk boundary c (of n_chunks - 1) lies behind the first partition at which the
    running job count reaches c / n_chunks of all jobs; a partition belongs to the chunk numbered by the boundaries
    before it."""
    total, running, boundary = sum(jobs_per_partition), 0, {}
    for p, jobs in enumerate(jobs_per_partition):
        running += jobs
        for c in range(1, n_chunks):
            if c not in boundary and running * n_chunks >= total * c:
                boundary[c] = p
    return {sum(boundary[c] < p for c in range(1, n_chunks)) for p in range(len(jobs_per_partition))}


def test_chunked_distance_jobs_of_a_dominant_partition(monkeypatch):
    """SVIM_COMBINE._job_distances in chunks (as for 30 000 jobs or more), one partition holding most of the jobs: the
    answer is the one-chunk answer and the restatement's, also where a chunk comes out empty."""
    assert M.is_non_trivial("chunks")
    one, proxy = M.check("chunks", helpers.OracleBackedContext())
    jobs = [len(cond) for _, _, cond in M.expected("chunks")[1]]
    assert proxy.distance_jobs == [sum(jobs)] and max(jobs) == 33 * 32 // 2 and len(jobs) == 13
    monkeypatch.setattr(SVIM_COMBINE, "_PAIR_CHUNK_MIN_JOBS", 1)
    empty = []
    for n_chunks in (2, 3, 8):
        monkeypatch.setattr(SVIM_COMBINE, "_PAIR_CHUNKS", n_chunks)
        got, proxy = M.check("chunks", helpers.OracleBackedContext())
        assert got == one
        filled = _non_empty_chunks(jobs, n_chunks)
        assert len(proxy.distance_jobs) == len(filled) > 1 and sum(proxy.distance_jobs) == sum(jobs)
        empty.append(n_chunks - len(filled))
    assert max(empty) > 0


class _OffByOne(helpers.OracleBackedContext):
    """One exact distance well above the cut comes back one too large."""

    def haplotype_distance_batch_mixed(self, pool, pieces, k_max):
        out = helpers.OracleBackedContext.haplotype_distance_batch_mixed(self, pool, pieces, k_max)
        out[int(np.argmax(out))] += 1
        return out


def test_a_distance_wrong_by_one_fails_on_the_vectors_where_the_records_survive():
    case = ("DEL", 17)
    got, proxy = M.run(case, _OffByOne())
    assert got == M.expected(case)[0]  # the largest distance lies above the cut: the flat clusters do not move
    with pytest.raises(AssertionError):
        M.check(case, _OffByOne())


# ------------------------------------------------------------------------------ the writer
def _merged(opts=None):
    o = helpers.options(**(opts or {}))
    tables = [CandidateTable.from_objects(s, BAM) for s in hand_built_cohort()]
    return SVIM_MERGE.merge_tables(tables, SAMPLES, FastaFile(REF), o, ctx=helpers.OracleBackedContext()) + (o,)


def _records(text):
    return [l.split("\t") for l in text.splitlines() if not l.startswith("#")]


TYPES = "DEL,INS,INV,DUP:TANDEM,DUP:INT,BND".split(",")


@pytest.mark.parametrize("opts", [{}, {"symbolic_alleles": True, "query_names": True}])
def test_cohort_vcf_has_a_column_per_sample_and_the_single_sample_order(tmp_path, opts):
    merged, G, o = _merged(opts)
    o.working_dir = str(tmp_path)
    path = SVIM_MERGE.write_cohort_vcf(merged, G, SAMPLES, "1.0.3", TYPES, FastaFile(REF), o)
    assert path == str(tmp_path / "cohort.vcf") and sorted(os.listdir(tmp_path)) == ["cohort.vcf"]
    text = open(path).read()
    head = [l for l in text.splitlines() if l.startswith("#")]
    assert head[-1].split("\t") == "#CHROM POS ID REF ALT QUAL FILTER INFO FORMAT".split() + SAMPLES
    for key in ("NS", "AC", "AN"):
        assert sum(l.startswith("##INFO=<ID=%s," % key) for l in head) == 1
    assert not any(l.startswith(("##INFO=<ID=READS", "##FORMAT=<ID=CN")) for l in head)
    # the same rows through the single-sample writer: same lines up to INFO's suffix and the sample columns
    o.query_names = False
    SVIM_COMBINE.write_vcf_table(merged, "1.0.3", merged.contigs, merged.contig_len.tolist(), TYPES, FastaFile(REF), o)
    single = _records(open(tmp_path / "variants.vcf").read())
    recs = _records(text)
    assert len(recs) == len(single) == len(merged) + int((merged.type == 5).sum())  # a breakend is two lines
    by_key = {}
    for c, row in zip(merged.objects(), G.tolist()):
        by_key.setdefault((c.type, c.get_key()[1:]), []).append(row)
    for rec, one in zip(recs, single):
        assert len(rec) == 9 + len(SAMPLES) and rec[8] == "GT"
        assert rec[:7] == one[:7]
        info = dict(kv.split("=") for kv in rec[7].split(";") if "=" in kv)
        assert rec[7].startswith(one[7] + ";NS=") and "READS" not in info
        gts = rec[9:]
        assert set(gts) <= {"./.", "1/0", "0/1", "1/1"}
        ns = sum(g != "./." for g in gts)
        assert (int(info["NS"]), int(info["AC"]), int(info["AN"])) == (ns, sum(g.count("1") for g in gts), 2 * ns)
    assert sorted(tuple(r[9:]) for r in recs if "BND" not in r[2]) == \
        sorted(tuple(SVIM_MERGE.GT_TEXT[g] for g in row) for row, t in zip(G.tolist(), merged.type.tolist()) if t != 5)


def test_cohort_vcf_bgzip_output_round_trips_through_its_index(tmp_path, monkeypatch):
    monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", "0")
    merged, G, o = _merged()
    o.working_dir = str(tmp_path)
    SVIM_MERGE.write_cohort_vcf(merged, G, SAMPLES, "1.0.3", TYPES, FastaFile(REF), o)
    plain = open(tmp_path / "cohort.vcf", "rb").read()
    os.remove(tmp_path / "cohort.vcf")
    o.bgzip_output = True
    path = SVIM_MERGE.write_cohort_vcf(merged, G, SAMPLES, "1.0.3", TYPES, FastaFile(REF), o)
    assert sorted(os.listdir(tmp_path)) == ["cohort.vcf.gz", "cohort.vcf.gz.tbi"]
    blob = open(path, "rb").read()
    text = gzip.decompress(blob)
    mask = lambda b: b"\n".join(l for l in b.split(b"\n") if not l.startswith(b"##fileDate="))
    assert mask(text) == mask(plain)
    tabix_reader.check_bgzf(blob, text)
    reader = tabix_reader.Reader(blob, open(path + ".tbi", "rb").read())
    for name in [x.decode() for x in reader.index.names]:
        assert reader.query(name, 0, 1 << 31) == tabix_reader.brute(text, name, 0, 1 << 31)
        assert reader.query(name, 89000, 91000) == tabix_reader.brute(text, name, 89000, 91000)


# ------------------------------------------------------------------------------ the command and --keep_candidates
def _diploid(wd, *extra):
    from svim_asm_amd import cli
    cli.main(["diploid", str(wd), os.path.join(GOLD, "hap1.bam"), os.path.join(GOLD, "hap2.bam"), REF] + list(extra))


def test_keep_candidates_writes_the_table_the_vcf_was_written_from(tmp_path, monkeypatch):
    helpers.oracle_backed_device(monkeypatch)
    seen = []
    real = SVIM_COMBINE.write_vcf_table
    from svim_asm_amd import cli
    monkeypatch.setattr(cli, "write_vcf_table", lambda table, *a, **kw: (seen.append(table), real(table, *a, **kw))[1])
    _diploid(tmp_path / "plain")
    _diploid(tmp_path / "kept", "--keep_candidates")
    names = lambda d: sorted(n for n in os.listdir(d) if not n.endswith(".log"))
    assert names(tmp_path / "plain") == ["variants.vcf"]
    assert names(tmp_path / "kept") == ["candidates.svxt", "variants.vcf"]
    undated = lambda p: [l for l in open(p) if not l.startswith("##fileDate=")]
    assert undated(tmp_path / "kept" / "variants.vcf") == undated(tmp_path / "plain" / "variants.vcf")
    back = CandidateTable.from_wire(open(tmp_path / "kept" / "candidates.svxt", "rb").read())
    assert back.to_wire() == seen[1].to_wire()
    assert [helpers.candidate_tuple(c) for c in back.objects()] == [helpers.candidate_tuple(c) for c in seen[1].objects()]


def test_merge_command_names_what_it_refuses(tmp_path, monkeypatch, capsys, caplog):
    from svim_asm_amd import merge_cli
    helpers.oracle_backed_device(monkeypatch)
    _diploid(tmp_path / "a" / "s", "--keep_candidates")
    _diploid(tmp_path / "b" / "s", "--keep_candidates")
    out = tmp_path / "out"
    assert merge_cli.main([str(out), REF, str(tmp_path / "a" / "s"), str(tmp_path / "b" / "s")]) == 2
    assert "column name s" in capsys.readouterr().err and not out.exists()
    os.rename(tmp_path / "b" / "s", tmp_path / "b" / "t")
    with caplog.at_level(logging.ERROR):
        assert merge_cli.main([str(out), REF, str(tmp_path / "a" / "s"), str(tmp_path / "missing")]) == 1
        whole = open(tmp_path / "b" / "t" / "candidates.svxt", "rb").read()
        open(tmp_path / "b" / "t" / "candidates.svxt", "wb").write(whole[:len(whole) // 2])
        assert merge_cli.main([str(out), REF, str(tmp_path / "a" / "s"), str(tmp_path / "b" / "t")]) == 1
    errors = [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR]
    assert len(errors) == 2 and all("--keep_candidates" in e for e in errors)
    assert str(tmp_path / "missing" / "candidates.svxt") in errors[0] and str(tmp_path / "b" / "t" / "candidates.svxt") in errors[1]
    assert not os.path.exists(out / "cohort.vcf")
    # and what it accepts: a sample merged with itself is homozygous where it was, NS=2 throughout
    open(tmp_path / "b" / "t" / "candidates.svxt", "wb").write(whole)
    manifest = tmp_path / "cohort.tsv"
    manifest.write_text("# a cohort\n%s x.bam y.bam\n%s x.bam y.bam\n" % (tmp_path / "a" / "s", tmp_path / "b" / "t"))
    assert merge_cli.main([str(out), REF, "--manifest", str(manifest)]) == 0
    recs = _records(open(out / "cohort.vcf").read())
    single = _records(open(tmp_path / "a" / "s" / "variants.vcf").read())
    assert [r[:7] for r in recs] == [r[:7] for r in single]
    assert all(r[9] == r[10] == one[9].split(":")[0] and ";NS=2;" in r[7] for r, one in zip(recs, single))


def test_cohort_command_merges_in_the_same_process(tmp_path, monkeypatch):
    """svim-asm-cohort --merge (single process; the device answered by the oracle): every sample keeps its table, the
    VCFs are the ones the command writes without the option, and the cohort file has a column per sample."""
    from svim_asm_amd import cli, cohort
    helpers.oracle_backed_device(monkeypatch)
    monkeypatch.setattr(cli, "_warm_device", lambda device: None)
    bams = os.path.join(GOLD, "hap1.bam"), os.path.join(GOLD, "hap2.bam")
    manifest = tmp_path / "cohort.tsv"
    manifest.write_text("%s %s %s\n%s %s %s\n" % ((tmp_path / "s1",) + bams + (tmp_path / "s2",) + bams[::-1]))
    assert cohort.main(["diploid", str(manifest), REF, "--merge", str(tmp_path / "all")]) == 0
    golden = open(os.path.join(GOLD, "diploid_default.vcf")).read()
    assert "".join(l for l in open(tmp_path / "s1" / "variants.vcf") if not l.startswith("##fileDate=")) == golden
    assert os.path.exists(tmp_path / "s1" / "candidates.svxt") and os.path.exists(tmp_path / "s2" / "candidates.svxt")
    text = open(tmp_path / "all" / "cohort.vcf").read()
    assert [l for l in text.splitlines() if l.startswith("#CHROM")][0].split("\t")[9:] == ["s1", "s2"]
    mirror = {"1/0": "0/1", "0/1": "1/0", "1/1": "1/1"}
    recs = _records(text)
    assert len(recs) == len(_records(golden)) and all(r[10] == mirror[r[9]] and ";NS=2;" in r[7] for r in recs)
    # a sample that fails: no merge
    manifest.write_text("%s %s %s\n" % (tmp_path / "s3", tmp_path / "none.bam", bams[1]))
    try:
        rc = cohort.main(["diploid", str(manifest), REF, "--merge", str(tmp_path / "never")])
    except Exception:  # noqa: BLE001 — a missing BAM may also raise, as it does without the option
        rc = 1
    assert rc != 0 and not os.path.exists(tmp_path / "never" / "cohort.vcf")
