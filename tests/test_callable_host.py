"""--callable_bed where there is no GPU: the kernels answered by the oracle (tests/helpers.OracleBackedContext)
and svx_cover_single by the plain loops of tests/callable_restatement.py — the file of a haploid and of a diploid sample from
all three readers, the filter, the cohort's count track line by line, the options' way through the cohort command, and the
derivation itself: a numpy slot form (the top two end keys of every prefix) against the restatement on every case the
device is held to in tests/test_gpu_callable.py."""
import logging
import os

import numpy as np
import pytest

from svim_asm_amd import SVIM_CALLABLE, SVIM_MERGE, bamio
from tests import callable_cases as K, callable_restatement as R, helpers, paf_writer as pw, sam_text_writer as stw
from tests import test_cover_host as cover_host
from tests.test_cover_host import HAP1, HAP2, REF, listing, python_intervals, run, undated
from tests.test_merge_cohort import _manifest, stub  # noqa: F401 — the stubbed children of --gpus N


def restated_cover_single(self, start_key, end_key, list_off):
    """Context.cover_single answered by the loops of tests/callable_restatement.py."""
    restated_cover_single.calls.append(len(list_off) - 1)
    off = [int(x) for x in list_off]
    pairs = list(zip([int(x) for x in start_key], [int(x) for x in end_key]))
    lo, hi, seg_off = R.flat(R.single([pairs[off[l]:off[l + 1]] for l in range(len(off) - 1)]))
    return np.array(lo, dtype=np.uint64), np.array(hi, dtype=np.uint64), np.array(seg_off, dtype=np.uint64)


restated_cover_single.calls = []


def restated_cover_query(self, *args):
    """tests/test_cover_host.py's stand-in for Context.cover_query, its call count left as that module's tests expect it."""
    calls = cover_host.restated_cover_query.calls
    try:
        return cover_host.restated_cover_query(self, *args)
    finally:
        cover_host.restated_cover_query.calls = calls


@pytest.fixture
def device(monkeypatch):
    monkeypatch.setattr(helpers.OracleBackedContext, "cover_single", restated_cover_single, raising=False)
    monkeypatch.setattr(helpers.OracleBackedContext, "cover_query", restated_cover_query, raising=False)
    restated_cover_single.calls = []
    return helpers.oracle_backed_device(monkeypatch)


CONTIGS = list(bamio.AlignmentFile(HAP1, reader="python").references)


def keyed(intervals, min_length=0):
    return [(R.key(t, s), R.key(t, e)) for t, s, e in intervals if e - s >= min_length]


def expected_set(paths, min_length=0):
    """A sample's callable set by the restatement alone, from the pure-Python reader's intervals."""
    return R.sample_set(R.single([keyed(python_intervals(p), min_length) for p in paths]))


def read(path):
    with open(path) as f:
        return f.read()


# ------------------------------------------------------------------------------ one sample
def test_callable_bed_of_a_haploid_and_a_diploid_sample_from_all_three_readers(tmp_path, device):
    sam1 = stw.bam_as_sam(HAP1, str(tmp_path / "h1.sam"), so="unsorted", shuffle_seed=11)
    sam2 = stw.bam_as_sam(HAP2, str(tmp_path / "h2.sam"), so="unsorted", shuffle_seed=13)
    paf1, query1 = pw.bam_as_paf(HAP1, str(tmp_path / "h1.paf"), str(tmp_path / "q1.fa"), shuffle_seed=12)
    paf2, query2 = pw.bam_as_paf(HAP2, str(tmp_path / "h2.paf"), str(tmp_path / "q2.fa"), shuffle_seed=14)
    haploid = R.bed_text(CONTIGS, expected_set([HAP1]))
    diploid = R.bed_text(CONTIGS, expected_set([HAP1, HAP2]))
    assert haploid.count("\n") > 20 and diploid.count("\n") > 20 and haploid != diploid
    for name, argv in (("bam", [HAP1]), ("sam", [sam1]), ("paf", [paf1, "--query", query1])):
        run(["haploid", str(tmp_path / ("h_" + name)), argv[0], REF] + argv[1:] + ["--callable_bed"])
        assert listing(tmp_path / ("h_" + name)) == ["callable.bed", "variants.vcf"]
        assert read(tmp_path / ("h_" + name) / "callable.bed") == haploid, name
    for name, argv in (("bam", [HAP1, HAP2]), ("sam", [sam1, sam2]), ("paf", [paf1, paf2, "--query1", query1, "--query2", query2])):
        run(["diploid", str(tmp_path / ("d_" + name)), argv[0], argv[1], REF] + argv[2:] + ["--callable_bed"])
        assert listing(tmp_path / ("d_" + name)) == ["callable.bed", "variants.vcf"]
        assert read(tmp_path / ("d_" + name) / "callable.bed") == diploid, name
    # ONE device call per sample: 1 list for a haploid run, 2 for a diploid one
    assert restated_cover_single.calls == [1, 1, 1, 2, 2, 2]
    # three columns, 0-based half-open, the header's contig order and then start; a line lies inside ONE alignment per haplotype
    rows = [l.split("\t") for l in diploid.splitlines()]
    assert all(len(r) == 3 and int(r[1]) < int(r[2]) for r in rows)
    assert [(CONTIGS.index(r[0]), int(r[1])) for r in rows] == sorted((CONTIGS.index(r[0]), int(r[1])) for r in rows)
    for r in rows:
        for path in (HAP1, HAP2):
            over = [iv for iv in python_intervals(path) if CONTIGS[iv[0]] == r[0] and iv[1] < int(r[2]) and iv[2] > int(r[1])]
            assert len(over) == 1 and over[0][1] <= int(r[1]) and over[0][2] >= int(r[2])


def test_callable_min_length_leaves_the_short_alignments_out(tmp_path, device):
    lengths = sorted(e - s for _, s, e in python_intervals(HAP1) + python_intervals(HAP2))
    n = lengths[len(lengths) // 3] + 1
    assert lengths[0] < n <= lengths[-1]
    run(["diploid", str(tmp_path / "all"), HAP1, HAP2, REF, "--callable_bed"])
    run(["diploid", str(tmp_path / "long"), HAP1, HAP2, REF, "--callable_bed", "--callable_min_length", str(n)])
    filtered = R.bed_text(CONTIGS, expected_set([HAP1, HAP2], n))
    assert read(tmp_path / "long" / "callable.bed") == filtered != read(tmp_path / "all" / "callable.bed")
    assert undated(tmp_path / "long" / "variants.vcf") == undated(tmp_path / "all" / "variants.vcf")  # the calls see every alignment
    assert run(["diploid", str(tmp_path / "neg"), HAP1, HAP2, REF, "--callable_bed", "--callable_min_length", "-1"]) == 2


def test_the_other_outputs_do_not_change_with_the_option(tmp_path, device):
    run(["diploid", str(tmp_path / "plain"), HAP1, HAP2, REF, "--keep_candidates", "--keep_coverage"])
    run(["diploid", str(tmp_path / "bed"), HAP1, HAP2, REF, "--keep_candidates", "--keep_coverage", "--callable_bed"])
    run(["diploid", str(tmp_path / "table"), HAP1, HAP2, REF, "--keep_candidates", "--callable_bed"])
    assert listing(tmp_path / "plain") == ["candidates.svxt", "coverage.svxt", "variants.vcf"]
    assert listing(tmp_path / "bed") == ["callable.bed", "candidates.svxt", "coverage.svxt", "variants.vcf"]
    assert listing(tmp_path / "table") == ["callable.bed", "candidates.svxt", "variants.vcf"]  # coverage.svxt only if asked for
    for name in ("candidates.svxt", "coverage.svxt"):
        assert open(tmp_path / "bed" / name, "rb").read() == open(tmp_path / "plain" / name, "rb").read()
    assert open(tmp_path / "table" / "candidates.svxt", "rb").read() == open(tmp_path / "plain" / "candidates.svxt", "rb").read()
    assert undated(tmp_path / "bed" / "variants.vcf") == undated(tmp_path / "plain" / "variants.vcf") == undated(tmp_path / "table" / "variants.vcf")
    assert read(tmp_path / "bed" / "callable.bed") == read(tmp_path / "table" / "callable.bed")
    assert restated_cover_single.calls == [2, 2]


def test_a_sharded_run_refuses_callable_bed_by_name(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    assert run(["diploid", str(tmp_path / "wd"), HAP1, HAP2, REF, "--callable_bed"]) == 2
    err = capsys.readouterr().err
    assert "--callable_bed is not available in a sharded run (WORLD_SIZE=2)" in err and not os.path.exists(tmp_path / "wd")


# ------------------------------------------------------------------------------ the cohort
@pytest.fixture
def cohort(tmp_path, device):
    """s1 = (hap1, hap2), s2 = (hap2, hap1), s3 = haploid on hap1 alone, each with its table and its coverage."""
    dirs = [str(tmp_path / n) for n in ("s1", "s2", "s3")]
    run(["diploid", dirs[0], HAP1, HAP2, REF, "--keep_candidates", "--keep_coverage"])
    run(["diploid", dirs[1], HAP2, HAP1, REF, "--keep_candidates", "--keep_coverage"])
    run(["haploid", dirs[2], HAP1, REF, "--keep_candidates", "--keep_coverage"])
    return dirs


def expected_track(min_length=0):
    sets = [expected_set([HAP1, HAP2], min_length), expected_set([HAP2, HAP1], min_length), expected_set([HAP1], min_length)]
    return R.count_track(sets)


def test_merge_writes_the_cohorts_count_track_as_the_restatement_does(tmp_path, cohort, device):
    from svim_asm_amd import merge_cli
    assert merge_cli.main([str(tmp_path / "plain"), REF] + cohort) == 0
    assert restated_cover_single.calls == [] and listing(tmp_path / "plain") == ["cohort.vcf"]
    assert merge_cli.main([str(tmp_path / "bed"), REF] + cohort + ["--callable_bed"]) == 0
    assert restated_cover_single.calls == [5]  # all lists of all samples: ONE call
    assert listing(tmp_path / "bed") == ["cohort.callable.bed", "cohort.vcf"]
    assert undated(tmp_path / "bed" / "cohort.vcf") == undated(tmp_path / "plain" / "cohort.vcf")
    track = expected_track()
    text = read(tmp_path / "bed" / "cohort.callable.bed")
    assert text == R.bed_text(CONTIGS, track)
    # s1 and s2 have one set and s3's contains it: all three or s3 alone; no line without a sample, equal neighbours joined
    assert {n for _, _, n in track} == {1, 3}
    rows = [l.split("\t") for l in text.splitlines()]
    assert all(len(r) == 4 and int(r[3]) >= 1 for r in rows)
    assert not any(a[0] == b[0] and a[2] == b[1] and a[3] == b[3] for a, b in zip(rows, rows[1:]))
    # the filter, and together with the genotypes: still one call each
    n = sorted(e - s for _, s, e in python_intervals(HAP1))[10] + 1
    assert merge_cli.main([str(tmp_path / "long"), REF] + cohort + ["--callable_bed", "--callable_min_length", str(n),
                                                                   "--genotype_non_carriers"]) == 0
    assert restated_cover_single.calls == [5, 5]
    assert read(tmp_path / "long" / "cohort.callable.bed") == R.bed_text(CONTIGS, expected_track(n)) != text
    assert merge_cli.main([str(tmp_path / "gt"), REF] + cohort + ["--genotype_non_carriers"]) == 0
    assert undated(tmp_path / "long" / "cohort.vcf") == undated(tmp_path / "gt" / "cohort.vcf")


def test_merge_names_a_missing_coverage_file(tmp_path, cohort, device, caplog):
    from svim_asm_amd import merge_cli
    os.remove(os.path.join(cohort[1], "coverage.svxt"))
    with caplog.at_level(logging.ERROR):
        assert merge_cli.main([str(tmp_path / "out"), REF] + cohort + ["--callable_bed"]) == 1
    errors = [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR]
    assert len(errors) == 1 and os.path.join(cohort[1], "coverage.svxt") in errors[0] and "--keep_coverage" in errors[0]
    assert not os.path.exists(tmp_path / "out" / "cohort.vcf") and not os.path.exists(tmp_path / "out" / "cohort.callable.bed")


def test_a_coverage_file_of_another_reference_is_refused(tmp_path, cohort, device, caplog):
    from svim_asm_amd import merge_cli
    cov = SVIM_MERGE.read_coverage(cohort[2])
    SVIM_MERGE.keep_coverage(cov.contigs, cov.contig_len - 1, cov.lists, cohort[2])
    with caplog.at_level(logging.ERROR):
        assert merge_cli.main([str(tmp_path / "out"), REF] + cohort + ["--callable_bed"]) == 1
    assert any("coverage of sample s3" in r.getMessage() for r in caplog.records)
    assert restated_cover_single.calls == []


def test_cohort_command_passes_the_options_on(tmp_path, device, monkeypatch):
    """svim-asm-cohort (single process): callable.bed for every sample; with --merge OUT also --keep_coverage for the samples
    and the merge with both options."""
    from svim_asm_amd import cli, cohort as cohort_cmd
    monkeypatch.setattr(cli, "_warm_device", lambda device: None)
    manifest = tmp_path / "cohort.tsv"
    manifest.write_text("%s %s %s\n%s %s %s\n" % (tmp_path / "s1", HAP1, HAP2, tmp_path / "s2", HAP2, HAP1))
    assert cohort_cmd.main(["diploid", str(manifest), REF, "--callable_bed"]) == 0
    diploid = R.bed_text(CONTIGS, expected_set([HAP1, HAP2]))
    for s in ("s1", "s2"):
        assert listing(tmp_path / s) == ["callable.bed", "variants.vcf"]
        assert read(tmp_path / s / "callable.bed") == diploid  # (an intersection: the order of the haplotypes does not matter)
    assert restated_cover_single.calls == [2, 2]
    n = sorted(e - s for _, s, e in python_intervals(HAP1))[10] + 1
    assert cohort_cmd.main(["diploid", str(manifest), REF, "--merge", str(tmp_path / "all"), "--callable_bed",
                            "--callable_min_length", str(n)]) == 0
    for s in ("s1", "s2"):
        assert listing(tmp_path / s) == ["callable.bed", "candidates.svxt", "coverage.svxt", "variants.vcf"]
        assert read(tmp_path / s / "callable.bed") == R.bed_text(CONTIGS, expected_set([HAP1, HAP2], n))
    assert restated_cover_single.calls == [2, 2, 2, 2, 4]
    both = [expected_set([HAP1, HAP2], n)] * 2
    assert read(tmp_path / "all" / "cohort.callable.bed") == R.bed_text(CONTIGS, R.count_track(both))
    # the argument lists
    rest, extra = cohort_cmd._take_callable(["--min_mapq", "30", "--callable_min_length", "70", "--callable_bed"], True)
    assert rest == ["--min_mapq", "30", "--callable_min_length", "70", "--callable_bed", "--keep_coverage"]
    assert extra == ["--callable_bed", "--callable_min_length", "70"]
    assert cohort_cmd._take_callable(["--callable_bed", "--keep_coverage"], True) == (["--callable_bed", "--keep_coverage"], ["--callable_bed"])
    assert cohort_cmd._take_callable(["--callable_bed"], False) == (["--callable_bed"], [])
    assert cohort_cmd._take_callable(["--verbose"], True) == (["--verbose"], [])


def test_the_children_of_gpus_n_and_the_merge_child_get_the_options(tmp_path, stub):  # noqa: F811
    from svim_asm_amd import cohort as cohort_cmd
    set_plan, records = stub
    assert cohort_cmd.main(["diploid", _manifest(tmp_path, 4), "ref.fa", "--gpus", "2", "--callable_bed", "--callable_min_length", "500"]) == 0
    children = records("child")
    assert len(children) == 2 and records("merge") == []
    for rec in children:
        a = rec["argv"]
        assert a.count("--callable_bed") == 1 and a[a.index("--callable_min_length") + 1] == "500" and "--keep_coverage" not in a
    assert cohort_cmd.main(["diploid", _manifest(tmp_path, 4), "ref.fa", "--gpus", "2", "--merge", str(tmp_path / "m"), "--callable_bed",
                            "--callable_min_length", "500", "--genotype_non_carriers"]) == 0
    children, merges = records("child"), records("merge")
    assert len(children) == 4 and len(merges) == 1
    for rec in [r for r in children if "--keep_coverage" in r["argv"]]:  # (the two of this run)
        a = rec["argv"]
        assert a.count("--callable_bed") == 1 and a.count("--keep_coverage") == 1 and a.count("--keep_candidates") == 1
        assert a[a.index("--callable_min_length") + 1] == "500" and "--genotype_non_carriers" not in a
    assert sum("--keep_coverage" in r["argv"] for r in children) == 2
    m = merges[0]["argv"]
    assert m.count("--callable_bed") == 1 and m[m.index("--callable_min_length") + 1] == "500" and "--genotype_non_carriers" in m
    assert "--keep_coverage" not in m and "--keep_candidates" not in m


# ------------------------------------------------------------------------------ host arithmetic on hand-built sets
def as_arrays(segs):
    return np.array([a for a, _ in segs], dtype=np.uint64), np.array([b for _, b in segs], dtype=np.uint64)


def as_tuples(*cols):
    return list(zip(*[np.asarray(c).tolist() for c in cols]))


def test_intersection_and_count_track_equal_the_restatement():
    import random
    rng = random.Random(41)

    def disjoint(n):
        cuts = sorted(rng.sample(range(1, 4000), 2 * n))
        # (some abut: a cut used as an end and as the next start)
        segs = [(cuts[2 * k], cuts[2 * k + 1]) for k in range(n)]
        return [(a, b) if rng.random() < 0.7 or k + 1 == n else (a, segs[k + 1][0]) for k, (a, b) in enumerate(segs)]
    sets = [disjoint(rng.randrange(1, 60)) for _ in range(7)] + [[]]
    for a in sets:
        for b in sets:
            assert as_tuples(*SVIM_CALLABLE.intersect(as_arrays(a), as_arrays(b))) == R.intersect(a, b)
    assert as_tuples(*SVIM_CALLABLE.count_track([as_arrays(s) for s in sets])) == R.count_track(sets)
    assert as_tuples(*SVIM_CALLABLE.count_track([])) == [] == as_tuples(*SVIM_CALLABLE.count_track([as_arrays([])]))
    # abutting segments of ONE sample stay two lines in its own set and are one range of the track
    two = [(10, 20), (20, 30)]
    assert as_tuples(*SVIM_CALLABLE.sample_set([as_arrays(two)])) == two
    assert as_tuples(*SVIM_CALLABLE.count_track([as_arrays(two)])) == [(10, 30, 1)] == R.count_track([two])
    assert as_tuples(*SVIM_CALLABLE.intersect(as_arrays(two), as_arrays([(5, 25)]))) == [(10, 20), (20, 25)]


def test_keys_of_filters_by_reference_length():
    lists = [(np.array([0, 0, 2]), np.array([5, 50, 7]), np.array([25, 60, 1007])), (np.zeros(0), np.zeros(0), np.zeros(0))]
    start, end, off = SVIM_CALLABLE.keys_of(lists, 0)
    assert start.tolist() == [R.key(0, 5), R.key(0, 50), R.key(2, 7)] and end.tolist() == [R.key(0, 25), R.key(0, 60), R.key(2, 1007)]
    assert off.tolist() == [0, 3, 3] and start.dtype == end.dtype == off.dtype == np.uint64
    start, end, off = SVIM_CALLABLE.keys_of(lists, 20)
    assert start.tolist() == [R.key(0, 5), R.key(2, 7)] and off.tolist() == [0, 2, 2]


# ------------------------------------------------------------------------------ the derivation and the device's cases
def slot_form(entries):
    """The argument of svx_cover_single in numpy: slot k = [s_k, s_k+1) (the last one open), m1 >= m2 the two largest end
    keys of entries 0..k — m1 the running maximum, m2 the running maximum of what lost against it: min(e_k, m1_k-1) —,
    depth 1 exactly on [max(s_k, m2), min(s_k+1, m1))."""
    if not entries:
        return []
    s = np.array([a for a, _ in entries], dtype=np.uint64)
    e = np.array([b for _, b in entries], dtype=np.uint64)
    m1 = np.maximum.accumulate(e)
    m2 = np.maximum.accumulate(np.minimum(e, np.concatenate([np.zeros(1, np.uint64), m1[:-1]])))
    lo = np.maximum(s, m2)
    hi = np.minimum(np.concatenate([s[1:], np.full(1, np.iinfo(np.uint64).max, np.uint64)]), m1)
    keep = lo < hi
    return list(zip(lo[keep].tolist(), hi[keep].tolist()))


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_the_slot_form_equals_the_restatement_on_every_device_case(name):
    lists = K.CASES[name]()
    K.check_inputs(lists)
    assert R.flat([slot_form(ivs) for ivs in lists]) == K.answers(name)
    assert all(len(slot_form(ivs)) <= len(ivs) for ivs in lists)


@pytest.mark.parametrize("name", sorted(K.MIXED))
def test_the_mixed_cases_are_balanced(name):
    assert K.is_balanced(name)


def test_the_targeted_cases_pin_what_they_are_named_after():
    lo, hi, off = K.answers("disjoint")
    assert off == [0] + list(np.cumsum([len(l) for l in K.disjoint()]))  # every slot a segment
    assert list(zip(lo, hi))[:len(K.disjoint()[0])] == K.disjoint()[0]
    assert K.answers("duplicated") == ([], [], [0, 0, 0, 0])
    lo, hi, off = K.answers("abutting")
    assert list(zip(lo, hi)) == K.abutting()[0] + K.abutting()[1] and all(a == b for a, b in zip(hi[:299], lo[1:300]))
    assert R.single_one(K.nested()[0]) == [(R.key(0, 0), R.key(0, 10)), (R.key(0, 20), R.key(0, 100))]
    assert len(R.single_one(K.nested()[1])) == 301
    groups = {}
    for s, e in K.equal_starts()[0]:
        groups.setdefault(s, []).append(e)
    assert R.single_one(K.equal_starts()[0]) == [(s if len(es) == 1 else sorted(es)[-2], max(es)) for s, es in sorted(groups.items())]
    assert any(es[0] == max(es) for es in groups.values() if len(es) > 2) and any(es[-1] == max(es) for es in groups.values() if len(es) > 2)
    (two,), (one,) = K.carry_two_long(), K.carry_one_long()
    assert len(two) == len(one) == 2 * K.CHUNK + 1
    assert R.single_one(two) == [(R.key(0, 0), R.key(0, 5)), (two[0][1], two[1][1])]
    assert R.single_one(one) == [(0, one[1][0])] + [(a[1], b[0]) for a, b in zip(one[1:], one[2:])] + [(one[-1][1], one[0][1])]
    big, small = K.last_slot_only()
    assert R.single_one(big) == [(R.key(0, 35150), R.key(0, 36000))] and R.single_one(small) == [(R.key(2, 9), R.key(2, 10))]
    assert R.single_one(K.contig_border()[0]) == [(R.key(0, 90000), R.key(0, 100000)), (R.key(1, 0), R.key(1, 4000)),
                                                  (R.key(1, 5000), R.key(1, 100000)), (R.key(2, 0), R.key(2, 10))]
    assert R.single_one(K.contig_border()[1]) == [(R.key(0, 10), R.key(0, 99999)), (R.key(1, 0), R.key(1, 1))]
    top, c = (1 << 31) - 1, 1 << 16
    far = R.single_one(K.far()[0])
    assert far[0] == (R.key(0, top - 1), R.key(0, top)) and (R.key(c, top - 5000), R.key(c, top - 1)) in far
    assert [len(ivs) for ivs in K.mixed()] == [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097]
    assert [len(ivs) for ivs in K.empty_between()] == [300, 0, 700]


def test_the_probes_host_sweep_equals_the_restatement():
    from tools import callable_probe
    for name in ("mixed", "nested", "abutting", "duplicated"):
        lists = K.CASES[name]()
        start = np.array([s for ivs in lists for s, _ in ivs], dtype=np.uint64)
        end = np.array([e for ivs in lists for _, e in ivs], dtype=np.uint64)
        off = np.cumsum([0] + [len(ivs) for ivs in lists]).astype(np.uint64)
        lo, hi, seg_off = callable_probe.on_host(start, end, off)
        assert (lo.tolist(), hi.tolist(), seg_off.tolist()) == K.answers(name)
