"""svx_cover_query on the device (svim_asm_amd/csrc/svx_cover.hip) against the plain loops of
tests/cover_restatement.py, element for element, on the cases of tests/cover_cases.py: the wave, workgroup and
chunk-carry edges of the scan in one call of twelve lists, every query count, nested intervals, inclusive bounds, contig
borders, keys up to contig 2^16 and position 2^31 - 1, an empty list between full ones, refused inputs and poisoned
scratch; then the commands end to end with --genotype_non_carriers, held to the expectation of tests/test_cover_host.py."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from svim_asm_amd import SVIM_MERGE, _lib, bamio
from svim_asm_amd.fasta import FastaFile
from tests import cover_cases as K, helpers, test_cover_host as host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arrays(lists, queries):
    start = np.array([s for ivs in lists for s, _ in ivs], dtype=np.uint64)
    end = np.array([e for ivs in lists for _, e in ivs], dtype=np.uint64)
    off = np.zeros(len(lists) + 1, np.uint64)
    np.cumsum([len(ivs) for ivs in lists], out=off[1:])
    return start, end, off, np.array([q[0] for q in queries], dtype=np.uint64), np.array([q[1] for q in queries], dtype=np.uint64)


def on_device(ctx, lists, queries):
    got = ctx.cover_query(*arrays(lists, queries))
    assert got.dtype == np.uint8 and got.shape == (len(lists), len(queries))
    return got.tolist()


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_case_equals_the_restatement(svx_ctx, name):
    lists, queries = K.CASES[name]()
    K.check_inputs(lists, queries)
    expected = K.answers(name)
    assert K.is_balanced(expected)
    assert on_device(svx_ctx, lists, queries) == expected


def test_the_mixed_case_holds_the_edges_of_the_scan():
    sizes = [len(ivs) for ivs in K.mixed()[0]]
    assert len(sizes) == 12 and {0, 1, 63, 64, 65, 255, 256, 257, 1025, 4097, K.CHUNK, K.CHUNK + 1} <= set(sizes)
    assert K.CHUNK == 1024  # SVX_COVER_SCAN_CHUNK: 256 lanes of four entries


@pytest.mark.parametrize("n_q", K.QUERY_COUNTS)
def test_query_counts(svx_ctx, n_q):
    lists, queries = K.mixed()
    expected = [row[:n_q] for row in K.answers("mixed")]
    if n_q:
        assert K.is_balanced(expected)
    assert on_device(svx_ctx, lists, queries[:n_q]) == expected


def test_more_lists_than_one_launch_takes_side_by_side(svx_ctx):
    """GRID_Y + 2 lists: the threads of lists 0 and 1 answer lists GRID_Y and GRID_Y + 1 in a second trip.  Each pair
    answers differently by the restatement, so a trip that is missing or that lands on the first one's row cannot pass."""
    lists, queries = K.many_lists()
    K.check_inputs(lists, queries)
    expected = K.many_lists_answers()
    assert len(lists) == K.GRID_Y + 2 == 65537 and len(queries) == 3 and max(len(ivs) for ivs in lists) == 2
    assert expected[0] != expected[K.GRID_Y] and expected[1] != expected[K.GRID_Y + 1]
    assert all(0 < sum(row[q] for row in expected) < len(lists) for q in range(3))
    got = svx_ctx.cover_query(*arrays(lists, queries))
    assert got.dtype == np.uint8 and got.shape == (len(lists), 3)
    assert np.array_equal(got, np.array(expected, dtype=np.uint8))


def test_queries_are_in_no_order():
    for name in K.CASES:
        los = [q[0] for q in K.CASES[name]()[1]]
        assert los != sorted(los), name


def test_no_lists_and_lists_without_entries(svx_ctx):
    lists, queries = K.mixed()
    assert svx_ctx.cover_query(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(1, np.uint64),
                               *arrays(lists, queries)[3:]).shape == (0, len(queries))
    assert on_device(svx_ctx, [[], [], []], queries[:70]) == [[0] * 70] * 3


@pytest.mark.parametrize("what", ["unsorted list", "interval across contigs", "query across contigs", "lo > hi"])
def test_invalid_inputs_are_refused_and_the_context_stays_usable(svx_ctx, what):
    lists, queries = K.empty_between()
    lists, queries = [list(ivs) for ivs in lists], list(queries)
    if what == "unsorted list":
        lists[2][400], lists[2][401] = lists[2][401], lists[2][400]
        assert lists[2][400][0] > lists[2][401][0]
    elif what == "interval across contigs":
        s, e = lists[0][17]
        lists[0][17] = (s, e + (1 << 32))
    elif what == "query across contigs":
        queries[5] = (queries[5][0], queries[5][1] + (1 << 32))
    else:
        queries[9] = (queries[9][1] + 1, queries[9][1])
    with pytest.raises(_lib.SvxError) as e:
        svx_ctx.cover_query(*arrays(lists, queries))
    assert e.value.status == _lib.SVX_E_INVALID
    assert on_device(svx_ctx, *K.empty_between()) == K.answers("empty_between")


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_answers_do_not_depend_on_what_scratch_held(svx_ctx, byte):
    lists, queries = K.mixed()
    assert on_device(svx_ctx, lists, queries) == K.answers("mixed")  # (the regions exist from here on)
    svx_ctx.scratch_fill(byte)
    assert on_device(svx_ctx, lists, queries) == K.answers("mixed")
    svx_ctx.scratch_fill(byte)
    assert on_device(svx_ctx, *K.nested()) == K.answers("nested")  # a smaller call inside the poisoned regions


# ------------------------------------------------------------------------------ --keep_coverage on the device
def test_ref_len_of_a_cigar_pool_that_is_in_hbm(svx_ctx):
    """Context.cigar_ref_len_dev (svx_cigar_stats_dev on a pool the caller holds in HBM) == cigar_stats == the oracle."""
    from oracle import orc
    from svim_asm_amd import synth
    cig, off, _ = synth.random_cigar_case(np.random.default_rng(23), 700, max_ops=400)
    d_cig = svx_ctx.dev_array(cig)
    got = svx_ctx.cigar_ref_len_dev(d_cig.ptr, len(cig), off)
    assert got.dtype == np.uint32 and len(got) == len(off) - 1 > 600
    assert np.array_equal(got, orc.cigar_stats(cig, off)["ref_len"])
    assert np.array_equal(got, svx_ctx.cigar_stats(cig, off.astype(np.uint64))["ref_len"])
    assert len(svx_ctx.cigar_ref_len_dev(d_cig.ptr, 0, np.zeros(1, np.uint64))) == 0


def test_coverage_from_the_native_reader_in_this_process(svx_ctx):
    """collect_tables with keep_coverage on the golden BAMs (the reader's own copy of the pool where it has one): the
    intervals of the pure-Python reader, and tables equal to a run without the option."""
    from svim_asm_amd import SVIM_COLLECT
    files = [bamio.AlignmentFile(p) for p in (host.HAP1, host.HAP2)]
    tables = SVIM_COLLECT.collect_tables(files, helpers.options(keep_coverage=True), ctx=svx_ctx)
    assert [host.as_tuples(t.coverage) for t in tables] == [host.python_intervals(host.HAP1), host.python_intervals(host.HAP2)]
    plain = SVIM_COLLECT.collect_tables([bamio.AlignmentFile(p) for p in (host.HAP1, host.HAP2)], helpers.options(), ctx=svx_ctx)
    assert [t.to_wire() for t in tables] == [t.to_wire() for t in plain]


# ------------------------------------------------------------------------------ the commands
def _run(argv, timeout=120):
    env = dict(os.environ)
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SVX_NODE_PROCESSES"):
        env.pop(name, None)
    r = subprocess.run([sys.executable] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


@pytest.mark.spawns_gpu_children
def test_commands_end_to_end_genotype_the_non_carriers(tmp_path, svx_ctx, monkeypatch):
    """s1 = (hap1, hap2) and s2 = (hap2, hap1) through `svim-asm-cohort diploid --merge OUT --genotype_non_carriers`, s3 =
    `svim-asm haploid` on hap1 with --keep_coverage (a diploid manifest has no line for it), then the merge command over
    the three: every line is the expectation of tests/test_cover_host.py, plain and through --bgzip_output."""
    names = ["s1", "s2", "s3"]
    dirs = [str(tmp_path / n) for n in names]
    manifest = tmp_path / "cohort.tsv"
    manifest.write_text("%s %s %s\n%s %s %s\n" % (dirs[0], host.HAP1, host.HAP2, dirs[1], host.HAP2, host.HAP1))
    _run([os.path.join(ROOT, "bin", "svim-asm-cohort"), "diploid", str(manifest), host.REF, "--merge", str(tmp_path / "two"),
          "--genotype_non_carriers"])
    _run([os.path.join(ROOT, "bin", "svim-asm"), "haploid", dirs[2], host.HAP1, host.REF, "--keep_candidates", "--keep_coverage"])
    for d in dirs:
        assert host.listing(d) == ["candidates.svxt", "coverage.svxt", "variants.vcf"]
    h1, h2 = host.python_intervals(host.HAP1), host.python_intervals(host.HAP2)
    cov = [SVIM_MERGE.read_coverage(d) for d in dirs]
    assert [host.as_tuples(t) for t in cov[0].lists] == [h1, h2] and [host.as_tuples(t) for t in cov[2].lists] == [h1]
    contigs = list(bamio.AlignmentFile(host.HAP1, reader="python").references)
    haplotypes = [[host.named(h1, contigs), host.named(h2, contigs)], [host.named(h2, contigs), host.named(h1, contigs)],
                  [host.named(h1, contigs)]]
    # the merges in this process (its default context): today's file for both cohorts, the three samples genotyped
    from svim_asm_amd import merge_cli
    assert merge_cli.main([str(tmp_path / "plain3"), host.REF] + dirs) == 0
    assert merge_cli.main([str(tmp_path / "plain2"), host.REF] + dirs[:2]) == 0
    assert merge_cli.main([str(tmp_path / "three"), host.REF] + dirs + ["--genotype_non_carriers"]) == 0
    assert merge_cli.main([str(tmp_path / "gz"), host.REF] + dirs + ["--genotype_non_carriers", "--bgzip_output"]) == 0
    o = helpers.options()
    for n, out, plain in ((3, "three", "plain3"), (2, "two", "plain2")):
        tables = [SVIM_MERGE.read_candidates(d) for d in dirs[:n]]
        merged, G = SVIM_MERGE.merge_tables(tables, names[:n], FastaFile(host.REF), o, ctx=svx_ctx)
        line_rec = host.line_records(merged, names, tmp_path / ("labels%d" % n), monkeypatch)
        texts = host.expected_texts(merged, G, haplotypes[:n], 1000)
        host.check_cohort_vcf(str(tmp_path / out / "cohort.vcf"), str(tmp_path / plain / "cohort.vcf"), merged, texts, line_rec)
        if n == 3:
            assert "0/0" in [t[2] for t in texts]
            # and the matrix itself, on this process's context
            C = SVIM_MERGE.genotype_non_carriers(merged, cov, helpers.options(), svx_ctx, sample_names=names)
            code = {"./.": 0, "0/.": 1, "./0": 2, "0/0": 3}
            for r, (row, text) in enumerate(zip(G.tolist(), texts)):
                for s in range(3):
                    if row[s] == 0:
                        assert int(C[r, s]) == code[text[s]], (r, s)
    text = gzip.decompress(open(tmp_path / "gz" / "cohort.vcf.gz", "rb").read()).decode()
    assert [l for l in text.splitlines(True) if not l.startswith("##fileDate=")] == host.undated(str(tmp_path / "three" / "cohort.vcf"))
    assert os.path.exists(tmp_path / "gz" / "cohort.vcf.gz.tbi")
