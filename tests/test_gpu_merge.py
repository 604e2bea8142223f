"""The cohort merge on the device: the hand-built four-sample cohort of tests/test_merge_host.py on the real context
against the plain-Python restatement, and the commands end to end — `svim-asm diploid --keep_candidates` twice on the
config-1 sample (haplotypes as they are, and swapped), then `svim-asm-merge`.  Every command is a fresh process with a
time limit of its own; this process only waits.

The cohort-sized partitions of tests/merge_cases.py — what PAIR's two to ten members never sent through the distance
and linkage kernels —: one partition of 11 to 129 distinct alleles of every type, the cohort with every type and size
in one call, a partition whose window is 10 kb wide, the chunked distance path with a worker thread on the context,
both sides of the recipes' thread switch, and the merged cohort through the device BGZF encoder.  Each is held to the
restatement in records, genotype matrix AND the condensed distance vectors handed to the linkage call; every
comparison is exact."""
import gzip
import os
import subprocess
import sys

import pytest

from svim_asm_amd import _lib, SVIM_COMBINE, SVIM_MERGE
from svim_asm_amd.fasta import FastaFile
from tests import merge_cases as M, tabix_reader, test_merge_host as host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "config1")


def test_hand_built_cohort_equals_the_restatement(svx_ctx):
    got = host.both(host.hand_built_cohort(), ctx=svx_ctx)
    assert len({k[0] for k, _ in got}) == 6


@pytest.mark.parametrize("group_min", [0, 2, _lib.LINKAGE_LANES_ONLY])
def test_a_partition_of_twelve_on_either_linkage_kernel(svx_ctx, group_min):
    svx_ctx.set_linkage_group_min(group_min)
    try:
        got = host.both(host.twelve(), ctx=svx_ctx, max_edit_distance=90)
    finally:
        svx_ctx.set_linkage_group_min(0)
    assert 1 < len(got) < 12


SIZED = [(t, n) for t in ("DEL", "INS") for n in M.SIZES] + [(t, n) for t in ("INV", "DUP_TAN", "DUP_INT") for n in (17, 33)] + \
    [("BND", 33), ("BND", 129)]


@pytest.mark.parametrize("case", SIZED, ids=lambda c: "%s-%d" % c)
def test_one_partition_beyond_ten_members(svx_ctx, case):
    got, proxy = M.check(case, svx_ctx)
    n = case[1]
    assert [sizes.tolist() for _, sizes, _ in proxy.linkage] == [[n]]
    assert proxy.distance_jobs == ([] if case[0] == "BND" else [n * (n - 1) // 2])


@pytest.mark.parametrize("n", [17, 33])
@pytest.mark.parametrize("typ", M.TYPES)
def test_the_same_partitions_on_the_lane_kernel(svx_ctx, typ, n):
    svx_ctx.set_linkage_group_min(_lib.LINKAGE_LANES_ONLY)
    try:
        M.check((typ, n), svx_ctx)
    finally:
        svx_ctx.set_linkage_group_min(0)


def test_every_type_and_partition_size_in_one_call(svx_ctx):
    """The non-breakend linkage call mixes the lane kernel, its HBM-scratch form and four classes of the group kernel."""
    got, proxy = M.check("everything", svx_ctx)
    assert len({k[0] for k, _ in got}) == 6
    assert {3, 10, 11, 15, 16, 17, 33, 65, 129} <= set(proxy.linkage[0][1].tolist())


def test_a_partition_with_a_window_of_ten_kilobases(svx_ctx):
    M.check("wide", svx_ctx)


@pytest.mark.parametrize("n", [128, 129])
def test_both_sides_of_the_recipes_thread_switch(svx_ctx, n):
    """svx_pair_recipes splits its jobs over threads from 8192 on: 128 alleles are 8128 jobs, 129 are 8256."""
    got, proxy = M.check(("DEL", n), svx_ctx)
    assert proxy.distance_jobs == [n * (n - 1) // 2] and (proxy.distance_jobs[0] >= 8192) == (n == 129)


@pytest.mark.parametrize("n_chunks", [2, 3])
def test_chunked_distance_jobs_with_a_worker_thread_on_the_context(svx_ctx, monkeypatch, n_chunks):
    monkeypatch.setattr(SVIM_COMBINE, "_PAIR_CHUNK_MIN_JOBS", 1)
    monkeypatch.setattr(SVIM_COMBINE, "_PAIR_CHUNKS", n_chunks)
    got, proxy = M.check("chunks", svx_ctx)
    assert len(proxy.distance_jobs) == 2 and sum(proxy.distance_jobs) == sum(len(c) for _, _, c in M.expected("chunks")[1])


def test_merged_cohort_through_the_device_bgzf_encoder(svx_ctx, tmp_path, monkeypatch):
    """tests/test_merge_host.py's --bgzip_output assertions with the encoder on the device, on the cohort with every type."""
    monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", "1")
    merged, G, o, _ = M.merged("everything", svx_ctx)
    o.working_dir = str(tmp_path)
    SVIM_MERGE.write_cohort_vcf(merged, G, host.SAMPLES, "1.0.3", host.TYPES, FastaFile(host.REF), o, ctx=svx_ctx)
    plain = open(tmp_path / "cohort.vcf", "rb").read()
    os.remove(tmp_path / "cohort.vcf")
    o.bgzip_output = True
    path = SVIM_MERGE.write_cohort_vcf(merged, G, host.SAMPLES, "1.0.3", host.TYPES, FastaFile(host.REF), o, ctx=svx_ctx)
    assert sorted(os.listdir(tmp_path)) == ["cohort.vcf.gz", "cohort.vcf.gz.tbi"]
    blob = open(path, "rb").read()
    text = gzip.decompress(blob)
    mask = lambda b: b"\n".join(l for l in b.split(b"\n") if not l.startswith(b"##fileDate="))
    assert mask(text) == mask(plain)
    assert {l.split(b"\t")[2].split(b".")[1] for l in text.split(b"\n") if l and not l.startswith(b"#")} == \
        {b"DEL", b"INS", b"INV", b"DUP_TANDEM", b"DUP_INT", b"BND"}
    tabix_reader.check_bgzf(blob, text)
    reader = tabix_reader.Reader(blob, open(path + ".tbi", "rb").read())
    assert len(reader.index.names) == 3
    for name in [x.decode() for x in reader.index.names]:
        assert reader.query(name, 0, 1 << 31) == tabix_reader.brute(text, name, 0, 1 << 31)
        for lo in (20000, 30000, 40000, 60000, 89000, 120000):
            assert reader.query(name, lo, lo + 2000) == tabix_reader.brute(text, name, lo, lo + 2000)


def _run(argv, timeout=120):
    env = dict(os.environ)
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SVX_NODE_PROCESSES"):
        env.pop(name, None)
    r = subprocess.run([sys.executable] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _records(path):
    return [l.rstrip("\n").split("\t") for l in open(path) if not l.startswith("#")]


@pytest.mark.spawns_gpu_children
def test_commands_end_to_end_on_a_sample_and_its_mirror_image(tmp_path):
    h1, h2, ref = (os.path.join(GOLD, n) for n in ("hap1.bam", "hap2.bam", "ref.fa"))
    as_is, swapped = str(tmp_path / "as_is"), str(tmp_path / "swapped")
    _run([os.path.join(ROOT, "bin", "svim-asm"), "diploid", as_is, h1, h2, ref, "--keep_candidates"])
    _run([os.path.join(ROOT, "bin", "svim-asm"), "diploid", swapped, h2, h1, ref, "--keep_candidates"])
    _run([os.path.join(ROOT, "bin", "svim-asm-merge"), str(tmp_path / "out"), ref, as_is, swapped])
    masked = "".join(l for l in open(os.path.join(as_is, "variants.vcf")) if not l.startswith("##fileDate="))
    assert masked == open(os.path.join(GOLD, "diploid_default.vcf")).read()
    # the swapped sample is the golden one with the haplotypes exchanged: same number of calls of every genotype class
    mirror = {"1/0": "0/1", "0/1": "1/0", "1/1": "1/1"}
    count = lambda path: sorted((r[2].split(".")[1], r[-1].split(":")[0]) for r in _records(path))
    assert count(os.path.join(swapped, "variants.vcf")) == sorted((t, mirror[g]) for t, g in count(os.path.join(as_is, "variants.vcf")))
    header = [l for l in open(tmp_path / "out" / "cohort.vcf") if l.startswith("#CHROM")]
    assert header[0].rstrip("\n").split("\t")[9:] == ["as_is", "swapped"]
    recs = _records(tmp_path / "out" / "cohort.vcf")
    assert len(recs) == len(_records(os.path.join(as_is, "variants.vcf")))
    for r in recs:
        assert r[8] == "GT" and r[10] == mirror[r[9]], r
        assert ";NS=2;" in r[7], r
