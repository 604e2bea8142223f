"""svim-asm-genotype end to end on the device: the config1 commands of tests/test_genotype_host.py with the real
kernels (svx_cover_locate, svx_cigar_lift, the haplotype distances), files byte-identical to what the restatement gives."""
import json
import os
import subprocess
import sys

import pytest

from tests import genotype_restatement as G, paf_writer as pw, sam_text_writer as stw, test_genotype_host as host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(out_dir, sites_path, sites, results, n_hap, sample="Sample"):
    assert open(os.path.join(out_dir, "genotypes.vcf")).read() == G.expected_vcf(sites_path, sites, results, sample)
    summary = json.load(open(os.path.join(out_dir, "summary.json")))
    assert summary["genotyped"] == len(sites) and summary["records"] == host.n_data_lines(sites_path)
    assert summary["haplotypes"] == G.expected_haplotype_counts(results, n_hap)


def test_golden_diploid_haploid_sam_and_paf_in_this_process(tmp_path, svx_ctx):
    from svim_asm_amd import genotype_cli
    sites, results = host.golden_expectation()
    assert genotype_cli.main([str(tmp_path / "d"), host.REF, host.SITES, host.HAP1, host.HAP2]) == 0
    check(str(tmp_path / "d"), host.SITES, sites, results, 2)
    sites1, results1 = host.golden_expectation(haploid=True)
    assert genotype_cli.main([str(tmp_path / "h"), host.REF, host.SITES, host.HAP1, "--sample", "one"]) == 0
    check(str(tmp_path / "h"), host.SITES, sites1, results1, 1, sample="one")
    sam = stw.bam_as_sam(host.HAP1, str(tmp_path / "h1.sam"), so="unsorted", shuffle_seed=11)
    paf, query = pw.bam_as_paf(host.HAP2, str(tmp_path / "h2.paf"), str(tmp_path / "q2.fa"), shuffle_seed=12)
    assert genotype_cli.main([str(tmp_path / "t"), host.REF, host.SITES, sam, paf, "--query2", query]) == 0
    check(str(tmp_path / "t"), host.SITES, sites, results, 2)


def test_made_up_sites_on_the_device(tmp_path, svx_ctx):
    from svim_asm_amd import genotype_cli
    path = host.made_up_vcf(str(tmp_path / "sites.vcf"))
    sites = G.sites_of(path)
    results = G.genotypes(sites, [host.alignments(host.HAP1), host.alignments(host.HAP2)], host.SEQS)
    assert genotype_cli.main([str(tmp_path / "out"), host.REF, path, host.HAP1, host.HAP2]) == 0
    check(str(tmp_path / "out"), path, sites, results, 2)


@pytest.mark.spawns_gpu_children
def test_the_command_in_a_fresh_process(tmp_path):
    env = dict(os.environ)
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SVX_NODE_PROCESSES"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "svim-asm-genotype"), str(tmp_path / "out"), host.REF, host.SITES, host.HAP1,
                        host.HAP2], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    sites, results = host.golden_expectation()
    check(str(tmp_path / "out"), host.SITES, sites, results, 2)
