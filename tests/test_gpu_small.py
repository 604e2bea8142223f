"""svim-asm-small end to end on the device: the config1 commands of tests/test_small_host.py with the real kernels
(svx_cigar_mismatch over the readers' CIGAR pools in HBM, svx_cigar_extract, svx_cover_single, the BGZF encoder), files
byte-identical to what tests/small_restatement.py writes."""
import os
import subprocess
import sys

import pytest

from tests import paf_writer as pw, sam_text_writer as stw, small_restatement as SR, tabix_reader as TR, test_small_host as host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_golden_diploid_haploid_sam_and_paf_in_this_process(tmp_path, svx_ctx):
    from svim_asm_amd import small_cli
    assert small_cli.main([str(tmp_path / "d"), host.REF, host.HAP1, host.HAP2]) == 0
    host.check_outputs(str(tmp_path / "d"), host.golden_expectation())
    assert small_cli.main([str(tmp_path / "h"), host.REF, host.HAP1, "--sample", "only"]) == 0
    host.check_outputs(str(tmp_path / "h"), host.golden_expectation(haploid=True, sample="only"))
    sam = stw.bam_as_sam(host.HAP1, str(tmp_path / "h1.sam"), so="unsorted", shuffle_seed=11)
    paf, query = pw.bam_as_paf(host.HAP2, str(tmp_path / "h2.paf"), str(tmp_path / "q2.fa"), shuffle_seed=12)
    assert small_cli.main([str(tmp_path / "t"), host.REF, sam, paf, "--query2", query]) == 0
    host.check_outputs(str(tmp_path / "t"), host.golden_expectation())


def test_several_batches_on_the_device(tmp_path, svx_ctx):
    from svim_asm_amd import small_cli
    assert small_cli.main([str(tmp_path / "b"), host.REF, host.HAP1, host.HAP2, "--batch_bases", "100000"]) == 0
    host.check_outputs(str(tmp_path / "b"), host.golden_expectation())


def test_bgzip_output_on_the_device(tmp_path, svx_ctx, monkeypatch):
    from svim_asm_amd import small_cli
    monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", "1")
    out = str(tmp_path / "z")
    assert small_cli.main([out, host.REF, host.HAP1, host.HAP2, "--bgzip_output"]) == 0
    assert sorted(os.listdir(out)) == ["small.vcf.gz", "small.vcf.gz.tbi", "summary.json"]
    text = host.golden_expectation()[0].encode()
    blob = open(os.path.join(out, "small.vcf.gz"), "rb").read()
    TR.check_bgzf(blob, text)
    reader = TR.Reader(blob, open(os.path.join(out, "small.vcf.gz.tbi"), "rb").read())
    for name, beg, end in (("chr1", 0, 1 << 29), ("chr2", 100000, 300000), ("chr10", 0, 5000)):
        assert reader.query(name, beg, end) == TR.brute(text, name, beg, end)
    assert open(os.path.join(out, "summary.json")).read() == host.golden_expectation()[1]


def test_made_up_records_on_the_device(tmp_path, svx_ctx):
    from svim_asm_amd import small_cli
    h1, h2 = host.made_up()
    sam1, sam2 = host.sam_of(str(tmp_path / "h1.sam"), h1, no_sequence=(5,)), host.sam_of(str(tmp_path / "h2.sam"), h2)
    h1[5] = h1[5][:3] + ("",)
    SR.write(str(tmp_path / "expected"), [h1, h2], host.SEQS, host.NAMES)
    assert small_cli.main([str(tmp_path / "out"), host.REF, sam1, sam2]) == 0
    for name in ("small.vcf", "summary.json"):
        assert open(str(tmp_path / "out" / name)).read() == open(str(tmp_path / "expected" / name)).read()


@pytest.mark.spawns_gpu_children
def test_the_command_in_a_fresh_process(tmp_path):
    env = dict(os.environ)
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SVX_NODE_PROCESSES"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "svim-asm-small"), str(tmp_path / "out"), host.REF, host.HAP1, host.HAP2],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    host.check_outputs(str(tmp_path / "out"), host.golden_expectation())
