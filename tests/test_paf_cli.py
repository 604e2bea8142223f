"""`svim-asm haploid|diploid` on minimap2's PAF plus the assembly FASTA (--query / --query1 / --query2) writes the VCF the
real reference wrote from the BAMs of the same alignments (tests/golden/config1).  The conversion is lossless: in both
config-1 BAMs no record has a hard clip, every record carries its full-length SEQ and all records of a query agree on the
query's sequence (tests/paf_writer.alns_of_bam asserts all three), so the goldens are the expected output.  The device is
answered by the oracle here (as in tests/test_sam_cli.py); tests/test_gpu_paf.py runs the real kernels."""
import logging
import os

import pytest

from tests import helpers, paf_writer as pw
from tests.test_oracle_pins import RUNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "config1")


@pytest.fixture(autouse=True)
def device_is_the_oracle(monkeypatch):
    helpers.oracle_backed_device(monkeypatch)


def _run(tmp_path, name, as_paf=(True, True), line=60, bgzip=False, seed=100):
    """RUNS[name] with BAM argument k replaced by a shuffled PAF + its --query FASTA where as_paf[k]."""
    from svim_asm_amd import cli, fasta
    argv = list(RUNS[name])
    wd = tmp_path / "wd"
    argv[1] = str(wd)
    haploid = argv[0] == "haploid"
    k, extra = 0, []
    for i, a in enumerate(argv):
        if a.endswith(".bam"):
            if as_paf[k]:
                paf, fa = pw.bam_as_paf(os.path.join(GOLD, a), str(tmp_path / ("in%d.paf" % k)), str(tmp_path / ("q%d.fa" % k)),
                                        shuffle_seed=seed + k, line=line)
                if bgzip:
                    fa = fasta.bgzip_fasta(fa, fa + ".gz", member_size=4096)
                argv[i] = paf
                extra += ["--query" if haploid else "--query%d" % (k + 1), fa]
            else:
                argv[i] = os.path.join(GOLD, a)
            k += 1
        elif a.endswith(".fa"):
            argv[i] = os.path.join(GOLD, a)
    cli.main(argv + extra)
    return "".join(l for l in open(wd / "variants.vcf") if not l.startswith("##fileDate="))


def _golden(name):
    return open(os.path.join(GOLD, name + ".vcf")).read()


@pytest.mark.parametrize("name", sorted(RUNS))
def test_cli_on_shuffled_pafs_reproduces_reference_vcf_config1(tmp_path, name):
    assert _run(tmp_path, name) == _golden(name)


@pytest.mark.parametrize("which", [0, 1])
def test_one_paf_and_one_bam_in_a_diploid_run(tmp_path, which):
    assert _run(tmp_path, "diploid_default", as_paf=(which == 0, which == 1)) == _golden("diploid_default")


def test_bgzip_compressed_query_assemblies_and_one_line_contigs(tmp_path):
    assert _run(tmp_path, "diploid_default", line=0, bgzip=True, seed=7) == _golden("diploid_default")


def test_the_command_says_where_the_bases_come_from(tmp_path, caplog):
    with caplog.at_level(logging.INFO):
        _run(tmp_path, "haploid_default")
    assert sum("read from the query assembly" in r.getMessage() for r in caplog.records) == 1


def test_query_assembly_without_fai_is_reported(tmp_path, caplog):
    from svim_asm_amd import cli
    paf, fa = pw.bam_as_paf(os.path.join(GOLD, "hap1.bam"), str(tmp_path / "a.paf"), str(tmp_path / "q.fa"))
    os.remove(fa + ".fai")
    with caplog.at_level(logging.ERROR):
        cli.main(["haploid", str(tmp_path / "wd"), paf, os.path.join(GOLD, "ref.fa"), "--query", fa])
    assert any("query assembly is missing an index file" in r.getMessage() for r in caplog.records)
    assert not os.path.exists(tmp_path / "wd" / "variants.vcf")


def test_a_paf_without_query_option_goes_where_it_went_before(tmp_path):
    """No --query: the file takes the path of every non-gzip input, the SAM reader, and its message."""
    from svim_asm_amd import cli
    paf, _ = pw.bam_as_paf(os.path.join(GOLD, "hap1.bam"), str(tmp_path / "a.paf"), str(tmp_path / "q.fa"))
    with pytest.raises(ValueError, match="not a SAM file"):
        cli.main(["haploid", str(tmp_path / "wd"), paf, os.path.join(GOLD, "ref.fa")])
