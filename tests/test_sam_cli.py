"""`svim-asm haploid|diploid` on uncompressed SAM input — records shuffled, no index, any `SO` — writes the VCF the
real reference wrote from the coordinate-sorted, indexed BAMs of the same records (tests/golden/config1).  The device is
answered by the oracle here (as in tests/test_host_pipeline_cpu.py); tests/test_gpu_sam.py runs the real kernels.
The config-1 BAMs hold 38 and 42 records and no two of a file share (tid, pos): the presented order is unique whatever
the shuffle."""
import os

import pytest

from tests import helpers, sam_text_writer as stw
from tests.test_oracle_pins import RUNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "config1")


@pytest.fixture(autouse=True)
def device_is_the_oracle(monkeypatch):
    helpers.oracle_backed_device(monkeypatch)


def _run(tmp_path, name, render):
    """RUNS[name] with every BAM argument replaced by what render(bam path, k) returns; the VCF without its date line."""
    from svim_asm_amd import cli
    argv = list(RUNS[name])
    wd = tmp_path / "wd"
    argv[1] = str(wd)
    k = 0
    for i, a in enumerate(argv):
        if a.endswith(".bam"):
            argv[i] = render(os.path.join(GOLD, a), k)
            k += 1
        elif a.endswith(".fa"):
            argv[i] = os.path.join(GOLD, a)
    cli.main(argv)
    return "".join(l for l in open(wd / "variants.vcf") if not l.startswith("##fileDate="))


def _golden(name):
    return open(os.path.join(GOLD, name + ".vcf")).read()


@pytest.mark.parametrize("name", sorted(RUNS))
def test_cli_on_shuffled_sams_reproduces_reference_vcf_config1(tmp_path, name):
    def render(bam, k):
        sam = stw.bam_as_sam(bam, str(tmp_path / ("in%d.sam" % k)), so="unsorted", shuffle_seed=100 + k)
        assert not os.path.exists(sam + ".bai") and not os.path.exists(sam + ".csi")
        return sam
    assert _run(tmp_path, name, render) == _golden(name)


def test_one_sam_and_one_bam_in_a_diploid_run(tmp_path):
    for which in (0, 1):
        d = tmp_path / ("mix%d" % which)
        d.mkdir()
        got = _run(d, "diploid_default", lambda bam, k: stw.bam_as_sam(bam, str(d / "h.sam"), shuffle_seed=7) if k == which else bam)
        assert got == _golden("diploid_default")


@pytest.mark.parametrize("so", [None, "queryname", "coordinate", "unknown"])
def test_sort_order_header_does_not_matter(tmp_path, so):
    got = _run(tmp_path, "diploid_options", lambda bam, k: stw.bam_as_sam(bam, str(tmp_path / ("s%d.sam" % k)), so=so, shuffle_seed=3 + k))
    assert got == _golden("diploid_options")


def test_crlf_line_ends_are_accepted(tmp_path):
    got = _run(tmp_path, "haploid_default", lambda bam, k: stw.bam_as_sam(bam, str(tmp_path / "crlf.sam"), shuffle_seed=5, eol="\r\n"))
    assert got == _golden("haploid_default")


def test_the_command_says_that_records_were_ordered_in_memory(tmp_path, caplog):
    import logging
    with caplog.at_level(logging.INFO):
        _run(tmp_path, "haploid_default", lambda bam, k: stw.bam_as_sam(bam, str(tmp_path / "a.sam")))
    assert sum("ordered in memory" in r.getMessage() for r in caplog.records) == 1


def test_cohort_manifest_may_name_sams(tmp_path):
    from svim_asm_amd import cohort
    sams = [stw.bam_as_sam(os.path.join(GOLD, "hap%d.bam" % (k + 1)), str(tmp_path / ("c%d.sam" % k)), shuffle_seed=k) for k in range(2)]
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("%s\t%s\t%s\n" % (tmp_path / "out", sams[0], sams[1]))
    assert cohort.main(["diploid", str(manifest), os.path.join(GOLD, "ref.fa")]) in (0, None)
    got = "".join(l for l in open(tmp_path / "out" / "variants.vcf") if not l.startswith("##fileDate="))
    assert got == _golden("diploid_default")
