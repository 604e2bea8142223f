"""The cohort merge on the device: the hand-built four-sample cohort of tests/test_merge_host.py on the real context
against the plain-Python restatement, and the commands end to end — `svim-asm diploid --keep_candidates` twice on the
config-1 sample (haplotypes as they are, and swapped), then `svim-asm-merge`.  Every command is a fresh process with a
time limit of its own; this process only waits."""
import os
import subprocess
import sys

import pytest

from svim_asm_amd import _lib
from tests import test_merge_host as host

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
