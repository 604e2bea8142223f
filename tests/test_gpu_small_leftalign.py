"""svim-asm-small --left_align end to end on the device: the commands of tests/test_small_leftalign_host.py with the real
kernels (svx_indel_shift on the pool of bases svx_cigar_mismatch compares), files equal to what tests/small_restatement.py
writes for the alignments with every small gap moved in the CIGAR."""
import pytest

from tests import test_small_host as host, test_small_leftalign_host as la

pytestmark = pytest.mark.gpu


def test_golden_diploid_and_batches_left_aligned_on_the_device(tmp_path, svx_ctx):
    from svim_asm_amd import small_cli
    assert small_cli.main([str(tmp_path / "d"), host.REF, host.HAP1, host.HAP2, "--left_align"]) == 0
    summary = la.check_outputs(str(tmp_path / "d"), la.golden_left_aligned())
    assert [(h["left_aligned"], h["shifted_bases"]) for h in summary["haplotypes"]] == [(52, 66), (44, 61)]
    assert small_cli.main([str(tmp_path / "b"), host.REF, host.HAP1, host.HAP2, "--left_align", "--batch_bases", "100000"]) == 0
    la.check_outputs(str(tmp_path / "b"), la.golden_left_aligned())


def test_the_repeat_pair_on_the_device(tmp_path, svx_ctx):
    h1, h2 = la.repeat_pair()
    _, plain, _ = la.run_command(tmp_path, "plain", h1, h2)
    assert len(plain) == 4 and "1|1" not in [r[3] for r in plain]
    out, moved, _ = la.run_command(tmp_path, "moved", h1, h2, ["--left_align"])
    assert [(r[0], r[3]) for r in moved] == [(la.RUNS[0][0], "1|1"), (la.RUNS[1][0], "1|1")]
    la.check_outputs(out, la.expectation_of([h1, h2]))
