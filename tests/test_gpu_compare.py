"""svim-asm-compare on the device: tests/test_compare_host.py's `check` — summary, the four VCFs, matches.tsv
and the distance matrices handed to the matching, all against tests/compare_restatement.py — with the real partition,
containment, distance and matching kernels.  The golden call sets, the synthetic pairs, and one case the golden files do
not have: a partition of 40 x 40 insertions and one of 129 deletions a side go through the distance and match kernels
together (the restatement's 18 000 distances of that case come from the oracle's compiled full DP, held to the textbook
recurrence on a sample of them first)."""
import json

import pytest

from tests import compare_cases as K, compare_restatement as R, test_compare_host as host

pytestmark = pytest.mark.gpu


def test_a_file_against_itself(svx_ctx, tmp_path):
    summary, _, _ = host.golden(svx_ctx, "diploid_default.vcf", "diploid_default.vcf", tmp_path, comp_min_sv_size=50)
    assert summary["FP"] == 0 and summary["FN"] == 0 and summary["gt_concordance"] == 1.0 and summary["TP-base"] > 50


@pytest.mark.parametrize("comp", ["diploid_tolerances.vcf", "haploid_default.vcf"])
def test_golden_call_sets_against_each_other(svx_ctx, tmp_path, comp):
    summary, _, _ = host.golden(svx_ctx, "diploid_default.vcf", comp, tmp_path)
    assert summary["TP-base"] > 20


@pytest.mark.parametrize("name", sorted(host.CASES))
def test_synthetic_pairs(svx_ctx, tmp_path, name):
    host.run_case(svx_ctx, name, tmp_path, gz=name == "genotypes")


def test_crowded_partitions_through_distance_and_match_kernels(svx_ctx, tmp_path):
    from oracle import orc
    case = K.crowded_case()
    base, comp, _ = K.write(case, tmp_path / "in")
    # the compiled DP against the textbook recurrence on some of the case's own pairs
    b_rows, c_rows = (R.rows_of(R.parse_vcf(p, K.LEN_OF)) for p in (base, comp))
    for i, j in ((0, 0), (3, 17), (39, 1), (40, 40), (100, 168), (168, 41)):
        ha, hb = R.haplotypes(b_rows[i], c_rows[j], K.SEQS)
        assert orc.edit_distance(ha.encode(), hb.encode()) == R.edit_distance(ha, hb)
    for group_min in (0, 1):
        svx_ctx.set_match_group_min(group_min)
        try:
            summary, want, rec = host.check(svx_ctx, base, comp, K.options_of(case), tmp_path / ("out%d" % group_min), key="crowded",
                                            compiled_distance=orc.edit_distance)
        finally:
            svx_ctx.set_match_group_min(0)
        assert sorted(zip(rec.matched[0][1], rec.matched[0][2])) == [(40, 40), (129, 129)]
        assert summary["TP-base"] > 100 and summary["by_type"]["INS"]["TP-base"] > 20


def test_the_command_on_the_device(tmp_path):
    from svim_asm_amd import compare_cli
    case = host.CASES["bed"]
    base, comp, bed = K.write(case, tmp_path / "in", gz=True)
    assert compare_cli.main([str(tmp_path / "out"), K.REF, base, comp, "--include_bed", bed]) == 0
    summary = json.load(open(tmp_path / "out" / "summary.json"))
    assert (summary["TP-base"], summary["FN"], summary["FP"], summary["base"]["out_of_regions"]) == (6, 0, 0, 5)
