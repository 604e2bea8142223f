"""svim-asm-small-compare on the device: the fixture pair, its haplotype columns exchanged, one
replay-matched record removed, and several batches — every file byte for byte against
tests/replay_restatement.compare_small, with the integers tests/test_smallcmp_host.py holds the stand-ins to."""
import pytest

from svim_asm_amd import smallcmp_cli
from tests import smallcmp_cases as S
from tests.test_smallcmp_host import insertion_and_the_edit_where_it_stands, integers

pytestmark = pytest.mark.gpu


def run(out_dir, base, comp, options):
    assert smallcmp_cli.main(S.argv_of(out_dir, base, comp, options)) == 0


def pair(tmp_path, comp_text=None):
    texts = S.fixture_texts()
    return S.write(tmp_path, "base.vcf", texts[0]), S.write(tmp_path, "comp.vcf", comp_text or texts[1])


def test_a_the_fixture_pair(svx_ctx, tmp_path):
    summary, details = S.check(run, *pair(tmp_path), tmp_path)
    assert integers(summary) == (929, 0, 929, 0, 846, 83, 846, 83) and summary["precision"] == summary["recall"] == 1.0
    assert summary["clusters"]["straight"] == 83 and all(d["flags"] == [1, 1, 0, 0] for d in details)


def test_b_haplotype_columns_exchanged(svx_ctx, tmp_path):
    summary, details = S.check(run, *pair(tmp_path, S.map_gt(S.fixture_texts()[1], S.swap_haplotypes)), tmp_path)
    assert integers(summary) == (929, 0, 929, 0, 846, 83, 846, 83) and summary["clusters"]["swapped"] == 83
    assert all(d["flags"] == [0, 0, 1, 1] for d in details)


def test_c_one_replay_matched_record_removed(svx_ctx, tmp_path):
    texts = S.fixture_texts()
    base_lines = set(texts[0].splitlines())
    lines = texts[1].splitlines()
    victim = next(i for i, l in enumerate(lines) if not l.startswith("#") and l not in base_lines)
    summary, details = S.check(run, *pair(tmp_path, "\n".join(lines[:victim] + lines[victim + 1:]) + "\n"), tmp_path)
    assert summary["FN"] >= 1 and summary["TP-base"] == 929 - summary["FN"] and sum(1 for d in details if d["flags"][:2] != [1, 1]) == 1


def test_d_unphased_comp_takes_the_union(svx_ctx, tmp_path):
    summary, _ = S.check(run, *pair(tmp_path, S.fixture_texts()[1].replace("|", "/")), tmp_path)
    assert integers(summary) == (927, 2, 927, 2, 846, 81, 846, 81) and summary["comp"]["conflict"] == 2


def test_f_several_batches_give_the_same_bytes(svx_ctx, tmp_path):
    summary, _ = S.check(run, *pair(tmp_path), tmp_path, batch_bases=300)
    assert integers(summary) == (929, 0, 929, 0, 846, 83, 846, 83)


def test_an_insertion_and_the_edit_where_it_stands_are_one_edit(svx_ctx, tmp_path):
    base, comp, twice = insertion_and_the_edit_where_it_stands()
    files = lambda d, body: (S.write(tmp_path / d, "base.vcf", S.HEADER + base), S.write(tmp_path / d, "comp.vcf", S.HEADER + body))
    summary, _ = S.check(run, *files("once", comp), tmp_path / "once")
    assert integers(summary) == (2, 0, 4, 0, 0, 2, 0, 4) and summary["comp"]["conflict"] == 0
    summary, _ = S.check(run, *files("twice", twice), tmp_path / "twice")
    assert summary["comp"]["conflict"] == 1 and integers(summary)[:4] == (1, 1, 2, 3)
