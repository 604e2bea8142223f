"""svx_vcfin_open_sites (vcfin.read_sites): a VCF read as a list of SITES — the sample columns are not looked at, no
record is not_carried, gt is 0 — on the hand-written lines and the golden files of tests/test_vcfin.py, whose results
under svx_vcfin_open stay what they were.  The reader's parsing does not change beyond that flag (the classifier runs
with "no sample column"), so the sanitizer driver of tests/test_vcfin_sanitizers.py covers it as it stands."""
import os

import pytest

from svim_asm_amd import vcfin
from tests import test_vcfin as V


def test_classes_by_hand_under_open_sites(tmp_path):
    p = V.write(tmp_path, V.body(*V.ALL_BUT_U))
    sites = vcfin.read_sites(p, V.CONTIGS, V.LENGTHS)
    assert sites.counts == {"DEL": 9, "INS": 3, "multiallelic": 1, "complex": 3, "unresolved": 1, "other": 3, "not_carried": 0, "filtered": 0}
    rows = V.rows_of(sites)
    assert [r["id"] for r in rows] == ["a", "b", "c", "d", "e", "f", "k", "l", "m", "r", "s", "t"]
    assert all(r["gt"] == 0 for r in rows)
    # the records a sample column dropped are sites like any other
    assert [(r["id"], r["class"], r["start"], r["end"]) for r in rows[-3:]] == [("r", "DEL", 50, 53), ("s", "DEL", 50, 53), ("t", "DEL", 50, 53)]
    # everything but gt and the class of the dropped ones is what svx_vcfin_open gives, for either sample
    for sample in (None, "S2"):
        rec = V.same_as_restatement(p, sample=sample)
        by_id = {r["id"]: r for r in rows}
        for r in V.rows_of(rec):
            assert {k: v for k, v in r.items() if k != "gt"} == {k: v for k, v in by_id[r["id"]].items() if k != "gt"}
        assert rec.counts["not_carried"] + len(rec) == len(sites) and rec.n_lines == sites.n_lines and rec.header == sites.header
    po = vcfin.read_sites(p, V.CONTIGS, V.LENGTHS, passonly=True)
    assert po.counts["filtered"] == 1 and "c" not in [r["id"] for r in V.rows_of(po)]


def test_open_is_unchanged_on_the_same_file(tmp_path):
    p = V.write(tmp_path, V.body(*V.ALL_BUT_U))
    rec = V.same_as_restatement(p)
    assert rec.counts == {"DEL": 6, "INS": 3, "multiallelic": 1, "complex": 3, "unresolved": 1, "other": 3, "not_carried": 3, "filtered": 0}
    assert [r["gt"] for r in V.rows_of(rec)] == [3, 2, 1, 3, 2, 3, 2, 2, 2]


def test_a_line_without_sample_columns_is_a_site(tmp_path):
    # refused by svx_vcfin_open in a file whose header names samples ("no column for the sample")
    p = V.write(tmp_path, V.body("u"))
    with pytest.raises(vcfin.VcfFormatError, match="no column for the sample"):
        vcfin.read_vcf(p, V.CONTIGS, V.LENGTHS)
    assert [(r["id"], r["class"], r["gt"]) for r in V.rows_of(vcfin.read_sites(p, V.CONTIGS, V.LENGTHS))] == [("u", "DEL", 0)]


@pytest.mark.parametrize("line,what", [r for r in V.REFUSALS if "sample" not in r[1]])
def test_the_other_refusals_stay(tmp_path, line, what):
    with pytest.raises(vcfin.VcfFormatError, match=what) as e:
        vcfin.read_sites(V.write(tmp_path, V.body("a") + line), V.CONTIGS, V.LENGTHS)
    assert "line 5" in str(e.value)  # (two header lines, `a`, the empty line body() ends with)


@pytest.mark.parametrize("name", ["diploid_default.vcf", "haploid_default.vcf"])
def test_golden_files(name):
    path = os.path.join(V.GOLD, name)
    rec, sites = V.same_as_restatement(path), vcfin.read_sites(path, V.CONTIGS, V.LENGTHS)
    assert rec.counts["not_carried"] == 0 and sites.counts == rec.counts
    a, b = V.rows_of(rec), V.rows_of(sites)
    assert [{k: v for k, v in r.items() if k != "gt"} for r in a] == [{k: v for k, v in r.items() if k != "gt"} for r in b]
    assert all(r["gt"] == 0 for r in b) and all(r["gt"] != 0 for r in a)
