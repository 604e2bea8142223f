"""svim-asm-small-compare where there is no GPU: `variant_replay` answered by the loop of
tests/replay_restatement.py and `cover_query` by a plain loop, patched onto tests/helpers.OracleBackedContext; every file
the command writes byte for byte against tests/replay_restatement.compare_small, and on top of that the integers of the
fixture pair, of its rewritten copies and of made-up files.  tests/test_gpu_smallcmp.py holds the real kernels to the
same expectation."""
import json
import os

import numpy as np
import pytest

from svim_asm_amd import smallcmp_cli
from tests import helpers, replay_restatement as RR, smallcmp_cases as S
from tests.test_compare_host import restated_cover_query

CALLS = {"variant_replay": 0, "jobs": 0}
ZERO = {"multiallelic": 0, "symbolic_or_other": 0, "not_carried": 0, "filtered": 0, "no_change": 0, "too_large": 0, "ref_mismatch": 0,
        "out_of_regions": 0, "duplicate": 0, "conflict": 0, "over_max_cluster": 0}


def restated_variant_replay(self, bases, win_off, win_len, ed_first, ed_start, ed_ref_len, ed_alt_off, ed_alt_len, pair_a=(), pair_b=(),
                            strings=False, cap=None):
    CALLS["variant_replay"] += 1
    CALLS["jobs"] += len(win_off)
    r = RR.replay_batch(bases, win_off, win_len, ed_first, ed_start, ed_ref_len, ed_alt_off, ed_alt_len, pair_a, pair_b)
    return {"out_len": np.array(r["out_len"], np.uint32), "status": np.array(r["status"], np.uint8), "equal": np.array(r["equal"], np.uint8),
            "total": r["total"]}


@pytest.fixture
def device(monkeypatch):
    monkeypatch.setattr(helpers.OracleBackedContext, "variant_replay", restated_variant_replay, raising=False)
    monkeypatch.setattr(helpers.OracleBackedContext, "cover_query", restated_cover_query, raising=False)
    for k in CALLS:
        CALLS[k] = 0
    return helpers.oracle_backed_device(monkeypatch)


def run(out_dir, base, comp, options):
    assert smallcmp_cli.main(S.argv_of(out_dir, base, comp, options)) == 0


def integers(summary):
    return tuple(summary[k] for k in ("TP-base", "FN", "TP-comp", "FP")) + (summary["TP_exact"]["base"], summary["TP_replay"]["base"],
                                                                           summary["TP_exact"]["comp"], summary["TP_replay"]["comp"])


# ------------------------------------------------------------------------------------------------- the fixture pair
def test_a_the_fixture_pair(device, tmp_path):
    base, comp = (S.write(tmp_path, n, t) for n, t in zip(("base.vcf", "comp.vcf"), S.fixture_texts()))
    summary, details = S.check(run, base, comp, tmp_path)
    assert integers(summary) == (929, 0, 929, 0, 846, 83, 846, 83)
    assert summary["precision"] == summary["recall"] == summary["f1"] == 1.0
    assert summary["clusters"] == {"all": 825, "replayed": 83, "phased": 83, "union": 0, "straight": 83, "swapped": 0, "over_max_cluster": 0}
    assert summary["base"] == dict(ZERO, records=929, compared=929) == summary["comp"]
    assert summary["gt_compared"] == summary["gt_concordant"] == 846
    assert sum(summary["by_type"][t]["TP-base"] for t in RR.TYPES) == 929 and summary["by_type"]["COMPLEX"]["TP-base"] == 0
    assert all(d["flags"] == [1, 1, 0, 0] for d in details)
    assert CALLS == {"variant_replay": 1, "jobs": 4 * 83}   # a cluster whose records all have twins is not sent


def test_b_haplotype_columns_exchanged(device, tmp_path):
    texts = S.fixture_texts()
    base, comp = S.write(tmp_path, "base.vcf", texts[0]), S.write(tmp_path, "comp.vcf", S.map_gt(texts[1], S.swap_haplotypes))
    summary, details = S.check(run, base, comp, tmp_path)
    assert integers(summary) == (929, 0, 929, 0, 846, 83, 846, 83)
    assert summary["clusters"]["swapped"] == 83 and summary["clusters"]["straight"] == 0
    assert all(d["flags"] == [0, 0, 1, 1] for d in details)


def test_c_one_replay_matched_record_removed(device, tmp_path):
    texts = S.fixture_texts()
    base_lines = set(texts[0].splitlines())
    lines = texts[1].splitlines()
    victim = next(i for i, l in enumerate(lines) if not l.startswith("#") and l not in base_lines)
    contig, pos, gt = lines[victim].split("\t")[0], int(lines[victim].split("\t")[1]), lines[victim].split("\t")[-1]
    comp = S.write(tmp_path, "comp.vcf", "\n".join(lines[:victim] + lines[victim + 1:]) + "\n")
    summary, details = S.check(run, S.write(tmp_path, "base.vcf", texts[0]), comp, tmp_path)
    fn = [l for l in open(str(tmp_path / "got" / "fn.vcf")).read().splitlines() if not l.startswith("#")]
    # exactly the base records of that cluster that are carried on the removed record's haplotype
    # (the removed record was the left-shifted spelling: it may lie in front of what is left of its cluster)
    d = next(d for d in details if d["flags"][:2] != [1, 1])
    assert d["contig"] == contig and abs(d["lo"] - pos) <= 100
    h = gt.split("|").index("1")
    assert d["flags"][h] == 0 and d["flags"][1 - h] == 1 and d["orientation"] == "straight"
    assert fn and all(l.split("\t")[0] == contig and d["lo"] <= int(l.split("\t")[1]) <= d["hi"] + 1 and l.split("\t")[-1].split("|")[h] == "1" for l in fn)
    assert summary["FN"] == len(fn) and summary["TP-base"] == 929 - len(fn)
    fp = [l for l in open(str(tmp_path / "got" / "fp.vcf")).read().splitlines() if not l.startswith("#")]
    assert summary["FP"] == len(fp) == summary["comp"]["compared"] - summary["TP-comp"] and summary["comp"]["compared"] == 928
    assert all(l.split("\t")[0] == contig and d["lo"] <= int(l.split("\t")[1]) <= d["hi"] + 1 for l in fp)
    assert sum(1 for x in details if x["flags"][:2] != [1, 1]) == 1          # nothing else moves


def test_d_unphased_comp_takes_the_union(device, tmp_path):
    """Every `|` of comp as `/`: a heterozygous record is no longer phased, its cluster replays both sides' records at once.
    The integers are the restatement's.  81 of the 83 replayed clusters still come out equal; in two (chr10:30184 and
    chr10:91516) records of the two haplotypes overlap, so taken together they collide on either side — 2 conflicts per
    side —, and the one record of each side in each of them that has no twin is FN / FP."""
    texts = S.fixture_texts()
    base, comp = S.write(tmp_path, "base.vcf", texts[0]), S.write(tmp_path, "comp.vcf", texts[1].replace("|", "/"))
    summary, details = S.check(run, base, comp, tmp_path)
    assert summary["clusters"]["union"] == summary["clusters"]["replayed"] == 83 and summary["clusters"]["phased"] == 0
    assert all(d["mode"] == "union" and len(d["flags"]) == 1 for d in details)
    assert integers(summary) == (927, 2, 927, 2, 846, 81, 846, 81)
    assert summary["base"]["conflict"] == summary["comp"]["conflict"] == 2
    assert [(d["contig"], d["lo"]) for d in details if d["flags"] == [0]] == [("chr10", 30184), ("chr10", 91516)]


def test_f_several_batches_give_the_same_bytes(device, tmp_path):
    base, comp = (S.write(tmp_path, n, t) for n, t in zip(("base.vcf", "comp.vcf"), S.fixture_texts()))
    S.check(run, base, comp, tmp_path, batch_bases=300)
    assert CALLS["variant_replay"] > 5 and CALLS["jobs"] == 4 * 83


# ------------------------------------------------------------------------------------------------- made-up files
C = "chr1"
SNV = lambda pos, gt="1|1", **kw: S.line(C, pos, S.ref_at(C, pos), S.other(S.ref_at(C, pos)), gt, **kw)


def made_up(tmp_path, base_body, comp_body, header=S.HEADER, **options):
    base, comp = S.write(tmp_path, "base.vcf", header + base_body), S.write(tmp_path, "comp.vcf", header + comp_body)
    return S.check(run, base, comp, tmp_path, **options)[0]


def only_non_tp(summary, side, key):
    """The one record of `side` that is not TP is the one counted under `key`."""
    other = "comp" if side == "base" else "base"
    assert summary[side][key] == 1 and summary[other][key] == 0


def test_e_ref_mismatch(device, tmp_path):
    good = SNV(1000) + SNV(2000)
    wrong = S.line(C, 3000, S.other(S.ref_at(C, 3000)), S.ref_at(C, 3000))
    s = made_up(tmp_path, good, good + wrong)
    only_non_tp(s, "comp", "ref_mismatch")
    assert integers(s)[:4] == (2, 0, 2, 0) and s["comp"]["compared"] == 2 and s["comp"]["records"] == 3


def test_e_too_large(device, tmp_path):
    good = SNV(1000)
    big = S.line(C, 3000, S.ref_at(C, 3000, 51), S.ref_at(C, 3000))        # 50 bases deleted: not < --max_size 50
    edge = S.line(C, 5000, S.ref_at(C, 5000, 50), S.ref_at(C, 5000))       # 49: compared
    s = made_up(tmp_path, good + edge, good + big + edge)
    only_non_tp(s, "comp", "too_large")
    assert integers(s)[:4] == (2, 0, 2, 0)


def test_e_duplicate(device, tmp_path):
    good = SNV(1000) + SNV(2000, rid="first")
    s = made_up(tmp_path, good, good + SNV(2000, rid="again"))
    only_non_tp(s, "comp", "duplicate")
    assert integers(s)[:4] == (2, 0, 2, 1) and s["comp"]["conflict"] == 0
    assert "again" in open(str(tmp_path / "got" / "fp.vcf")).read() and "first" in open(str(tmp_path / "got" / "tp-comp.vcf")).read()


def test_e_conflict(device, tmp_path):
    """Two comp records that overlap on haplotype 0: that job has no string; haplotype 1, which only the first is on, agrees."""
    a = S.line(C, 1000, S.ref_at(C, 1000, 3), S.ref_at(C, 1000), "1|1")                    # deletes 1001-1002
    b = S.line(C, 1001, S.ref_at(C, 1001), S.other(S.ref_at(C, 1001)), "1|0", rid="over")   # an SNV inside it, haplotype 0
    s = made_up(tmp_path, a, a + b)
    assert s["comp"]["conflict"] == 1 and s["base"]["conflict"] == 0
    assert integers(s)[:4] == (1, 0, 1, 1)                                                  # a has its twin; b is the only non-TP


def test_e_a_cluster_over_max_cluster(device, tmp_path, caplog):
    run5 = "".join(SNV(1000 + 10 * k) for k in range(5))                                    # one cluster of 10 records
    moved = S.line(C, 3000, S.ref_at(C, 3000, 2), S.ref_at(C, 3000))
    s = made_up(tmp_path, run5 + moved, run5 + moved, max_cluster=4)
    assert s["clusters"]["over_max_cluster"] == 1 and s["base"]["over_max_cluster"] == s["comp"]["over_max_cluster"] == 5
    assert integers(s)[:4] == (6, 0, 6, 0)                                                  # exact twins still count
    assert sum("--max_cluster" in r.getMessage() for r in caplog.records) == 1
    extra = SNV(1025, rid="extra")                                                          # without a twin inside the big cluster: FP
    s = made_up(tmp_path / "two", run5, run5 + extra, max_cluster=4)
    assert integers(s)[:4] == (5, 0, 5, 1) and CALLS["variant_replay"] == 0


def test_e_include_bed_is_one_line(device, tmp_path):
    bed = S.write(tmp_path, "r.bed", "%s\t900\t1001\n%s\t1001\t3000\n" % (C, C))
    inside = SNV(950) + SNV(2000)
    straddling = S.line(C, 1000, S.ref_at(C, 1000, 4), S.ref_at(C, 1000), rid="straddle")    # [1000, 1003) over both abutting lines
    s = made_up(tmp_path, inside, inside + straddling, include_bed=bed)
    only_non_tp(s, "comp", "out_of_regions")
    assert integers(s)[:4] == (2, 0, 2, 0)
    point = S.line(C, 3000, S.ref_at(C, 3000), S.ref_at(C, 3000) + "TT")                    # an insertion at 3000 == hi
    s = made_up(tmp_path / "ins", inside + point, inside + point, include_bed=bed)
    assert integers(s)[:4] == (3, 0, 3, 0)


def test_e_a_file_without_sample_columns(device, tmp_path):
    """No genotype: carried on both haplotypes, phased.  Comp spells base's deletion in a homopolymer one base further on."""
    seq = S.SEQS[C].upper()
    at = next(i for i in range(1000, len(seq) - 5) if seq[i] == seq[i + 1] == seq[i + 2] and seq[i - 1] != seq[i] and seq[i + 3] != seq[i])
    strip = lambda body: "".join("\t".join(l.split("\t")[:8]) + "\n" for l in body.splitlines())
    base_body = S.line(C, at, seq[at - 1:at + 1], seq[at - 1], "1|1")                       # deletes seq[at]
    comp_body = S.line(C, at + 1, seq[at:at + 2], seq[at])                                   # deletes seq[at + 1]
    base, comp = S.write(tmp_path, "base.vcf", S.HEADER + base_body), S.write(tmp_path, "comp.vcf", S.HEADER.replace("\tFORMAT\tS", "") + strip(comp_body))
    s = S.check(run, base, comp, tmp_path)[0]
    assert integers(s) == (1, 0, 1, 0, 0, 1, 0, 1) and s["clusters"]["phased"] == 1 and s["gt_compared"] == 0


def test_e_passonly(device, tmp_path):
    good = SNV(1000)
    s = made_up(tmp_path, good, good + SNV(2000, flt="q10"), passonly=True)
    only_non_tp(s, "comp", "filtered")
    assert integers(s)[:4] == (1, 0, 1, 0)
    s = made_up(tmp_path / "all", good, good + SNV(2000, flt="q10"))
    assert integers(s)[:4] == (1, 0, 1, 1)


def test_an_mnp_against_its_two_snvs_and_empty_sides(device, tmp_path):
    r = S.ref_at(C, 1000, 2)
    mnp = S.line(C, 1000, r, S.other(r[0]) + S.other(r[1]), "0|1")
    two = S.line(C, 1000, r[0], S.other(r[0]), "0|1") + S.line(C, 1001, r[1], S.other(r[1]), "0|1")
    s = made_up(tmp_path, mnp, two)
    assert integers(s) == (1, 0, 2, 0, 0, 1, 0, 2) and s["by_type"]["COMPLEX"]["TP-base"] == 1 and s["by_type"]["SNV"]["TP-comp"] == 2
    s = made_up(tmp_path / "none", "", two)
    assert integers(s)[:4] == (0, 0, 0, 2) and s["recall"] is None and s["precision"] == 0.0
    s = made_up(tmp_path / "both", "", "")
    assert s["precision"] is None and s["clusters"]["all"] == 0


def insertion_and_the_edit_where_it_stands():
    """(base, comp, comp with a second insertion) as svim-asm-small writes `..I D..` and a mismatching column behind an
    insertion: two records with one start each; base spells each pair as one complex record."""
    a, b = S.ref_at(C, 1000, 4), S.ref_at(C, 2000, 2)
    comp = S.line(C, 1000, a[0], a[0] + "GG", "1|0") + S.line(C, 1000, a, a[0], "1|0")                 # 1000: GG inserted, three bases deleted
    comp += S.line(C, 2000, b[0], b[0] + "TTT", "0|1") + S.line(C, 2001, b[1], S.other(b[1]), "0|1")  # 2000: TTT inserted in front of an SNV
    base = S.line(C, 1000, a, a[0] + "GG", "1|0") + S.line(C, 2000, b, b[0] + "TTT" + S.other(b[1]), "0|1")
    return base, comp, comp + S.line(C, 1000, a[0], a[0] + "C", "1|0", rid="second")


def test_an_insertion_and_the_edit_where_it_stands_are_one_edit(device, tmp_path):
    base, comp, twice = insertion_and_the_edit_where_it_stands()
    s = made_up(tmp_path, base, comp)
    assert integers(s) == (2, 0, 4, 0, 0, 2, 0, 4) and s["comp"]["conflict"] == s["base"]["conflict"] == 0
    assert s["clusters"]["replayed"] == 2 and CALLS == {"variant_replay": 1, "jobs": 8}
    s = made_up(tmp_path / "twice", base, twice)     # two insertions at one start: out of order, as before
    assert s["comp"]["conflict"] == 1 and integers(s)[:4] == (1, 1, 2, 3)


# ------------------------------------------------------------------------------------------------- exit statuses
def test_g_exit_codes_and_help(device, tmp_path, capsys, caplog):
    base, comp = (S.write(tmp_path, n, S.HEADER + SNV(1000)) for n in ("base.vcf", "comp.vcf"))
    out = str(tmp_path / "out")
    for extra in (["--max_size", "0"], ["--batch_bases", "0"], ["--max_cluster", "0"], ["--cluster_distance", "-1"], ["--include_bed", str(tmp_path / "no.bed")]):
        assert smallcmp_cli.main([out, S.REF, base, comp] + extra) == 2
    assert smallcmp_cli.main([out, S.REF, str(tmp_path / "none.vcf"), comp]) == 2
    assert "svim-asm-small-compare:" in capsys.readouterr().err and not os.path.exists(out)
    with pytest.raises(SystemExit) as ei:
        smallcmp_cli.main(["--help"])
    assert ei.value.code == 0 and "--cluster_distance" in capsys.readouterr().out
    assert smallcmp_cli.main([out, str(tmp_path / "none.fa"), base, comp]) == 1
    elsewhere = S.write(tmp_path, "else.vcf", S.HEADER + S.line("chrNowhere", 5, "A", "C"))
    assert smallcmp_cli.main([out, S.REF, base, elsewhere]) == 1 and any("chrNowhere" in r.getMessage() for r in caplog.records)
    assert smallcmp_cli.main([out, S.REF, base, comp, "--comp_sample", "nobody"]) == 1
    assert not os.path.exists(out)
    assert smallcmp_cli.main([out, S.REF, base, comp]) == 0 and json.load(open(os.path.join(out, "summary.json")))["TP-base"] == 1
    assert not [f for f in os.listdir(out) if f.endswith(".tmp")]


def test_the_command_line_tool_exists():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "svim-asm-small-compare")
    assert os.access(path, os.X_OK) and "smallcmp_cli" in open(path).read()
