"""Randomised differential test: oracle/svim_oracle.py vs the REAL reference (run with the stub pysam/edlib of
oracle/refstub).  The inputs come from the seeded generators below; what the reference returned for them is stored
in tests/golden/reference_diff.json.gz (`oracle/make_golden.py refdiff`), so the test needs no reference checkout."""
import numpy as np
import pytest

from oracle import svim_oracle
from tests import helpers

NAMES = ["chr1", "chr10", "chr2", "chrX"]
LENGTHS = [3_000_000, 1_500_000, 2_000_000, 800_000]
COLLECT_OPTIONS = [dict(), dict(min_sv_size=30, max_sv_size=3000), dict(min_mapq=0, query_gap_tolerance=500),
                   dict(reference_overlap_tolerance=0, query_overlap_tolerance=0)]


def collect_case(seed):
    rng = np.random.default_rng(seed)
    recs = helpers.random_records(rng, NAMES, LENGTHS, 60) + helpers.engineered_split_records(rng, NAMES, LENGTHS, 60)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return recs, helpers.options(**COLLECT_OPTIONS[seed % 4])


def all_types_case():
    rng = np.random.default_rng(123)
    return helpers.engineered_split_records(rng, NAMES, LENGTHS, 1500), helpers.options()


def pair_case(seed):
    rng = np.random.default_rng(100 + seed)
    seqs = {n: "".join(rng.choice(list("ACGTacgtN"), size=min(l, 40000))) for n, l in zip(NAMES, LENGTHS)}
    lengths = [len(seqs[n]) for n in NAMES]
    t1 = helpers.random_candidates(rng, NAMES, lengths, seqs, 120, "h1")
    t2 = helpers.random_candidates(rng, NAMES, lengths, seqs, 120, "h2")
    # a share of haplotype-2 candidates are near-copies of haplotype-1 ones (→ 1/1 calls)
    for c in t1[:60]:
        if c[0] in ("DEL", "INS", "INV", "DUP_TAN"):
            shift = int(rng.integers(-3, 4))
            lst = list(c)
            lst[2] = max(0, c[2] + shift)
            lst[3] = max(lst[2], c[3] + shift)
            rd_i = {"DEL": 4, "INS": 4, "INV": 4, "DUP_TAN": 6}[c[0]]
            lst[rd_i] = ("h2_copy",)
            t2.append(tuple(lst))
    o = helpers.options(max_edit_distance=[200, 10, 50][seed % 3], partition_max_distance=[1000, 100][seed % 2],
                        query_names=bool(seed % 2), tandem_duplications_as_insertions=bool(seed & 2),
                        interspersed_duplications_as_insertions=bool(seed & 4))
    return seqs, lengths, t1, t2, o


@pytest.fixture(scope="module")
def ref():
    return helpers.load_reference_diff()["oracle"]


@pytest.mark.parametrize("seed", range(8))
def test_collect_matches_reference(ref, seed):
    recs, o = collect_case(seed)
    exp = helpers.reference_answer(ref["collect"][seed], recs, o)
    got = svim_oracle.collect(recs, NAMES, LENGTHS, o)
    assert got == exp
    if seed == 0:
        kinds = {c[0] for c in exp}
        assert {"DEL", "INS", "BND"} <= kinds


def test_all_sv_types_reachable(ref):
    recs, o = all_types_case()
    exp = helpers.reference_answer(ref["all_types"], recs, o)
    got = svim_oracle.collect(recs, NAMES, LENGTHS, o)
    assert got == exp
    assert {c[0] for c in got} == {"DEL", "INS", "BND", "DUP_TAN", "DUP_INT", "INV"}


@pytest.mark.parametrize("seed", range(6))
def test_pair_and_vcf_match_reference(ref, seed):
    seqs, lengths, t1, t2, o = pair_case(seed)
    fasta = helpers.FakeFasta(seqs)
    exp = helpers.reference_answer(ref["pair"][seed], (seqs, t1, t2), o)
    ref_lens = dict(zip(NAMES, lengths))
    from oracle import orc
    got = svim_oracle.pair_candidates(helpers.constructed_again(t1, ref_lens), helpers.constructed_again(t2, ref_lens), fasta.fetch, NAMES, lengths, ref_lens, o,
                                      edit=lambda a, b: orc.edit_distance(a.encode(), b.encode()))
    assert got == exp
    assert {c[-1] for c in got} == {"1/1", "1/0", "0/1"}
    # VCF text (##fileDate masked)
    assert svim_oracle.vcf_text(got, fasta.fetch, NAMES, lengths, o) == ref["pair"][seed]["vcf"]
