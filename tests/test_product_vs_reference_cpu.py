"""Randomised differential test of the PRODUCT's host path (svim_asm_amd COLLECT / PAIR / VCF writer, the device
answered by the CPU oracle) against the REAL reference (run with the stub pysam / edlib of oracle/refstub).  The
inputs come from the seeded generators below; what the reference returned for them is stored in
tests/golden/reference_diff.json.gz (`oracle/make_golden.py refdiff`), so the test needs no reference checkout."""
import os
import tempfile

import numpy as np
import pytest

from svim_asm_amd import SVCandidate, SVIM_COLLECT, SVIM_COMBINE
from tests import helpers
from tests.test_oracle_vs_reference import COLLECT_OPTIONS, LENGTHS, NAMES


def collect_case(seed):
    rng = np.random.default_rng(5000 + seed)
    recs = helpers.random_records(rng, NAMES, LENGTHS, 60) + helpers.engineered_split_records(rng, NAMES, LENGTHS, 90)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return recs, helpers.options(**COLLECT_OPTIONS[seed % 4])


def pair_case(seed):
    rng = np.random.default_rng(5100 + seed)
    seqs = {n: "".join(rng.choice(list("ACGTacgtN"), size=30000)) for n in NAMES}
    lengths = [30000] * len(NAMES)
    t1 = helpers.random_candidates(rng, NAMES, lengths, seqs, 110, "h1")
    t2 = helpers.random_candidates(rng, NAMES, lengths, seqs, 110, "h2")
    for c in t1[:60]:
        if c[0] in ("DEL", "INS", "INV", "DUP_TAN"):
            shift = int(rng.integers(-3, 4))
            lst = list(c)
            lst[2] = max(0, c[2] + shift)
            lst[3] = max(lst[2], c[3] + shift)
            lst[{"DEL": 4, "INS": 4, "INV": 4, "DUP_TAN": 6}[c[0]]] = ("h2_copy",)
            t2.append(tuple(lst))
    o = helpers.options(max_edit_distance=[200, 10, 50, 0][seed], partition_max_distance=[1000, 100][seed % 2],
                        query_names=bool(seed % 2), tandem_duplications_as_insertions=bool(seed & 2))
    return seqs, lengths, t1, t2, o


@pytest.fixture(scope="module")
def ref():
    return helpers.load_reference_diff()["product"]


@pytest.fixture(autouse=True)
def device_is_the_oracle(monkeypatch):
    helpers.oracle_backed_device(monkeypatch)


@pytest.mark.parametrize("seed", range(6))
def test_collect_matches_the_real_reference(ref, seed):
    recs, o = collect_case(seed)
    exp = helpers.reference_answer(ref["collect"][seed], recs, o)
    got = [helpers.candidate_tuple(c) for c in
           SVIM_COLLECT.analyze_alignment_file_coordsorted(helpers.FakeBam(NAMES, LENGTHS, recs), o)]
    assert got == exp


@pytest.mark.parametrize("seed", range(4))
def test_pair_and_vcf_match_the_real_reference(ref, seed, tmp_path):
    seqs, lengths, t1, t2, o = pair_case(seed)
    exp = helpers.reference_answer(ref["pair"][seed], (seqs, t1, t2), o)
    bam = helpers.FakeBam(NAMES, lengths, [])
    got_objs = SVIM_COMBINE.pair_candidates([helpers.build_candidate(t, bam, SVCandidate) for t in t1],
                                            [helpers.build_candidate(t, bam, SVCandidate) for t in t2],
                                            helpers.FakeFasta(seqs), bam, o)
    assert [helpers.candidate_tuple(c) for c in got_objs] == exp
    # VCF text of the product's writer against the reference's (##fileDate masked)
    types = [t.strip() for t in o.types.split(",")]
    o.working_dir = tempfile.mkdtemp(dir=str(tmp_path))
    by = lambda t: [c for c in got_objs if c.type == t]
    SVIM_COMBINE.write_final_vcf(by("DUP_INT"), by("INV"), by("DUP_TAN"), by("DEL"), by("INS"), by("BND"), "1.0.3", NAMES,
                                 lengths, types, helpers.FakeFasta(seqs), o)
    got_vcf = "".join(l for l in open(os.path.join(o.working_dir, "variants.vcf")) if not l.startswith("##fileDate="))
    assert got_vcf == ref["pair"][seed]["vcf"]
