"""The case table of the CIGAR tile walk (tests/cigar_tile_cases.py) where there is no GPU: the C oracle and the numpy
restatement of the walk (tests/cigar_long_cases.py) agree on every case and on the combined batch, so that what
tests/test_gpu_cigar_tiles.py expects of the kernels rests on two independent computations; every case shows the classes
it lists and the numbers its name promises, every class is shown on each path it applies to; the table's constants are
those of svx_cigar.hip; and a constant moved by one makes the preconditions fail."""
import os
import re

import numpy as np
import pytest

from oracle import orc
from tests import cigar_long_cases as LC
from tests import cigar_tile_cases as TC

KEYS = ("aln", "ref_pos", "read_pos", "len", "type")
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svim_asm_amd", "csrc", "svx_cigar.hip")


def assert_oracle_equals_restatement(cigar, aln_off, ref_start):
    exp = LC.restated_extract(cigar, aln_off, ref_start, TC.MIN_LEN)
    got = orc.cigar_extract(cigar, aln_off, ref_start, TC.MIN_LEN)
    for k in KEYS:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), k
    return exp


@pytest.mark.parametrize("family", TC.FAMILIES)
def test_oracle_equals_the_restatement(family):
    cases = TC.family(family)
    assert cases
    for c in cases:
        exp = assert_oracle_equals_restatement(c.cigar, c.aln_off, c.ref_start)
        F = TC.case_facts(c.name, "streaming")
        assert len(exp["aln"]) == F.n_sig == TC.case_facts(c.name, "two_launch").n_sig, c.name
        # the builder's promise: the k-th signature is MIN_LEN + k long, I and D alternate (but for planted lengths)
        if c.family != "lengths":
            assert exp["len"].tolist() == list(range(TC.MIN_LEN, TC.MIN_LEN + F.n_sig)), c.name
            assert exp["type"].tolist() == [k & 1 for k in range(F.n_sig)], c.name
        assert len(c.cigar) <= (33 * TC.ROUND if c.family == "finish" else 3 * TC.TILE), c.name


def test_combined_batch():
    b = TC.combined()
    exp = assert_oracle_equals_restatement(b["cigar"], b["aln_off"], b["ref_start"])
    assert all(at % TC.TILE == 0 for at in b["bases"].values()) and len(b["cigar"]) % TC.TILE == 0
    assert 200_000 <= len(b["cigar"]) <= 900_000
    # every case keeps its tiles: the signatures are the cases' own, and so are the dense tiles of both paths
    assert len(exp["aln"]) == sum(TC.case_facts(n, "streaming").n_sig for n in TC.CASES)
    for path in TC.PATHS:
        F = TC.facts(b["cigar"], b["aln_off"], path)
        per_case = [at // F.tile_ops + t for n, at in b["bases"].items() for t in TC.case_facts(n, path).dense]
        assert F.dense == sorted(per_case) and len(per_case) > 20, path


def test_preconditions():
    shown = TC.check_preconditions()
    assert len(TC.CASES) >= 60 and set(c.family for c in TC.CASES.values()) == set(TC.FAMILIES)
    assert {cid for cid, _ in shown} == set(TC.CLASSES) - set(TC.EXEMPT)
    for name in TC.CAPACITY_CASES:
        assert name in TC.CASES
    staged, dense, past = [TC.case_facts(n, "streaming").tiles[1] for n in TC.CAPACITY_CASES]
    assert not staged.dense and staged.drains and dense.dense
    assert TC.case_facts(TC.CAPACITY_CASES[2], "two_launch").tiles[5].direct_slab == 32


def test_a_case_that_belies_its_name_fails():
    c = TC.CASES["profile-40-30-40-18"]
    cig = c.cigar.copy()
    at = TC.TILE + TC.ROUND + np.nonzero(((cig[TC.TILE + TC.ROUND:] & 15) == 0))[0][0]
    cig[at] = (77 << 4) | 1    # a 31st signature in the tile's round 1
    with pytest.raises(AssertionError, match="profile-40-30-40-18"):
        TC.check_preconditions(cases={c.name: c._replace(cigar=cig)})


def test_constants_are_those_of_the_kernel_source():
    """A retune has to move the table in the same change, not move the thresholds off it."""
    text = open(SOURCE).read()
    for macro, key in TC.DEFINES.items():
        found = re.findall(r"^#define\s+%s\s+(\d+)\b" % macro, text, re.M)
        assert len(found) == 1 and int(found[0]) == TC.K[key], (macro, found, TC.K[key])
    lanes = re.findall(r"^constexpr int kFinLanes = (\d+);", text, re.M)
    assert len(lanes) == 1 and int(lanes[0]) == TC.K["FIN_LANES"], lanes
    groups = re.findall(r"^#define\s+SVX_FIN_GROUPS\s+(\d+)\b", text, re.M)
    per = re.findall(r"^constexpr uint32_t kFinTiles = (\d+)u \* kFinGroups;", text, re.M)
    assert len(groups) == 1 and len(per) == 1 and int(per[0]) * int(groups[0]) == TC.K["FIN_TILES"], (groups, per)
    assert int(per[0]) == TC.FOLD
    assert TC.ROUND == TC.WAVE * TC.K["LANE_OPS"] and TC.TILE == TC.ROUND * TC.K["ROUNDS"]


@pytest.mark.parametrize("delta", [-1, 1])
@pytest.mark.parametrize("key", ["QUEUE", "QUEUE_SMALL", "STAGE", "SLAB", "FIN_TILES"])
def test_a_threshold_moved_by_one_fails_the_preconditions(key, delta):
    k = dict(TC.K)
    k[key] += delta
    with pytest.raises(AssertionError):
        TC.check_preconditions(k)
