"""The C oracle's CIGAR walk and statistics on the long-alignment cases of tests/cigar_long_cases.py against the numpy
restatement there (cumulative sums in 64 bits, reduced modulo 2^32) — so that what tests/test_gpu_cigar_long.py expects
of the kernels rests on two computations written from the reference's rules independently of each other — and the
preconditions of every case."""
import numpy as np
import pytest

from oracle import orc
from tests import cigar_long_cases as LC

KEYS = ("aln", "ref_pos", "read_pos", "len", "type")


def test_case_list():
    """The units and starts under test (tile sizes and scan widths of svx_cigar.hip at the default macros)."""
    got = {(c.path, c.unit): set() for c in LC.CASES.values()}
    for c in LC.CASES.values():
        got[(c.path, c.unit)].add(c.P)
        assert c.L >= 2 * c.unit + c.unit // 2
    four = lambda U: {U - 1, U, U + 1, U // 2 + 7}
    two = lambda U: {U - 1, U // 2 + 7}
    assert got == {("streaming", 65536): four(65536), ("streaming", 262144): four(262144), ("streaming", 4194304): two(4194304),
                   ("small", 32768): four(32768), ("small", 524288): four(524288), ("small", 2097152): two(2097152)}
    assert sum(n.endswith("-ends-on-tile") for n in LC.SMALL) == 1
    assert LC.CAP_CASE in LC.STREAMING and len(LC.BLOCK_LEVEL) == 2


@pytest.mark.parametrize("name", list(LC.CASES))
def test_oracle_equals_the_restatement(name):
    b = LC.build(name)
    f = LC.check_preconditions(name, b)
    exp = LC.restated_extract(b["cigar"], b["aln_off"], b["ref_start"], LC.MIN_LEN)
    got = orc.cigar_extract(b["cigar"], b["aln_off"], b["ref_start"], LC.MIN_LEN)
    for k in KEYS:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), k
    # the signatures of the long alignment reach past its covered units, and so do the restatement's 64-bit cursors
    mine = got["aln"] == f["long"]
    assert int(mine.sum()) > 2 * LC.DENSE_RUN
    if name in LC.BLOCK_LEVEL:
        wide = LC.restated_extract(b["cigar"], b["aln_off"], np.zeros_like(b["ref_start"]), LC.MIN_LEN)
        assert np.any(np.diff(wide["ref_pos"][mine].astype(np.int64)) < 0)   # the 32-bit cursors wrapped on the way
        assert np.any(np.diff(wide["read_pos"][mine].astype(np.int64)) < 0)
    stats, exp_stats = orc.cigar_stats(b["cigar"], b["aln_off"]), LC.restated_stats(b["cigar"], b["aln_off"])
    assert sorted(stats) == sorted(exp_stats)
    for k in exp_stats:
        assert np.array_equal(stats[k], exp_stats[k]), k
    assert int(stats["q_start"].max()) > 0 and int(stats["n_hard"][f["long"]]) > 0


def test_restatement_on_the_reference_known_answers():
    """The reference's own vectors (src/tests/test_intra.py:8-22, min_length 30) and SURVEY.md A1.2, by the restatement."""
    def words(tuples):
        return np.array([(l << 4) | o for o, l in tuples], dtype=np.uint32)
    c = words([(5, 10), (4, 20), (0, 30), (1, 40), (2, 50), (0, 30), (4, 25), (5, 15)])
    out = LC.restated_extract(c, [0, len(c)], [0], 30)
    assert [out[k].tolist() for k in KEYS] == [[0, 0], [30, 30], [50, 90], [40, 50], [0, 1]]
    c = words([(0, 10), (3, 1000), (0, 10), (2, 50)])
    out = LC.restated_extract(c, [0, 0, 4], [7, 100], 40)
    assert [out[k].tolist() for k in KEYS] == [[1], [120], [20], [50], [1]]
    st = LC.restated_stats(words([(5, 3), (4, 2), (4, 5), (0, 10), (1, 4), (3, 6), (4, 7), (5, 1), (0, 9)]), [0, 8, 8, 9])
    assert {k: v.tolist() for k, v in st.items()} == {"ref_len": [16, 0, 9], "q_start": [7, 0, 0], "q_end": [21, 0, 9],
                                                      "read_len": [32, 0, 9], "n_hard": [4, 0, 0]}
