"""svx_match_greedy_batch (svx_match.hip) against the restatement (tests/match_restatement.py: sort the eligible pairs,
scan them), element for element, in both forms: set_match_group_min(1) — every partition with a pair on the
workgroup kernel — and set_match_group_min(MATCH_LANES_ONLY) — one lane per partition.

The shapes are the ones at which the code takes another path: the empty sides, 1 x 1, the sub-group widths of the row
scan (1, 2, 4 ... 64 lanes a row: n_comp of 1, 2, 5, 17, 65), both sides of the default threshold between the two
kernels (9 pairs), of the group kernel's launch classes (1024 and 4096 pairs), of the LDS bound of the matrix
(MATCH_LDS_PAIRS: 128 x 256, and one row more) and of the LDS bound of the per-row state (24 KiB: 1 x 8192 and
2100 x 16 have theirs in the context's scratch), and the largest partition the entry point takes (2^20 pairs).  A
lane needs min(nb, nc) * nb * nc reads, so the lane form is left out where that is seconds (512 x 512 and beyond)."""
import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import match_cases as M

pytestmark = pytest.mark.gpu

NONE = _lib.MATCH_NONE
LDS_ROWS = _lib.MATCH_LDS_PAIRS // 256
GROUP, LANES = 1, _lib.MATCH_LANES_ONLY


@pytest.fixture
def group_min(svx_ctx):
    yield svx_ctx.set_match_group_min
    svx_ctx.set_match_group_min(0)


def _run(ctx, dist, n_base, n_comp):
    mb, mc = ctx.match_greedy_batch(dist, n_base, n_comp)
    return mb.tolist(), mc.tolist()


def _both_forms(ctx, group_min, parts, lanes=True):
    dist, n_base, n_comp, want_base, want_comp = M.batch(parts)
    for setting in (GROUP, LANES) if lanes else (GROUP,):
        group_min(setting)
        got_base, got_comp = _run(ctx, dist, n_base, n_comp)
        assert got_base == want_base, (setting, parts)
        assert got_comp == want_comp, (setting, parts)


SHAPES = [(0, 0), (0, 3), (3, 0), (1, 1), (1, 2), (2, 1), (7, 5), (33, 65), (17, 17), (15, 17), (16, 16), (1, 257), (32, 32),
          (25, 41), (64, 64), (65, 63)]


@pytest.mark.parametrize("family", M.FAMILIES)
def test_small_shapes_every_family(svx_ctx, group_min, family):
    _both_forms(svx_ctx, group_min, [(family, nb, nc) for nb, nc in SHAPES])


def test_one_by_one_eligible_and_not(svx_ctx, group_min):
    for setting in (GROUP, LANES, 0):
        group_min(setting)
        assert _run(svx_ctx, [3], [1], [1]) == ([0], [0])
        assert _run(svx_ctx, [0], [1], [1]) == ([0], [0])
        assert _run(svx_ctx, [NONE - 1], [1], [1]) == ([0], [0])
        assert _run(svx_ctx, [NONE], [1], [1]) == ([NONE], [NONE])
        assert _run(svx_ctx, [NONE, 3, 9, NONE], [1, 1, 1, 1], [1, 1, 1, 1]) == ([NONE, 0, 0, NONE], [NONE, 0, 0, NONE])


def test_greedy_is_not_optimal_and_ties_give_the_diagonal(svx_ctx, group_min):
    for setting in (GROUP, LANES, 0):
        group_min(setting)
        # the optimal assignment would take (0, 1) and (1, 0): 4 instead of 101
        assert _run(svx_ctx, [1, 2, 2, 100], [2], [2]) == ([0, 1], [0, 1])
        assert _run(svx_ctx, [5] * 9, [3], [3]) == ([0, 1, 2], [0, 1, 2])
        assert _run(svx_ctx, [5] * 9 + [1, 2, 2, 100], [3, 2], [3, 2]) == ([0, 1, 2, 0, 1], [0, 1, 2, 0, 1])
        # 1 x 2 and 2 x 1: the smaller distance, the first at a tie
        assert _run(svx_ctx, [4, 3, 4, 4, 3, 4, 4, 4], [1, 1, 2, 2], [2, 2, 1, 1]) == \
            ([1, 0, 0, NONE, 0, NONE], [NONE, 0, 0, NONE, 0, 0])


def test_empty_sides_and_empty_batches(svx_ctx, group_min):
    for setting in (GROUP, LANES):
        group_min(setting)
        assert _run(svx_ctx, [], [], []) == ([], [])
        assert _run(svx_ctx, [], [0], [0]) == ([], [])
        assert _run(svx_ctx, [], [0, 2], [3, 0]) == ([NONE, NONE], [NONE, NONE, NONE])
        assert _run(svx_ctx, [7], [0, 1, 2], [3, 1, 0]) == ([0, NONE, NONE], [NONE, NONE, NONE, 0])


@pytest.mark.parametrize("family", ("none", "last", "equal"))
def test_nothing_eligible_only_the_last_cell_and_all_equal(svx_ctx, group_min, family):
    _both_forms(svx_ctx, group_min, [(family, 64, 64), (family, 129, 127), (family, 1, 1), (family, 3, 3)])


def test_threshold_between_the_two_kernels(svx_ctx, group_min):
    """Thresholds inside the batch's sizes, the default (9 pairs: 2 x 4 is a lane's, 3 x 3 and 1 x 9 a group's) among
    them: both kernels in one call."""
    parts = [("ties", 7, 5), ("wide", 16, 16), ("ties", 15, 17), ("same_rows", 1, 257), ("wide", 33, 65), ("ties", 1, 1),
             ("ties", 6, 6), ("edge", 255, 1), ("edge", 1, 256), ("ties", 2, 4), ("wide", 4, 2), ("ties", 3, 3), ("wide", 1, 9),
             ("ties", 9, 1), ("wide", 2, 5), ("ties", 1, 8), ("ties", 1, 2), ("wide", 2, 2)]
    dist, n_base, n_comp, want_base, want_comp = M.batch(parts)
    for setting in (0, 8, 9, 10, 35, 36, 37, 255, 256, 257, 258):
        group_min(setting)
        assert _run(svx_ctx, dist, n_base, n_comp) == (want_base, want_comp), setting


def test_launch_classes_of_the_group_kernel(svx_ctx, group_min):
    """1024 | 1025 and 4096 | 4097 pairs: 64 and 256 lanes a group, each launch with the LDS of its largest partition."""
    _both_forms(svx_ctx, group_min, [("ties", 32, 32), ("wide", 25, 41), ("ties", 64, 64), ("wide", 17, 241), ("ties", 1, 1)])


@pytest.mark.parametrize("family", ("ties", "wide"))
def test_both_sides_of_the_lds_bound(svx_ctx, group_min, family):
    """The largest matrix in LDS, one row more (read where the call staged it), and the two beside smaller ones."""
    _both_forms(svx_ctx, group_min, [(family, LDS_ROWS, 256)])
    _both_forms(svx_ctx, group_min, [(family, LDS_ROWS + 1, 256)])
    _both_forms(svx_ctx, group_min, [(family, 7, 5), (family, LDS_ROWS + 1, 256), (family, 3, 3), (family, LDS_ROWS, 256)], lanes=False)


def test_row_state_outside_lds(svx_ctx, group_min):
    """More than 24 KiB of row keys, rescan list and column flags: the state lives in the context's scratch — with the
    matrix in LDS (1 x 8192), with the matrix outside too (2100 x 16); 16 x 2100 keeps its state in LDS."""
    _both_forms(svx_ctx, group_min, [("ties", 1, 8192), ("wide", 3, 3), ("ties", 2100, 16), ("ties", 16, 2100), ("wide", 2, 6150)])


@pytest.mark.parametrize("nb,nc", [(1, 1024), (1024, 1)])
def test_one_against_a_thousand(svx_ctx, group_min, nb, nc):
    for family in M.FAMILIES:
        _both_forms(svx_ctx, group_min, [(family, nb, nc)])


@pytest.mark.parametrize("family", ("ties", "wide", "same_rows"))
def test_the_commands_worst_partition(svx_ctx, group_min, family):
    """512 x 512: the cap of 1024 members at its worst.  Group form only (a lane would need 10^8 reads)."""
    _both_forms(svx_ctx, group_min, [(family, 512, 512)], lanes=False)


def test_largest_partition(svx_ctx, group_min):
    """2^20 pairs as one row: a few eligible cells, the smallest of them late in the row."""
    n = _lib.MATCH_MAX_PAIRS
    dist = np.full(n, NONE, np.uint32)
    dist[[5, 70000, n - 3, n - 1]] = [9, 9, 2, 2]
    for setting in (GROUP, LANES, 0):
        group_min(setting)
        mb, mc = svx_ctx.match_greedy_batch(dist, [1], [n])
        assert mb.tolist() == [n - 3]
        assert np.flatnonzero(mc != NONE).tolist() == [n - 3] and mc[n - 3] == 0


def test_a_hundred_thousand_partitions(svx_ctx, group_min):
    parts = M.many_parts(100000)
    dist, n_base, n_comp, want_base, want_comp = M.batch(parts)
    assert len(n_base) == 100000 and int(n_base.max()) == 129
    for setting in (0, GROUP, LANES):
        group_min(setting)
        assert _run(svx_ctx, dist, n_base, n_comp) == (want_base, want_comp), setting


def test_poisoned_scratch(svx_ctx, group_min):
    """DESIGN's scratch contract: the call repeated after svx_ctx_scratch_fill with 0x00, 0xFF and 0xA5 — lanes, groups
    with matrix and state in LDS, and groups with either outside."""
    parts = [("ties", 7, 5), ("wide", 33, 65), ("ties", 1, 8192), ("ties", 2100, 16), ("same_rows", 40, 40), ("ties", 1, 1),
             ("wide", LDS_ROWS + 1, 256), ("ties", 0, 4), ("edge", 64, 64)]
    dist, n_base, n_comp, want_base, want_comp = M.batch(parts)
    for setting in (0, GROUP):
        group_min(setting)
        assert _run(svx_ctx, dist, n_base, n_comp) == (want_base, want_comp)
        for byte in (0x00, 0xFF, 0xA5):
            svx_ctx.scratch_fill(byte)
            assert _run(svx_ctx, dist, n_base, n_comp) == (want_base, want_comp), (setting, byte)


def test_argument_errors(svx_ctx, group_min):
    lib, h = svx_ctx.lib, svx_ctx.h
    one = np.ones(1, np.uint32)
    out_b, out_c = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data
    assert lib.svx_match_greedy_batch(None, p(one), p(one), p(one), 1, p(out_b), p(out_c)) == _lib.SVX_E_INVALID
    assert lib.svx_match_greedy_batch(h, None, None, None, 0, None, None) == _lib.SVX_OK
    assert lib.svx_match_greedy_batch(h, p(one), None, p(one), 1, p(out_b), p(out_c)) == _lib.SVX_E_INVALID
    assert lib.svx_match_greedy_batch(h, p(one), p(one), None, 1, p(out_b), p(out_c)) == _lib.SVX_E_INVALID
    assert lib.svx_match_greedy_batch(h, None, p(one), p(one), 1, p(out_b), p(out_c)) == _lib.SVX_E_INVALID
    assert lib.svx_match_greedy_batch(h, p(one), p(one), p(one), 1, None, p(out_c)) == _lib.SVX_E_INVALID
    assert lib.svx_match_greedy_batch(h, p(one), p(one), p(one), 1, p(out_b), None) == _lib.SVX_E_INVALID
    assert lib.svx_ctx_set_match_group_min(None, 4) == _lib.SVX_E_INVALID
    # more than 2^20 pairs: refused before anything is read or launched
    nb, nc = np.array([1, 1025], np.uint32), np.array([1, 1024], np.uint32)
    assert lib.svx_match_greedy_batch(h, p(one), p(nb), p(nc), 2, p(out_b), p(out_c)) == _lib.SVX_E_TOO_LARGE
    assert b"2^20" in lib.svx_last_error(h)
    with pytest.raises(_lib.SvxError):
        svx_ctx.match_greedy_batch([1, 2, 3], [1], [2])
    # and the context goes on working
    assert _run(svx_ctx, [3], [1], [1]) == ([0], [0])
