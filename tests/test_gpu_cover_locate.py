"""svx_cover_locate on the device (svim_asm_amd/csrc/svx_cover.hip) against the plain loop of tests/lift_restatement.py
on the lists of tests/cover_cases.py: every index, `!= NONE` equal to svx_cover_query's bit on the same inputs, the
lowest index among equal end keys, a winner that reaches the last pass through the carry, poisoned scratch, refusals."""
import functools

import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import cover_cases as K, cover_restatement as R, lift_restatement as LR
from tests.test_gpu_cover import arrays

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def located(name):
    return LR.locate(*K.CASES[name]())


def on_device(ctx, lists, queries):
    got = ctx.cover_locate(*arrays(lists, queries))
    assert got.dtype == np.uint32 and got.shape == (len(lists), len(queries))
    return got.tolist()


def test_the_restatements_agree():
    for name in K.CASES:
        assert [[int(i != LR.NONE) for i in row] for row in located(name)] == K.answers(name)
    assert LR.NONE == _lib.COVER_NONE


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_index_equals_the_restatement_and_none_is_cover_querys_zero(svx_ctx, name):
    lists, queries = K.CASES[name]()
    got = on_device(svx_ctx, lists, queries)
    assert got == located(name)
    bits = svx_ctx.cover_query(*arrays(lists, queries))
    assert np.array_equal(np.array(got, dtype=np.uint32) != _lib.COVER_NONE, bits.astype(bool))
    # the entry named does contain the window
    for ivs, row in zip(lists, got):
        for (lo, hi), i in zip(queries, row):
            assert i == LR.NONE or (ivs[i][0] <= lo and ivs[i][1] >= hi)


@pytest.mark.parametrize("n_q", K.QUERY_COUNTS)
def test_query_counts(svx_ctx, n_q):
    lists, queries = K.mixed()
    assert on_device(svx_ctx, lists, queries[:n_q]) == [row[:n_q] for row in located("mixed")]


def test_more_lists_than_one_launch_takes_side_by_side(svx_ctx):
    """tests/test_gpu_cover.py's batch of GRID_Y + 2 lists: the second trip of k_locate_search's threads."""
    lists, queries = K.many_lists()
    expected = LR.locate(lists, queries)
    assert [[int(i != LR.NONE) for i in row] for row in expected] == K.many_lists_answers()
    assert expected[0] != expected[K.GRID_Y] and expected[1] != expected[K.GRID_Y + 1]
    assert {0, 1, LR.NONE} == set(i for row in expected for i in row)
    got = svx_ctx.cover_locate(*arrays(lists, queries))
    assert got.dtype == np.uint32 and got.shape == (len(lists), 3)
    assert np.array_equal(got, np.array(expected, dtype=np.uint32))


def equal_ends():
    """Runs of entries with one end key, spread over lanes, waves and passes: the lowest index of the run wins."""
    c = 3
    ivs = [(R.key(c, 10 * k), R.key(c, 50000 + 1000 * (k // 700))) for k in range(3000)]
    queries = [(R.key(c, 10 * k + 3), R.key(c, 50000 + 1000 * (k // 700))) for k in range(0, 3000, 37)]
    queries += [(R.key(c, 10 * k + 3), R.key(c, 50000 + 1000 * (k // 700) + 1)) for k in range(0, 3000, 91)]
    return [ivs], queries


def test_equal_end_keys_the_lowest_index_wins(svx_ctx):
    lists, queries = equal_ends()
    K.check_inputs(lists, queries)
    expected = LR.locate(lists, queries)
    assert set(expected[0]) >= {0, 700, 1400, 2100, 2800, LR.NONE}
    assert on_device(svx_ctx, lists, queries) == expected


def test_the_winner_of_pass_0_arrives_through_the_carry(svx_ctx):
    """Three passes of 1024: entry 5 ends behind everything, so every query of passes 1 and 2 is answered with an index
    the scan carried over two pass borders."""
    n = 2 * K.CHUNK + 300
    ivs = [(R.key(0, 20 * k), R.key(0, 20 * k + 15)) for k in range(n)]
    ivs[5] = (ivs[5][0], R.key(0, 20 * n + 100))
    queries = [(R.key(0, 20 * k + 2), R.key(0, 20 * k + 40)) for k in range(0, n, 13)] + \
              [(R.key(0, 20 * k + 2), R.key(0, 20 * n + 101)) for k in range(7, n, 257)] + [(R.key(0, 20 * k), R.key(0, 20 * k + 15)) for k in range(5)]
    expected = LR.locate([ivs], queries)
    assert expected[0].count(5) > 150 and LR.NONE in expected[0] and {0, 1, 2, 3, 4} <= set(expected[0])
    assert on_device(svx_ctx, [ivs], queries) == expected


def test_no_lists_and_lists_without_entries(svx_ctx):
    lists, queries = K.mixed()
    assert svx_ctx.cover_locate(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(1, np.uint64),
                                *arrays(lists, queries)[3:]).shape == (0, len(queries))
    assert on_device(svx_ctx, [[], [], []], queries[:70]) == [[LR.NONE] * 70] * 3


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_answers_do_not_depend_on_what_scratch_held(svx_ctx, byte):
    lists, queries = K.mixed()
    assert on_device(svx_ctx, lists, queries) == located("mixed")  # (the regions exist from here on)
    svx_ctx.scratch_fill(byte)
    assert on_device(svx_ctx, lists, queries) == located("mixed")
    svx_ctx.scratch_fill(byte)
    assert on_device(svx_ctx, *K.nested()) == located("nested")


@pytest.mark.parametrize("what", ["unsorted list", "interval across contigs", "query across contigs", "lo > hi"])
def test_invalid_inputs_are_refused_as_cover_query_refuses_them(svx_ctx, what):
    lists, queries = K.empty_between()
    lists, queries = [list(ivs) for ivs in lists], list(queries)
    if what == "unsorted list":
        lists[2][400], lists[2][401] = lists[2][401], lists[2][400]
        assert lists[2][400][0] > lists[2][401][0]
    elif what == "interval across contigs":
        s, e = lists[0][17]
        lists[0][17] = (s, e + (1 << 32))
    elif what == "query across contigs":
        queries[5] = (queries[5][0], queries[5][1] + (1 << 32))
    else:
        queries[9] = (queries[9][1] + 1, queries[9][1])
    messages = []
    for call in (svx_ctx.cover_locate, svx_ctx.cover_query):
        with pytest.raises(_lib.SvxError) as e:
            call(*arrays(lists, queries))
        assert e.value.status == _lib.SVX_E_INVALID
        messages.append(str(e.value).replace("svx_cover_locate", "X").replace("svx_cover_query", "X"))
    assert messages[0] == messages[1]  # one checker
    start, end, off, lo, hi = arrays(*K.empty_between())
    off[0] = 1
    with pytest.raises(_lib.SvxError) as e:
        svx_ctx._check(svx_ctx.lib.svx_cover_locate(svx_ctx.h, start.ctypes.data, end.ctypes.data, off.ctypes.data, 3, lo.ctypes.data,
                                                     hi.ctypes.data, len(lo), np.zeros(3 * len(lo), np.uint32).ctypes.data))
    assert e.value.status == _lib.SVX_E_INVALID
    assert on_device(svx_ctx, *K.empty_between()) == located("empty_between")
