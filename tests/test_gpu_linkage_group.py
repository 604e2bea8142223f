"""The workgroup-per-partition complete linkage (k_linkage_group, svx_linkage.hip) against the lane path and scipy.

Every batch is clustered twice, with set_linkage_group_min(2) — every partition of two or more members on the group
kernel — and with set_linkage_group_min(LINKAGE_LANES_ONLY) — the lane path, which is all there was before —; the
labels must be equal between the two and equal to scipy's fcluster(linkage(y, "complete"), t, "distance").
Edit distances tie constantly, so four of the five distance families are made of ties."""
import functools

import numpy as np
import pytest

from svim_asm_amd import _lib

pytestmark = pytest.mark.gpu

LDS_N = _lib.LINKAGE_GROUP_LDS_N
SIZES = [2, 3, 10, 11, 33, 63, 64, 65, 255, 256, 257, LDS_N, LDS_N + 1]
LARGE = 600
CUTOFFS = (0.3, 2.0, 200.0)
FAMILIES = ("equal", "int4", "int50", "random", "tenths")


def _condensed(family, n):
    m = n * (n - 1) // 2
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + n)
    if family == "equal":
        return np.full(m, 7.0)
    if family == "int4":
        return rng.integers(0, 4, m).astype(np.float64)
    if family == "int50":
        return rng.integers(0, 50, m).astype(np.float64)
    if family == "random":
        return rng.random(m) * 3.0
    return 1 - rng.integers(0, 11, m) / 10.0


@functools.lru_cache(maxsize=None)
def _dendrogram(family, n):
    from scipy.cluster.hierarchy import linkage
    return linkage(_condensed(family, n), method="complete")


def _scipy_labels(family, n, cutoff):
    from scipy.cluster.hierarchy import fcluster
    if n == 1:
        return [1]
    return fcluster(_dendrogram(family, n), cutoff, criterion="distance").tolist()


def _batch(sizes):
    """Large and small partitions of every family interleaved in one launch, single members between them."""
    parts = []
    for n in sizes:
        for family in FAMILIES:
            parts.append((family, n))
        parts.append(("equal", 1))
    counts = np.array([n for _, n in parts], np.uint32)
    dist = np.concatenate([_condensed(f, n) for f, n in parts if n > 1])
    return parts, counts, dist


def _expected(parts, cutoff):
    return [l for f, n in parts for l in _scipy_labels(f, n, cutoff)]


@pytest.fixture
def group_min(svx_ctx):
    yield svx_ctx.set_linkage_group_min
    svx_ctx.set_linkage_group_min(0)


def _run_dev(ctx, dist, counts, cutoff):
    d_dist, d_n = ctx.dev_array(host=dist), ctx.dev_array(host=counts)
    d_lab = ctx.dev_array(nbytes=4 * int(counts.sum()))
    try:
        ctx._check(ctx.lib.svx_linkage_cut_batch_dev(ctx.h, d_dist.ptr, counts.ctypes.data, d_n.ptr, len(counts), float(cutoff),
                                                     d_lab.ptr))
        ctx.sync()
        return d_lab.download(np.uint32).tolist()
    finally:
        for d in (d_dist, d_n, d_lab):
            d.free()


@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_host_entry_group_equals_lanes_equals_scipy(svx_ctx, group_min, cutoff):
    parts, counts, dist = _batch(SIZES + [LARGE])
    group_min(2)
    grouped = svx_ctx.linkage_cut_batch(dist, counts, cutoff).tolist()
    group_min(_lib.LINKAGE_LANES_ONLY)
    lanes = svx_ctx.linkage_cut_batch(dist, counts, cutoff).tolist()
    assert grouped == lanes
    assert grouped == _expected(parts, cutoff)


@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_dev_entry_group_equals_lanes_equals_scipy(svx_ctx, group_min, cutoff):
    parts, counts, dist = _batch(SIZES)
    group_min(2)
    grouped = _run_dev(svx_ctx, dist, counts, cutoff)
    group_min(_lib.LINKAGE_LANES_ONLY)
    lanes = _run_dev(svx_ctx, dist, counts, cutoff)
    assert grouped == lanes
    assert grouped == _expected(parts, cutoff)


def test_threshold_between_the_two_kernels(svx_ctx, group_min):
    """A threshold inside the batch's sizes: both kernels in one call, and the default one."""
    parts, counts, dist = _batch([3, 15, 16, 17, 32, 33, 34, 70])
    want = _expected(parts, 2.0)
    for setting in (0, 16, 33, 64):
        group_min(setting)
        assert svx_ctx.linkage_cut_batch(dist, counts, 2.0).tolist() == want
        assert _run_dev(svx_ctx, dist, counts, 2.0) == want


def test_single_members_and_empty_batches(svx_ctx, group_min):
    for setting in (2, _lib.LINKAGE_LANES_ONLY):
        group_min(setting)
        assert svx_ctx.linkage_cut_batch([], [], 0.3).tolist() == []
        assert svx_ctx.linkage_cut_batch([], [1, 1, 1], 0.3).tolist() == [1, 1, 1]
        assert svx_ctx.linkage_cut_batch([5.0], [1, 2, 1], 4.0).tolist() == [1, 1, 2, 1]
        assert svx_ctx.lib.svx_linkage_cut_batch(svx_ctx.h, None, None, 0, 0.3, None) == 0
        assert svx_ctx.lib.svx_linkage_cut_batch_dev(svx_ctx.h, None, None, None, 0, 0.3, None) == 0
        ones = np.ones(3, np.uint32)
        assert _run_dev(svx_ctx, np.zeros(1), ones, 0.3) == [1, 1, 1]
