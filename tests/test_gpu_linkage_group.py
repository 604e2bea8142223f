"""The workgroup-per-partition complete linkage (k_linkage_group, svx_linkage.hip) against the lane path and scipy.

Every batch is clustered twice, with set_linkage_group_min(2) — every partition of two or more members on the group
kernel — and with set_linkage_group_min(LINKAGE_LANES_ONLY) — the lane path, which is all there was before —; the
labels must be equal between the two and equal to scipy's fcluster(linkage(y, "complete"), t, "distance").
Edit distances tie constantly, so four of the five distance families are made of ties.

The kernel's last size class (513 ... 2048 members, matrix in the workspace) is held to scipy alone — a lane needs
seconds at these sizes —: 512 | 513, the product's cap of 1024, 2047 | 2048, and 2049, the first size the group kernel
hands back to the lanes.  One more batch mixes everything that shares the call's scratch buffer at the default
threshold: lane partitions on HBM scratch (11-15 members) between group partitions with their matrix in LDS and in
the workspace, the offsets computed by the host entry (plan_add) and by the device entry (k_linkage_offsets)."""
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


# ------------------------------------------------------------------------------ the last size class, against scipy alone
BIG = [512, 513, 1024, 2047, 2048]


def _big_batch(n):
    """The five families at n members, single members and a few partitions of 3 between them."""
    parts = []
    for family in FAMILIES:
        parts += [(family, n), ("equal", 1), (family, 3)]
    counts = np.array([m for _, m in parts], np.uint32)
    dist = np.concatenate([_condensed(f, m) for f, m in parts if m > 1])
    return parts, counts, dist


@pytest.mark.parametrize("n", BIG)
def test_last_size_class_equals_scipy_on_both_entries(svx_ctx, group_min, n):
    parts, counts, dist = _big_batch(n)
    group_min(2)
    for cutoff in CUTOFFS:
        want = _expected(parts, cutoff)
        assert svx_ctx.linkage_cut_batch(dist, counts, cutoff).tolist() == want
        assert _run_dev(svx_ctx, dist, counts, cutoff) == want


def test_first_size_handed_back_to_the_lanes(svx_ctx):
    """2049 members beside 2048 and 16 at the default settings: the group kernel's largest size and the lane path's
    HBM scratch slice in one call.  (The 2049-member lane takes seconds: one family, one cut-off.)"""
    parts = [("int4", 2048), ("int4", 16), ("int4", 2049)]
    counts = np.array([m for _, m in parts], np.uint32)
    dist = np.concatenate([_condensed(f, m) for f, m in parts])
    assert svx_ctx.linkage_cut_batch(dist, counts, 2.0).tolist() == _expected(parts, 2.0)


def test_lane_scratch_and_group_matrices_share_one_buffer(svx_ctx):
    """Default threshold (16): 11-15 members are lanes on HBM scratch, 129 and more are group partitions with their
    matrix in the same buffer, 1 takes nothing.  Both entries; then the device entry again behind 300 partitions of two
    and three members, so that k_linkage_offsets (256 threads) walks chunks of two partitions."""
    sizes = [11, 300, 13, 129, 15, 513, 12, 1, 1024, 14]
    parts = [(FAMILIES[i % len(FAMILIES)], n) for i, n in enumerate(sizes)]
    front = [(FAMILIES[i % len(FAMILIES)], 2 + i % 2) for i in range(300)]
    for batch in (parts, front + parts):
        counts = np.array([m for _, m in batch], np.uint32)
        dist = np.concatenate([_condensed(f, m) for f, m in batch if m > 1])
        want = _expected(batch, 2.0)
        assert _run_dev(svx_ctx, dist, counts, 2.0) == want
        assert svx_ctx.linkage_cut_batch(dist, counts, 2.0).tolist() == want
