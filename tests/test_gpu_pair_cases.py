"""The pair sort's kernels and host plans (svim_asm_amd/csrc/svx_pair.hip) held to the case table of tests/pair_cases.py:
every case on the one-launch plan, the radix plan and the wait-free plan — windows at 5120 | 5121 keys with counting
passes on both sides, 1 to 5 and 32 | 33 gathered runs, empty windows, cuts on bucket borders, every digit plan from 5 to
64 live bits, the sweep at 8192 | 8193, 16384 | 16385 and with two chunks per workgroup, k_key_or's stride loop —
against the C oracle, which tests/test_pair_cases.py holds to a numpy restatement of form_partitions where there is no
GPU.  perm, part_id and n_parts are compared for equality.  The random-key tests of tests/test_gpu_pair.py stay as they
are; the waits between workgroups running out are tests/test_gpu_ctx.py's."""
import functools

import numpy as np
import pytest

from oracle import orc
from tests import pair_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(params=P.PLANS)
def plan(request, svx_ctx):
    """As in tests/test_gpu_pair.py: the one-launch plan, the radix plan (svx_ctx_set_pair_single_launch_max(0)) and the
    plan without waits between workgroups (svx_ctx_set_pair_wait_free(1)); restored afterwards."""
    svx_ctx.set_pair_single_launch_max(0 if request.param == "radix" else P.SINGLE_LAUNCH_MAX)
    svx_ctx.set_pair_wait_free(request.param == "wait_free")
    yield request.param
    svx_ctx.set_pair_single_launch_max(P.SINGLE_LAUNCH_MAX)
    svx_ctx.set_pair_wait_free(False)


@functools.lru_cache(maxsize=None)
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def expected(name, max_dist):
    """The oracle's answer, once per (case, distance) and module."""
    keys = P.combined()[0] if name == "combined" else P.CASES[name].keys
    perm, part, n_parts = orc.pair_partition(keys, max_dist)
    for a in (perm, part):
        a.setflags(write=False)
    return perm, part, n_parts


def keys_of(name):
    return P.combined()[0] if name == "combined" else P.CASES[name].keys


def run(svx_ctx, name, max_dist, what=""):
    perm, part, n_parts = svx_ctx.pair_partition(keys_of(name), max_dist)
    e_perm, e_part, e_n = expected(name, max_dist)
    where = "%s, max_dist %d %s" % (name, max_dist, what)
    assert n_parts == e_n, where
    assert np.array_equal(perm, e_perm), where
    assert np.array_equal(part, e_part), where


def grid_of(name):
    """The one-launch grid of a case (None where the batch is too large for that plan)."""
    n = len(keys_of(name))
    if n > P.SINGLE_LAUNCH_MAX:
        return None
    grid_max = min(P.K["SINGLE_GRID_MAX"], max(1, n_cu() // 4))
    return -(-n // max(-(-n // grid_max), P.WG))


def test_the_table_holds_on_this_device():
    """The cases reach their classes through the device's CU count (the one-launch grid, the sweep's grid, k_key_or's):
    on a device with another count the table has to be moved — this fails, it does not skip."""
    cus = n_cu()
    try:
        P.check_preconditions(n_cu=cus)
    except AssertionError as e:
        raise AssertionError("this device has %d CUs; tests/pair_cases.py is laid out for 256 and has to move with the device: %s" % (cus, e))


@pytest.mark.parametrize("family", P.FAMILIES)
def test_every_case(svx_ctx, plan, family):
    """perm, part_id and n_parts of every case at every distance it names.  The one-launch plan's two sets of arrival
    counters alternate from launch to launch: there every case runs three times in a row (both sets meet its grid, and
    the next case begins on the other set than this one did) and, where the launch before it had the same grid, behind a
    case of another grid."""
    cases = [c for c in P.family(family) if plan in c.plans]
    assert cases
    last_grid = None
    for c in cases:
        for d in c.max_dists:
            grid = grid_of(c.name) if plan == "single_launch" else None
            if grid is None:
                run(svx_ctx, c.name, d)
                continue
            if grid == last_grid:
                other = "grid-1025-keys-two-windows" if grid != 2 else "grid-1024-keys-one-window"
                run(svx_ctx, other, 0)
            for rep in range(3):
                run(svx_ctx, c.name, d, "(call %d of 3)" % (rep + 1))
            last_grid = grid


def default_superset(keys):
    """Every bit between the lowest and the highest live one of each half, and the neighbours of both."""
    bits = int(np.bitwise_or.reduce(keys))
    lo, hi = bits & 0xFFFFFFFF, bits >> 32
    return bits | ((1 << max(lo.bit_length() + 1, 1)) - 1) & 0xFFFFFFFF | (((1 << (hi.bit_length() + 1)) - 1) & 0xFFFFFFFF) << 32


@pytest.mark.parametrize("family", P.DEVICE_ENTRY_FAMILIES)
def test_device_entry_points(svx_ctx, plan, family):
    """svx_pair_partition_dev (k_key_or derives the live bits) and svx_pair_partition_dev_bits with exactly the live bits
    and with a superset (the case's own where it names one): other fields, another `live`, other windows, same result.
    The output buffers are zeroed before every call."""
    for c in P.family(family):
        if plan not in c.plans:
            continue
        n = len(c.keys)
        exact = int(np.bitwise_or.reduce(c.keys))
        superset = c.superset if c.superset is not None else default_superset(c.keys)
        assert superset & exact == exact and (superset != exact or exact == (1 << 64) - 1), c.name
        d_keys = svx_ctx.dev_array(c.keys)
        d_perm, d_part = svx_ctx.dev_array(nbytes=4 * n), svx_ctx.dev_array(nbytes=4 * n)
        d_np = svx_ctx.dev_array(np.zeros(1, np.uint32))
        zeros = np.zeros(n, np.uint32)
        try:
            for d in c.max_dists:
                e_perm, e_part, e_n = expected(c.name, d)
                for bits in (None, exact, superset):
                    for buf in (d_perm, d_part):
                        svx_ctx._check(svx_ctx.lib.svx_dev_upload(svx_ctx.h, buf.ptr, zeros.ctypes.data, zeros.nbytes))
                    svx_ctx._check(svx_ctx.lib.svx_dev_upload(svx_ctx.h, d_np.ptr, zeros.ctypes.data, 4))
                    if bits is None:
                        rc = svx_ctx.lib.svx_pair_partition_dev(svx_ctx.h, d_keys.ptr, n, d, d_perm.ptr, d_part.ptr, d_np.ptr)
                    else:
                        rc = svx_ctx.lib.svx_pair_partition_dev_bits(svx_ctx.h, d_keys.ptr, n, d, bits, d_perm.ptr, d_part.ptr, d_np.ptr)
                    where = "%s, max_dist %d, bits %s" % (c.name, d, "derived" if bits is None else hex(bits))
                    assert rc == 0, where
                    svx_ctx.sync()
                    assert int(d_np.download(np.uint32)[0]) == e_n, where
                    assert np.array_equal(d_perm.download(np.uint32), e_perm), where
                    assert np.array_equal(d_part.download(np.uint32), e_part), where
        finally:
            for buf in (d_keys, d_perm, d_part, d_np):
                buf.free()


def test_combined_batch(svx_ctx, plan):
    """The small cases as one batch (each under a group field of its own): other windows, other slices, same keys."""
    for d in (0, 1):
        for rep in range(3 if plan == "single_launch" else 1):
            run(svx_ctx, "combined", d, "(call %d)" % (rep + 1))


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_poisoned_scratch(svx_ctx, plan, byte):
    """The storage and sweep cases on scratch filled with a byte: the HBM halves of a crowded window, the rows, the
    histograms and block_tot are written before they are read.  (The two-chunk sweep case runs once per plan in
    test_every_case, not once per byte.)"""
    for fam in P.POISON_FAMILIES:
        for c in P.family(fam):
            if plan not in c.plans or c.name == P.TWO_CHUNK_CASE:
                continue
            for d in c.max_dists:
                svx_ctx.scratch_fill(byte)
                run(svx_ctx, c.name, d, "(scratch 0x%02X)" % byte)
