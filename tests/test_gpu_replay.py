"""svx_variant_replay on the device (svim_asm_amd/csrc/svx_replay.hip) against the loop of tests/replay_restatement.py,
element for element: every case of tests/replay_cases.py (what each shows is held there, where there is no GPU) with the
strings downloaded and with the strings left in the workspace; the cap convention; empty calls; every refusal with the
context usable afterwards; poisoned scratch, held against the loop and never against an earlier call; and 200 seeded
random calls."""
import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import replay_cases as T
from tests import replay_restatement as RR

pytestmark = pytest.mark.gpu


def assert_equals(got, exp, strings=True):
    assert got["out_len"].dtype == np.uint32 and got["status"].dtype == np.uint8 and got["equal"].dtype == np.uint8
    assert got["status"].tolist() == exp["status"]
    assert got["out_len"].tolist() == exp["out_len"]
    bad = [(k, g, x) for k, (g, x) in enumerate(zip(got["equal"].tolist(), exp["equal"])) if g != x]
    assert not bad, bad[:10]
    assert got["total"] == exp["total"]
    if strings:
        assert got["out_off"].tolist() == exp["out_off"]
        if got["out"].tobytes() != exp["out"]:
            g = got["out"].tobytes()
            at = next(i for i in range(min(len(g), len(exp["out"]))) if g[i] != exp["out"][i]) if len(g) == len(exp["out"]) else -1
            raise AssertionError("strings differ from byte %d on: %r, expected %r" % (at, g[max(at, 0):at + 24], exp["out"][max(at, 0):at + 24]))


def check(ctx, args, exp=None):
    exp = exp or RR.replay_batch(*args)
    assert_equals(ctx.variant_replay(*args, strings=True), exp)
    assert_equals(ctx.variant_replay(*args), exp, strings=False)
    return exp


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_case(svx_ctx, name):
    check(svx_ctx, T.case(name), T.expected(name))


def test_pairs_alone_and_jobs_alone(svx_ctx):
    args = T.case("pairs")
    exp = T.expected("pairs")
    none = np.zeros(0, np.uint32)
    got = svx_ctx.variant_replay(*args[:8], none, none, strings=True)
    assert len(got["equal"]) == 0 and got["out"].tobytes() == exp["out"] and got["out_len"].tolist() == exp["out_len"]
    # every pair the other way round
    got = svx_ctx.variant_replay(*args[:8], args[9], args[8])
    assert got["equal"].tolist() == exp["equal"]


def test_empty_calls(svx_ctx):
    pool = np.frombuffer(b"ACGT", np.uint8)
    e32, e64 = np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    for bases in (pool, pool[:0]):
        got = svx_ctx.variant_replay(bases, e64, e32, np.zeros(1, np.uint32), e32, e32, e64, e32, strings=True)
        assert got["total"] == 0 and got["out_off"].tolist() == [0] and len(got["out"]) == 0 and len(got["out_len"]) == 0
    # jobs without edits and without pairs; one job without anything
    args = (pool, [0, 1, 4], [4, 2, 0], [0, 0, 0, 0], e32, e32, e64, e32)
    check(svx_ctx, args)
    check(svx_ctx, (pool[:0], [0], [0], [0, 0], e32, e32, e64, e32, [0], [0]))


def test_the_cap_convention(svx_ctx):
    args, exp = T.case("out-lengths-in-a-row"), T.expected("out-lengths-in-a-row")
    total = exp["total"]
    for cap in (0, 1, total - 1):
        with pytest.raises(_lib.SvxError) as ei:
            svx_ctx.variant_replay(*args, strings=True, cap=cap)
        assert ei.value.status == _lib.SVX_E_CAPACITY
        part = ei.value.partial
        assert part["total"] == total and part["out"].tobytes() == exp["out"][:cap]
        assert part["out_off"].tolist() == exp["out_off"] and part["out_len"].tolist() == exp["out_len"]
        assert part["status"].tolist() == exp["status"]
    for cap in (total, total + 100):
        assert_equals(svx_ctx.variant_replay(*args, strings=True, cap=cap), exp)
    # out == NULL with a cap: the cap is ignored, the total and the offsets are served
    lib, h = svx_ctx.lib, svx_ctx.h
    a = [np.ascontiguousarray(x) for x in args]
    n_jobs = len(a[1])
    out_len, status, off = np.zeros(n_jobs, np.uint32), np.zeros(n_jobs, np.uint8), np.zeros(n_jobs + 1, np.uint32)
    import ctypes as C
    n = C.c_uint64(7)
    rc = lib.svx_variant_replay(h, a[0].ctypes.data, len(a[0]), a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, n_jobs, a[4].ctypes.data,
                                a[5].ctypes.data, a[6].ctypes.data, a[7].ctypes.data, len(a[4]), None, None, 0, out_len.ctypes.data,
                                status.ctypes.data, None, None, off.ctypes.data, 3, C.byref(n))
    assert rc == 0 and n.value == total and off.tolist() == exp["out_off"] and out_len.tolist() == exp["out_len"]
    rc = lib.svx_variant_replay(h, a[0].ctypes.data, len(a[0]), a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, n_jobs, a[4].ctypes.data,
                                a[5].ctypes.data, a[6].ctypes.data, a[7].ctypes.data, len(a[4]), None, None, 0, out_len.ctypes.data,
                                status.ctypes.data, None, None, None, 0, None)
    assert rc == 0 and status.tolist() == exp["status"]


def test_refusals_leave_the_context_usable(svx_ctx):
    c = T.Call(77)
    c.job(b"ACGTACGT", [(2, 1, b"T"), (5, 0, b"GG")])
    c.job(b"ACTTAGGCGT", [])
    c.pair(0, 1)
    good = c.args()
    exp = RR.replay_batch(*good)
    assert exp["equal"] == [1]
    names = ("bases", "win_off", "win_len", "ed_first", "ed_start", "ed_ref_len", "ed_alt_off", "ed_alt_len", "pair_a", "pair_b")
    n_bases = len(good[0])

    def refused(word, status=_lib.SVX_E_INVALID, **change):
        args = [np.array(x) for x in good]
        for name, (at, value) in change.items():
            args[names.index(name)][at] = value
        with pytest.raises(_lib.SvxError) as ei:
            svx_ctx.variant_replay(*args)
        assert ei.value.status == status and word in str(ei.value), str(ei.value)
        assert_equals(svx_ctx.variant_replay(*good, strings=True), exp)
    refused("ed_first[0]", ed_first=(0, 1))
    refused("decreases at job 1", ed_first=(1, 3))
    refused("ends at 3", ed_first=(2, 3))                  # its last entry is not n_edits
    refused("window of job 1", win_off=(1, n_bases - 9))
    refused("window of job 0", win_len=(0, n_bases))
    refused("window of job 1", win_off=(1, n_bases + 1))
    refused("edit 1 (job 0)", ed_alt_len=(1, n_bases))
    refused("edit 0 (job 0)", ed_alt_off=(0, n_bases + 1))
    refused("pair 0", pair_a=(0, 2))
    refused("pair 0", pair_b=(0, 0xFFFFFFFF))
    # a window and an allele that end exactly at the pool's end are taken
    args = [np.array(x) for x in good]
    args[1][1], args[2][1] = n_bases - 3, 3
    args[6][1], args[7][1] = n_bases - 2, 2
    check(svx_ctx, args)
    # null pointers where a count is positive: the C entry itself
    lib, h = svx_ctx.lib, svx_ctx.h
    a = [np.ascontiguousarray(x) for x in good]
    out_len, status, equal = np.zeros(2, np.uint32), np.zeros(2, np.uint8), np.zeros(1, np.uint8)
    full = [a[0].ctypes.data, len(a[0]), a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, 2, a[4].ctypes.data, a[5].ctypes.data,
            a[6].ctypes.data, a[7].ctypes.data, 2, a[8].ctypes.data, a[9].ctypes.data, 1, out_len.ctypes.data, status.ctypes.data,
            equal.ctypes.data, None, None, 0, None]
    assert lib.svx_variant_replay(h, *full) == 0 and equal.tolist() == [1]
    for at in (0, 2, 3, 4, 6, 7, 8, 9, 11, 12, 14, 15, 16):
        args = list(full)
        args[at] = None
        assert lib.svx_variant_replay(h, *args) == _lib.SVX_E_INVALID, at
    assert lib.svx_variant_replay(h, *full) == 0
    # more window and allele bytes than the 32-bit offsets hold: one window of 2^20 bytes in 4096 jobs; nothing is launched
    big = np.zeros(1 << 20, np.uint8)
    n = 4096
    with pytest.raises(_lib.SvxError) as ei:
        svx_ctx.variant_replay(big, np.zeros(n, np.uint64), np.full(n, 1 << 20, np.uint32), np.zeros(n + 1, np.uint32), [], [], [], [])
    assert ei.value.status == _lib.SVX_E_TOO_LARGE and str(_lib.REPLAY_MAX_BYTES) in str(ei.value)
    assert_equals(svx_ctx.variant_replay(*good, strings=True), exp)


@pytest.mark.parametrize("fill", (0x00, 0xFF, 0xA5))
def test_poisoned_scratch(svx_ctx, fill):
    for name in ("edit-counts", "pairs", "status", "job-boundary+0"):
        args, exp = T.case(name), T.expected(name)
        svx_ctx.variant_replay(*args, strings=True)  # (the regions exist and have their size)
        svx_ctx.scratch_fill(fill)
        assert_equals(svx_ctx.variant_replay(*args, strings=True), exp)
        svx_ctx.scratch_fill(fill)
        assert_equals(svx_ctx.variant_replay(*args), exp, strings=False)


def test_random_calls(svx_ctx):
    seen = {0: 0, 1: 0, 2: 0}
    equal = 0
    for seed in range(200):
        exp = check(svx_ctx, T.case_random(1000 + seed).args())
        for s in exp["status"]:
            seen[s] += 1
        equal += sum(exp["equal"])
    assert min(seen.values()) > 10 and equal > 50
