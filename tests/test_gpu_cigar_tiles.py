"""The case table of the CIGAR tile walk (tests/cigar_tile_cases.py) on the device: every case, element for element on
all five output columns, against the numpy restatement of the walk (tests/cigar_long_cases.restated_extract, which
tests/test_cigar_tile_cases.py holds to the C oracle) — on both paths (tiles of 4096 ops and five launches; tiles of 1024
ops and two), in the packed and the SoA layout, with ref_start given and NULL, through the host entries and through
svx_cigar_extract_dev / svx_cigar_extract_soa_dev.

Streaming path: after every call the workspace header's word 2, the dense-tile count the descriptor scan published, is
held to EXACTLY the dense set facts() derives from the input (count > SLAB, or a round with count > QUEUE), and words 0
and 1 to zero.  That makes the thresholds observable: a tile that goes dense one signature early or late still computes
the right records.  A call with another count goes in front of every such call, so that a stale word cannot pass.

Two-launch path: it has no such observable (its dense tiles are marked in the folded descriptors and consumed by the
same submission); there the result alone is held.

One test function per class family, not one pytest item per case and setting: a case takes 32 calls."""
import ctypes as C
import functools

import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import cigar_long_cases as LC
from tests import cigar_tile_cases as TC
from tests import test_gpu_collect as tcol

pytestmark = pytest.mark.gpu
KEYS = ("aln", "ref_pos", "read_pos", "len", "type")
DTYPES = (np.uint32, np.uint32, np.uint32, np.uint32, np.uint8)
W_COUNTER, W_TICKET, W_PUBLISHED = 0, 1, 2
SENTINEL, GUARD = 0xAB, 16   # byte of the untouched output rows; rows behind the capacity


@functools.lru_cache(maxsize=None)
def expected(name, with_ref_start):
    c = TC.CASES[name]
    rs = c.ref_start if with_ref_start else np.zeros_like(c.ref_start)
    return LC.restated_extract(c.cigar, c.aln_off, rs, TC.MIN_LEN)


def assert_same(got, exp, what):
    for k in KEYS:
        assert len(got[k]) == len(exp[k]), (what, k, len(got[k]), len(exp[k]))
        bad = np.nonzero(got[k] != exp[k])[0]
        assert not len(bad), (what, k, "first difference at row", int(bad[0]), int(got[k][bad[0]]), int(exp[k][bad[0]]))


class Device:
    """The arrays of one batch in HBM for the *_dev entries, with output buffers of `rows` + GUARD rows."""

    def __init__(self, ctx, cigar, aln_off, ref_start, rows):
        self.ctx, self.n_ops, self.n_aln, self.rows = ctx, len(cigar), len(aln_off) - 1, rows
        self.cig = ctx.dev_array(cigar)
        self.len = ctx.dev_array((cigar >> 4).astype(np.uint32))
        self.op = ctx.dev_array(np.concatenate(((cigar & 15).astype(np.uint8), np.zeros(16, np.uint8))))
        self.off = ctx.dev_array(np.asarray(aln_off, np.uint64))
        self.rs = ctx.dev_array(np.asarray(ref_start, np.int32))
        self.fill = [np.full(rows + GUARD, SENTINEL, np.uint8).repeat(np.dtype(dt).itemsize) for dt in DTYPES]
        self.outs = [ctx.dev_array(f) for f in self.fill]
        self.n = ctx.dev_array(np.zeros(1, np.uint64))

    def call(self, soa, with_rs, cap, min_len=TC.MIN_LEN):
        """One call with fresh sentinels -> (count, the output buffers whole)."""
        ctx = self.ctx
        for o, f in zip(self.outs, self.fill):
            ctx._check(ctx.lib.svx_dev_upload(ctx.h, o.ptr, f.ctypes.data, f.nbytes))
        ctx.sync()
        sig = _lib.SigSoa(*[o.ptr for o in self.outs])
        rs = self.rs.ptr if with_rs else None
        if soa:
            rc = ctx.lib.svx_cigar_extract_soa_dev(ctx.h, self.op.ptr, self.len.ptr, self.n_ops, self.off.ptr, self.n_aln, rs,
                                                   min_len, sig, cap, self.n.ptr)
        else:
            rc = ctx.lib.svx_cigar_extract_dev(ctx.h, self.cig.ptr, self.n_ops, self.off.ptr, self.n_aln, rs, min_len, sig, cap,
                                               self.n.ptr)
        assert rc == 0, rc
        ctx.sync()
        return int(self.n.download(np.uint64)[0]), [o.download(dt) for o, dt in zip(self.outs, DTYPES)]

    def free(self):
        for a in [self.cig, self.len, self.op, self.off, self.rs, self.n] + self.outs:
            a.free()


def check_rows(bufs, exp, k, what):
    """Rows [0, k) are the expected ones, every byte behind them is the sentinel's."""
    for b, key, dt in zip(bufs, KEYS, DTYPES):
        bad = np.nonzero(b[:k] != exp[key][:k])[0]
        assert not len(bad), (what, key, "first difference at row", int(bad[0]), int(b[bad[0]]), int(exp[key][bad[0]]))
        assert (b[k:].view(np.uint8) == SENTINEL).all(), (what, key, "rows behind the first %d were written" % k)


class Primer:
    """A streaming call of two all-indel tiles (published count 2), or of none (0): made in front of a call whose
    published count is checked, with the other count, so that the word has to be written by the call under test."""

    def __init__(self, ctx):
        dense = np.full(2 * TC.TILE, (50 << 4) | 1, np.uint32)
        sparse = np.full(2 * TC.TILE, (50 << 4) | 0, np.uint32)
        off, rs = np.array([0, 2 * TC.TILE], np.uint64), np.zeros(1, np.int32)
        self.ctx, self.dev = ctx, {2: Device(ctx, dense, off, rs, 0), 0: Device(ctx, sparse, off, rs, 0)}

    def before(self, n_dense):
        other = 0 if n_dense == 2 else 2
        self.ctx.set_small_batch_ops(0)
        self.dev[other].call(False, False, 0)
        assert int(self.ctx.scratch_header()[W_PUBLISHED]) == other

    def free(self):
        for d in self.dev.values():
            d.free()


@pytest.fixture(scope="module")
def primer(svx_ctx):
    p = Primer(svx_ctx)
    yield p
    svx_ctx.set_small_batch_ops(1 << 23)
    p.free()


def check_header(ctx, n_dense, what):
    h = ctx.scratch_header()
    assert int(h[W_COUNTER]) == 0 and int(h[W_TICKET]) == 0, (what, h[:3])
    assert int(h[W_PUBLISHED]) == n_dense, (what, "published dense tiles", int(h[W_PUBLISHED]), "facts", n_dense)


def run_everywhere(ctx, primer, name, cigar, aln_off, ref_start, exp_rs, exp_no_rs, dense_streaming,
                   entries=("host", "dev"), ref_starts=(True, False)):
    """One batch in every setting of the module docstring."""
    op, ln = (cigar & 15).astype(np.uint8), (cigar >> 4).astype(np.uint32)
    n_exp = len(exp_rs["aln"])
    dev = Device(ctx, cigar, aln_off, ref_start, n_exp) if "dev" in entries else None
    try:
        for path in TC.PATHS:
            streaming = path == "streaming"
            for soa in (False, True):
                for with_rs in ref_starts:
                    exp = exp_rs if with_rs else exp_no_rs
                    for entry in entries:
                        what = (name, path, "soa" if soa else "packed", "ref_start" if with_rs else "NULL", entry)
                        if streaming:
                            primer.before(dense_streaming)
                        ctx.set_small_batch_ops(0 if streaming else 1 << 23)
                        if entry == "host":
                            rs = ref_start if with_rs else None
                            got = ctx.cigar_extract(ln, aln_off, rs, TC.MIN_LEN, op=op) if soa else ctx.cigar_extract(cigar, aln_off, rs, TC.MIN_LEN)
                            assert_same(got, exp, what)
                        else:
                            n, bufs = dev.call(soa, with_rs, n_exp)
                            assert n == n_exp, (what, n, n_exp)
                            check_rows(bufs, exp, n_exp, what)
                        if streaming:
                            check_header(ctx, dense_streaming, what)
    finally:
        ctx.set_small_batch_ops(1 << 23)
        if dev:
            dev.free()


@pytest.mark.parametrize("family", TC.FAMILIES)
def test_every_case_in_every_setting(svx_ctx, primer, family):
    for c in TC.family(family):
        dense = len(TC.case_facts(c.name, "streaming").dense)
        run_everywhere(svx_ctx, primer, c.name, c.cigar, c.aln_off, c.ref_start, expected(c.name, True), expected(c.name, False), dense)


def test_table_is_what_the_cpu_module_checks():
    """(No case is left out of a family, skipped or expected to fail: the families partition the table.)"""
    assert sorted(c.name for f in TC.FAMILIES for c in TC.family(f)) == sorted(TC.CASES)
    TC.check_preconditions()


@functools.lru_cache(maxsize=1)
def _combined():
    b = TC.combined()
    exp = LC.restated_extract(b["cigar"], b["aln_off"], b["ref_start"], TC.MIN_LEN)
    dense = len(TC.facts(b["cigar"], b["aln_off"], "streaming").dense)
    assert dense == sum(len(TC.case_facts(n, "streaming").dense) for n in TC.CASES)   # the sum of the cases' counts
    return b, exp, dense


def test_combined_batch(svx_ctx, primer):
    b, exp, dense = _combined()
    run_everywhere(svx_ctx, primer, "combined", b["cigar"], b["aln_off"], b["ref_start"], exp, None, dense, ref_starts=(True,))


@pytest.mark.parametrize("chain", ["fused_chain", "split_chain"])
def test_combined_batch_in_one_submission_with_chimeric_reads(svx_ctx, primer, chain):
    """svx_collect_batch_dev (under svx_collect_batch): the table goes through k_tiles_a3 and k_finish_a3, the walk's
    instantiations that share a launch with the split-segment chain.  The chimeric reads are test_gpu_collect's: its
    random batch rides behind the table's, in a CIGAR pool of its own, on a tile boundary."""
    b, exp, dense = _combined()
    r = tcol.random_batch(np.random.default_rng(20261020), n_aln=40, n_parts=1, n_reads=12, long_aln=0.3, long_max=2500)
    n_table, n_aln_table = len(b["cigar"]), len(b["ref_start"])
    sub = dict(r, parts=[b["cigar"]] + r["parts"], aln_off=np.concatenate((b["aln_off"][:-1], r["aln_off"] + np.uint64(n_table))),
               ref_start=np.concatenate((b["ref_start"], r["ref_start"])), seg_src=r["seg_src"] + np.uint32(n_aln_table))
    cig = np.concatenate(sub["parts"])
    want = LC.restated_extract(cig, sub["aln_off"], sub["ref_start"], TC.MIN_LEN)
    for k in KEYS:   # the table's signatures come first and are the plain call's
        assert np.array_equal(want[k][:len(exp[k])], exp[k]), k
    n_dense = len(TC.facts(cig, sub["aln_off"], "streaming").dense)
    assert n_dense >= dense
    svx_ctx.set_split_chain(chain == "split_chain")
    try:
        for path in TC.PATHS:
            if path == "streaming":
                primer.before(n_dense)
            svx_ctx.set_small_batch_ops(0 if path == "streaming" else 1 << 23)
            sig, raw, post, first = tcol.call(svx_ctx.collect_batch, sub, TC.MIN_LEN)
            assert_same(sig, want, ("collect", path, chain))
            if path == "streaming":
                check_header(svx_ctx, n_dense, ("collect", chain))
            plain = svx_ctx.cigar_extract(cig, sub["aln_off"], sub["ref_start"], TC.MIN_LEN)
            assert_same(sig, plain, ("collect against the plain call", path, chain))
            assert len(raw) == len(r["seg_src"]) and len(first) == len(r["read_off"])
    finally:
        svx_ctx.set_split_chain(False)
        svx_ctx.set_small_batch_ops(1 << 23)


@pytest.mark.parametrize("name", TC.CAPACITY_CASES)
def test_capacity_protocol(svx_ctx, primer, name):
    """A staged tile, a dense one and the tile with records past the stage buffer, with room for all, all but one and
    half of the signatures: the full count comes back, exactly min(count, cap) rows are written, every byte behind them
    is intact — device entries — and the host entry reports SVX_E_CAPACITY with the full count."""
    c = TC.CASES[name]
    exp = expected(name, True)
    count = len(exp["aln"])
    dense = len(TC.case_facts(name, "streaming").dense)
    dev = Device(svx_ctx, c.cigar, c.aln_off, c.ref_start, count)
    try:
        for path in TC.PATHS:
            for soa in (False, True):
                for cap in (count, count - 1, count // 2):
                    what = (name, path, "soa" if soa else "packed", cap)
                    if path == "streaming":
                        primer.before(dense)
                    svx_ctx.set_small_batch_ops(0 if path == "streaming" else 1 << 23)
                    n, bufs = dev.call(soa, True, cap)
                    assert n == count, (what, n, count)
                    check_rows(bufs, exp, min(count, cap), what)
                    if path == "streaming":
                        check_header(svx_ctx, dense, what)
            for cap in (count, count - 1, count // 2):   # the host entry: rows + 8 sentinel rows behind the capacity
                bufs = [np.full(cap + 8, SENTINEL, np.uint8).repeat(np.dtype(dt).itemsize).view(dt) for dt in DTYPES]
                n = C.c_uint64(0)
                rc = svx_ctx.lib.svx_cigar_extract(svx_ctx.h, c.cigar.ctypes.data, c.aln_off.ctypes.data, len(c.aln_off) - 1,
                                                   c.ref_start.ctypes.data, TC.MIN_LEN, _lib.SigSoa(*[b.ctypes.data for b in bufs]),
                                                   cap, C.byref(n))
                assert rc == (0 if cap >= count else _lib.SVX_E_CAPACITY) and n.value == count, (name, path, cap, rc, n.value)
                check_rows(bufs, exp, min(count, cap), (name, path, "host", cap))
    finally:
        svx_ctx.set_small_batch_ops(1 << 23)
        dev.free()
