"""HIP CIGAR walk on batches with one alignment of 10^5 to 10^7 ops (tests/cigar_long_cases.py) — bit-exact against the
CPU oracle, which tests/test_cigar_long_pins.py holds against a numpy restatement on the same cases.

The cursors of an alignment that crosses tiles come out of segmented scans over tile descriptors, and at every level of
those scans one branch serves a unit without any alignment start: a DPP row, a wave and a whole workgroup of k_desc_scan
(with the last workgroup's scan of blk_agg behind it) on the streaming path, a thread's own eight descriptors, a row and
a wave of k_cigar_finish_small on the two-launch path.  Every case covers two such units of its level with one
alignment, reads the carry in a sparse tile behind each of them and in two tiles that take the dense re-walk; the
block-level ones move both cursors past 2^32 on the way.  The last part sends chimeric reads with primaries of that
length through svx_collect_batch: the chain's rows from CIGARs of 262 145 and 1 300 000 ops."""
import functools

import numpy as np
import pytest

from oracle import orc
from svim_asm_amd import _lib
from tests import cigar_long_cases as LC
from tests import helpers
from tests.test_gpu_collect import PARAMS, call, same_as_oracle

pytestmark = pytest.mark.gpu
KEYS = ("aln", "ref_pos", "read_pos", "len", "type")
SMALL_BATCH_DEFAULT = 1 << 23


def assert_same(got, exp, what):
    for k in KEYS:
        assert len(got[k]) == len(exp[k]), (what, k, len(got[k]), len(exp[k]))
        bad = np.nonzero(got[k] != exp[k])[0]
        assert len(bad) == 0, (what, k, len(bad), int(bad[0]), int(exp["aln"][bad[0]]), int(got[k][bad[0]]), int(exp[k][bad[0]]))


def half_capacity(ctx, b, exp):
    """svx_cigar_extract_dev with room for half the signatures: the full count comes back, exactly `cap` rows are
    written."""
    cig, off, rs = b["cigar"], b["aln_off"], b["ref_start"]
    n_exp = len(exp["aln"])
    cap = n_exp // 2
    assert cap > LC.DENSE_RUN  # the cut falls behind the first re-walked tile's rows
    d_cig, d_off, d_rs = ctx.dev_array(cig), ctx.dev_array(off), ctx.dev_array(rs)
    dtypes = (np.uint32, np.uint32, np.uint32, np.uint32, np.uint8)
    outs = [ctx.dev_array(np.full(cap + 64, 0xAB, dt)) for dt in dtypes]
    d_n = ctx.dev_array(np.zeros(1, np.uint64))
    rc = ctx.lib.svx_cigar_extract_dev(ctx.h, d_cig.ptr, len(cig), d_off.ptr, len(off) - 1, d_rs.ptr, LC.MIN_LEN,
                                       _lib.SigSoa(*[o.ptr for o in outs]), cap, d_n.ptr)
    assert rc == 0
    assert int(d_n.download(np.uint64)[0]) == n_exp
    for o, key, dt in zip(outs, KEYS, dtypes):
        got = o.download(dt)
        assert np.array_equal(got[:cap], exp[key][:cap]), key
        assert (got[cap:] == np.array(0xAB, dt)).all(), (key, "wrote past cap")


@pytest.mark.parametrize("name", list(LC.CASES))
def test_long_alignment_on_its_path(svx_ctx, name):
    case, b = LC.CASES[name], LC.build(name)
    f = LC.check_preconditions(name, b)
    cig, off, rs = b["cigar"], b["aln_off"], b["ref_start"]
    exp = orc.cigar_extract(cig, off, rs, LC.MIN_LEN)
    assert int((exp["aln"] == f["long"]).sum()) > 2 * LC.DENSE_RUN
    exp_stats = orc.cigar_stats(cig, off)
    svx_ctx.set_small_batch_ops(0 if case.path == "streaming" else SMALL_BATCH_DEFAULT)
    try:
        assert_same(svx_ctx.cigar_extract(cig, off, rs, LC.MIN_LEN), exp, "packed")
        op, ln = (cig & 15).astype(np.uint8), cig >> 4
        assert_same(svx_ctx.cigar_extract(ln, off, rs, LC.MIN_LEN, op=op), exp, "SoA")
        if name == LC.CAP_CASE:
            half_capacity(svx_ctx, b, exp)
        got = svx_ctx.cigar_stats(cig, off)
        for k in exp_stats:
            assert np.array_equal(got[k], exp_stats[k]), k
    finally:
        svx_ctx.set_small_batch_ops(SMALL_BATCH_DEFAULT)


# ------------------------------------------------------------------------------ chain rows on long primaries
PRIMARY_OPS = (262145, 1300000)
LEAD_CLIPS = (0, 130)   # 130: the chain's whole first chunk of 128 ops is clips
STAT_KEYS = ("ref_len", "q_start", "q_end", "read_len")
GAP = 45                # overlap on the read of a primary and the segment beside it: a deletion record of that length


def _words(*tuples):
    return np.array([(l << 4) | o for o, l in tuples], np.uint32)


def _rows_to_records(st, b):
    segs, read_len = orc.segment_rows(st, b["seg_src"], b["seg_tid"], b["seg_pos"], b["seg_rev"], b["seg_qend"], b["read_off"])
    return orc.segments_classify(segs, b["read_off"], read_len, PARAMS)


@functools.lru_cache(maxsize=1)
def chimeric_submission():
    """Chimeric reads on four primaries — 262 145 and 1 300 000 ops, each with no clip in front and with 130 — that lie
    between short records.  Every read is its primary and two SA-derived segments of 3 ops, and every primary has two
    reads whose segments are laid out from the ORACLE's statistics of the primary so that the adjacency records
    carry those statistics exactly (a segment 45 bases into the primary on the read and flush with it on the reference
    makes a deletion record of 45 bases at the primary's end of the reference):
      reverse read  filler, segment ending at read_len - q_end + 45 and starting at the primary's reference end, primary
      forward read  segment ending at q_start + 45 (filler where the next does not fit), primary, segment starting at
                    q_end - 45 (a leading S of up to 2^28 - 1 bases: the shorter primaries only)
    -> (batch, the oracle's answer)."""
    rng = np.random.default_rng(20261020)
    words, primaries = [], []
    for n in PRIMARY_OPS:
        for lead in LEAD_CLIPS:
            w = LC.random_ops(rng, n)
            w[:lead] = (w[:lead] & ~np.uint32(15)) | rng.choice(np.array([4, 5], np.uint32), size=lead)
            w[lead] = (w[lead] & ~np.uint32(15)) | np.uint32(0)
            words.append(LC.random_ops(rng, int(rng.integers(1, 3001))))
            primaries.append(len(words))
            words.append(w)
    words.append(LC.random_ops(rng, 2 * LC.STREAM_TILE + 1237))
    n_aln = len(words)
    cigar = np.concatenate(words)
    aln_off = np.concatenate(([0], np.cumsum([len(w) for w in words]))).astype(np.uint64)
    assert len(cigar) <= SMALL_BATCH_DEFAULT  # both CIGAR paths take it
    assert np.diff(aln_off.astype(np.int64))[primaries].tolist() == [n for n in PRIMARY_OPS for _ in LEAD_CLIPS]
    assert [int(np.argmax(~np.isin(words[a] & 15, (4, 5)))) for a in primaries] == list(LEAD_CLIPS) * len(PRIMARY_OPS)
    ref_start = rng.integers(1 << 26, 1 << 27, size=n_aln).astype(np.int32)
    st = {k: v.astype(np.int64) for k, v in orc.cigar_stats(cigar, aln_off).items()}
    extra, seg = [], []   # seg: (source, contig, position, reverse)
    counts = []

    def sa(w, tid, pos, rev):
        seg.append((n_aln + len(extra), tid, pos, rev))
        extra.append(w)

    filler = _words((0, 1), (4, 1), (4, 1))
    for a in primaries:
        ref_len, qs, qe, rl = (int(st[k][a]) for k in STAT_KEYS)
        pos = int(ref_start[a])
        assert 0 < ref_len and pos + ref_len + (1 << 28) < (1 << 31) and rl < (1 << 31)
        # reverse: the primary's row is (read_len - q_end, read_len - q_start); of S a, M m, S z it is (z, z + m)
        x = rl - qe
        assert GAP < x < (1 << 28) - GAP
        seg.append((a, 1, pos, 1))
        sa(filler, 2, 1000, 0)
        sa(_words((4, 7), (0, x + GAP - 2), (4, 2)), 1, pos + ref_len, 1)
        counts.append(3)
        # forward
        seg.append((a, 1, pos, 0))
        sa(_words((0, qs + GAP), (4, 1), (4, 1)), 1, pos - (qs + GAP), 0)
        if qe - GAP < 1 << 28:
            sa(_words((4, qe - GAP), (0, 500), (4, 3)), 1, pos + ref_len, 0)
        else:
            sa(filler, 2, 1000, 0)
        counts.append(3)
    assert sum(len(extra[i - n_aln]) == 3 and extra[i - n_aln][0] >> 4 > 1 << 27 for i, _, _, _ in seg if i >= n_aln) == 2
    b = dict(parts=[cigar], aln_off=aln_off, ref_start=ref_start, extra_cigar=np.concatenate(extra),
             extra_off=np.arange(0, 3 * len(extra) + 1, 3).astype(np.uint64), seg_src=np.array([t[0] for t in seg], np.uint32),
             seg_tid=np.array([t[1] for t in seg], np.int32), seg_pos=np.array([t[2] for t in seg], np.int32),
             seg_rev=np.array([t[3] for t in seg], np.uint8), seg_qend=np.full(len(seg), -1, np.int32),
             read_off=np.concatenate(([0], np.cumsum(counts))).astype(np.uint32), rank=np.array([2, 0, 3, 1], dtype=np.int32))
    exp = call(helpers.oracle_collect, b)
    # the records pin every statistic of every primary: one base more or less in any of them changes them
    st_all = orc.cigar_stats(np.concatenate((cigar, b["extra_cigar"])), np.concatenate((aln_off, len(cigar) + b["extra_off"][1:])))
    assert np.array_equal(_rows_to_records(st_all, b), exp[1])
    assert int((exp[1]["kind"] == 2).sum()) >= 2 * len(primaries) + 2   # (2: a deletion record)
    for a in primaries:
        for k in STAT_KEYS:
            for d in (-1, 1):
                if k == "q_start" and d == -1 and st_all[k][a] == 0:
                    continue
                off_by_one = {key: v.copy() for key, v in st_all.items()}
                off_by_one[k][a] = int(off_by_one[k][a]) + d
                assert not np.array_equal(_rows_to_records(off_by_one, b), exp[1]), (a, k, d)
    return b, exp


@pytest.mark.parametrize("split_chain", [False, True])
@pytest.mark.parametrize("streaming", [False, True])
def test_chain_rows_on_long_primaries(svx_ctx, streaming, split_chain):
    b, exp = chimeric_submission()
    assert len(exp[1]) == 24 and len(exp[0]["aln"]) > 1000
    svx_ctx.set_small_batch_ops(0 if streaming else SMALL_BATCH_DEFAULT)
    svx_ctx.set_split_chain(split_chain)
    try:
        same_as_oracle(call(svx_ctx.collect_batch, b), exp)
    finally:
        svx_ctx.set_split_chain(False)
        svx_ctx.set_small_batch_ops(SMALL_BATCH_DEFAULT)
