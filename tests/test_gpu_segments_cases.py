"""The device forms of the split-segment chain against the case table (tests/segments_cases.py) and the restatement
(tests/segments_restatement.py): svx_segments_classify(_dev), svx_segments_postpass(_dev) and the chain inside
svx_collect_batch(_dev), fused and split, on both CIGAR paths.  Every comparison is integer-exact, record for record.

Reference: analyze_read_segments (SVIM_inter.py:62-340).  tests/test_segments_restatement.py shows on the CPU that the
table reaches every comparison from both sides and that the restatement agrees with the pinned oracles."""
import ctypes as C
import functools

import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import helpers, segments_cases as SC, segments_restatement as R

pytestmark = pytest.mark.gpu
SET_NAMES = list(SC.PARAM_SETS)
SHAPES = ("pairs", "chains", "ties", "mirrored")
MI355X_CUS = 256  # what svx_ctx assumes too where the device does not say; k_segments launches at most n_cu * 8 workgroups


@functools.lru_cache(maxsize=None)
def table(name, shape, n_reads=0):
    """(reads, arrays, expected raw rows) of one shape under one parameter set, computed once."""
    cases = SC.tree_cases(SC.PARAM_SETS[name])
    reads = SC.packed(cases, n_reads) if shape == "packed" else getattr(SC, shape)(cases)
    return reads, SC.to_arrays(reads, _lib.SEG_DTYPE), SC.expected_raw(reads, SC.PARAM_SETS[name])


def rows8(a):
    return np.ascontiguousarray(a).view(np.int32).reshape(-1, 8)


def same_rows(got, exp, what):
    """All seven fields and pad == 0 (the expectation's pad column is 0)."""
    assert got.shape == exp.shape, what
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, (what, bad[:5].tolist(), got[bad[:3]].tolist(), exp[bad[:3]].tolist())


def classify_dev(ctx, segs, off, rl, prm):
    """svx_segments_classify_dev on buffers of the caller (svx_dev_malloc)."""
    n_segs, n_reads = len(segs), len(rl)
    d_segs, d_off, d_rl = ctx.dev_array(segs), ctx.dev_array(off), ctx.dev_array(rl)
    d_raw = ctx.dev_array(np.full(8 * n_segs, -1, np.int32))  # (the kernel writes every slot, pad included)
    p = _lib.SegParams(*prm)
    ctx._check(ctx.lib.svx_segments_classify_dev(ctx.h, d_segs.ptr, n_segs, d_off.ptr, n_reads, d_rl.ptr, C.byref(p), d_raw.ptr))
    ctx.sync()
    return d_raw.download(np.int32).reshape(-1, 8)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_classify_on_the_table(svx_ctx, name, shape):
    reads, (segs, off, rl), exp = table(name, shape)
    prm = SC.PARAM_SETS[name]
    same_rows(rows8(svx_ctx.segments_classify(segs, off, rl, prm)), exp, "host entry")
    same_rows(classify_dev(svx_ctx, segs, off, rl, prm), exp, "device entry")


@pytest.mark.parametrize("name", SET_NAMES)
def test_classify_packed_between_other_reads(svx_ctx, name):
    """The two-segment reads with reads of 0, 1, 3, 8 and 9 segments between them, at read counts around the eight reads
    of a wave and the 32 of a workgroup."""
    prm = SC.PARAM_SETS[name]
    for n in SC.PACKED_COUNTS:
        reads, (segs, off, rl), exp = table(name, "packed", n)
        same_rows(rows8(svx_ctx.segments_classify(segs, off, rl, prm)), exp, ("host entry", n))
        same_rows(classify_dev(svx_ctx, segs, off, rl, prm), exp, ("device entry", n))


def test_classify_second_trip_of_the_grid_stride_loop(svx_ctx):
    """More reads than n_cu * 8 workgroups of 32: the loop of k_segments goes round again."""
    n = getattr(svx_ctx, "n_cu", MI355X_CUS) * 8 * 32 + 9
    reads, (segs, off, rl), exp = table("DISTINCT", "packed", n)
    assert len(reads) == n
    same_rows(rows8(svx_ctx.segments_classify(segs, off, rl, SC.DISTINCT)), exp, "host entry")
    same_rows(classify_dev(svx_ctx, segs, off, rl, SC.DISTINCT), exp, "device entry")


# ------------------------------------------------------------------------------------------ post-passes
def raw_table(prm):
    cases = SC.postpass_cases(*prm)
    read_off = np.concatenate(([0], np.cumsum([len(raw) for _, raw in cases]))).astype(np.uint32)
    rows = [rec + (0,) for _, raw in cases for rec in raw]
    return cases, np.array(rows, np.int32).reshape(-1, 8).view(_lib.RAW_DTYPE).reshape(-1), read_off


def postpass_dev(ctx, raw, read_off, rank, prm):
    """svx_segments_postpass_dev on buffers of the caller; (packed records, first record per read)."""
    n_reads = len(read_off) - 1
    slots = np.diff(read_off.astype(np.int64))
    post_off = np.concatenate(([0], np.cumsum(slots * (slots + 3) // 2))).astype(np.uint64)
    d_raw, d_roff, d_rank, d_poff = ctx.dev_array(raw), ctx.dev_array(read_off), ctx.dev_array(rank), ctx.dev_array(post_off)
    d_post, d_cnt = ctx.dev_array(nbytes=32 * int(post_off[-1])), ctx.dev_array(nbytes=4 * n_reads)
    p = _lib.SegParams(*prm)
    ctx._check(ctx.lib.svx_segments_postpass_dev(ctx.h, d_raw.ptr, read_off.ctypes.data, d_roff.ptr, n_reads, d_rank.ptr,
                                                 len(rank), C.byref(p), d_post.ptr, post_off.ctypes.data, d_poff.ptr, d_cnt.ptr))
    ctx.sync()
    cnt = d_cnt.download(np.uint32)
    first = np.concatenate(([0], np.cumsum(cnt.astype(np.int64))))
    take = np.repeat(post_off[:-1].astype(np.int64) - first[:-1], cnt) + np.arange(int(first[-1]))
    return d_post.download(np.int32).reshape(-1, 8)[take].copy().view(_lib.RAW_DTYPE).reshape(-1), first


@pytest.mark.parametrize("prm", SC.POST_PARAMS)
def test_postpass_on_the_table(svx_ctx, prm):
    cases, raw, read_off = raw_table(prm)
    rank = np.array(SC.POST_RANK, np.int32)
    exp = [R.postpass_read(rows, SC.POST_RANK, *prm) for _, rows in cases]
    prm6 = prm + (50, 50, 50, 50)
    for what, (post, first) in (("host entry", svx_ctx.segments_postpass(raw, read_off, rank, prm6)),
                                ("device entry", postpass_dev(svx_ctx, raw, read_off, rank, prm6))):
        assert (rows8(post)[:, 7] == 0).all(), what
        got = helpers.post_records_as_tuples(post, first)  # per-read counts, records and order
        for (name, _), g, e in zip(cases, got, exp):
            assert g == e, (what, name)


# ------------------------------------------------------------------------------------------ the chain inside COLLECT
@functools.lru_cache(maxsize=None)
def submission(name):
    """The `chains`, `ties` and `mirrored` reads as the records of one submission: every segment a record
    `{lead}S{len}M{tail}S` at its position and strand, the first of a read a pool record, the others SA-derived."""
    prm = SC.PARAM_SETS[name]
    reads = table(name, "chains")[0] + table(name, "ties")[0] + table(name, "mirrored")[0]
    words, ref_start, extra, seg_src, seg_tid, seg_pos, seg_rev = [], [], [], [], [], [], []
    for rd in reads:
        for i, s in enumerate(rd["segs"]):
            w = helpers.segment_cigar(s.q_start, s.q_end, rd["read_len"], s.is_reverse)
            if i == 0:
                seg_src.append(len(words)); words.append(w); ref_start.append(s.ref_start)
            else:
                seg_src.append(-1 - len(extra)); extra.append(w)
            seg_tid.append(s.ref_id); seg_pos.append(s.ref_start); seg_rev.append(s.is_reverse)
    b = helpers.chimeric_batch(np.random.default_rng(5), words, ref_start, extra, seg_src, seg_tid, seg_pos, seg_rev,
                               [len(rd["segs"]) for rd in reads], n_unrelated=len(reads) // 2,
                               rank=np.array(SC.CONTIG_RANK, np.int32))
    raw = [R.classify_read(rd["segs"], rd["read_len"], prm) for rd in reads]
    post = [R.postpass_read(rows, SC.CONTIG_RANK, prm[0], prm[1]) for rows in raw]
    return b, SC.to_arrays(reads, _lib.SEG_DTYPE), SC.expected_raw(reads, prm), post


def collect_dev(ctx, b, prm):
    """svx_collect_batch_dev on resident buffers: (segment rows, read lengths, raw rows, packed post records, first)."""
    n_aln, n_ops = len(b["aln_off"]) - 1, int(b["aln_off"][-1])
    cigar = np.concatenate((b["parts"][0], b["extra_cigar"]))
    off = np.concatenate((b["aln_off"], n_ops + b["extra_off"][1:])).astype(np.uint64)
    n_segs, n_reads = len(b["seg_src"]), len(b["read_off"]) - 1
    slots = np.diff(b["read_off"].astype(np.int64))
    post_off = np.concatenate(([0], np.cumsum(slots * (slots + 3) // 2))).astype(np.uint64)
    d = {k: ctx.dev_array(v) for k, v in dict(cigar=cigar, off=off, rs=b["ref_start"], src=b["seg_src"], tid=b["seg_tid"],
                                               pos=b["seg_pos"], rev=b["seg_rev"], qend=b["seg_qend"], roff=b["read_off"],
                                               rank=b["rank"], poff=post_off).items()}
    cap = max(1024, n_ops)
    o = [ctx.dev_array(nbytes=4 * cap) for _ in range(4)] + [ctx.dev_array(nbytes=cap), ctx.dev_array(np.zeros(1, np.uint64))]
    d_segs, d_rl = ctx.dev_array(nbytes=24 * n_segs), ctx.dev_array(nbytes=4 * n_reads)
    d_raw, d_post, d_cnt = ctx.dev_array(nbytes=32 * n_segs), ctx.dev_array(nbytes=32 * int(post_off[-1])), ctx.dev_array(nbytes=4 * n_reads)
    dv = _lib.CollectDev(d_cigar=d["cigar"].ptr, n_ops=n_ops, d_aln_off=d["off"].ptr, n_aln=n_aln, n_extra=len(b["extra_off"]) - 1,
                         d_ref_start=d["rs"].ptr, min_len=40, d_seg_src=d["src"].ptr, d_seg_tid=d["tid"].ptr, d_seg_pos=d["pos"].ptr,
                         d_seg_rev=d["rev"].ptr, d_seg_qend=d["qend"].ptr, n_segs=n_segs, read_off=b["read_off"].ctypes.data,
                         d_read_off=d["roff"].ptr, n_reads=n_reads, d_contig_rank=d["rank"].ptr, n_contigs=len(b["rank"]),
                         params=_lib.SegParams(*prm), d_sig=_lib.SigSoa(*[x.ptr for x in o[:5]]), sig_cap=cap, d_n_sig=o[5].ptr,
                         d_segs=d_segs.ptr, d_read_len=d_rl.ptr, d_raw=d_raw.ptr, d_post=d_post.ptr, post_off=post_off.ctypes.data,
                         d_post_off=d["poff"].ptr, d_post_cnt=d_cnt.ptr)
    ctx._check(ctx.lib.svx_collect_batch_dev(ctx.h, C.byref(dv)))
    ctx.sync()
    cnt = d_cnt.download(np.uint32)
    first = np.concatenate(([0], np.cumsum(cnt.astype(np.int64))))
    take = np.repeat(post_off[:-1].astype(np.int64) - first[:-1], cnt) + np.arange(int(first[-1]))
    post = d_post.download(np.int32).reshape(-1, 8)[take].copy().view(_lib.RAW_DTYPE).reshape(-1)
    return d_segs.download(np.int32).reshape(-1, 6), d_rl.download(np.int32), d_raw.download(np.int32).reshape(-1, 8), post, first


@pytest.fixture(params=["fused_chain", "split_chain"])
def chain_form(request, svx_ctx):
    svx_ctx.set_split_chain(request.param == "split_chain")
    try:
        yield request.param
    finally:
        svx_ctx.set_split_chain(False)


@pytest.fixture(params=["small_batch", "streaming"])
def cigar_path(request, svx_ctx):
    svx_ctx.set_small_batch_ops(0 if request.param == "streaming" else 1 << 23)
    try:
        yield request.param
    finally:
        svx_ctx.set_small_batch_ops(1 << 23)


@pytest.mark.parametrize("name", ["DISTINCT", "DEFAULT"])
def test_chain_inside_collect_on_the_table(svx_ctx, chain_form, cigar_path, name):
    """Rows, raw records and derived records of the chain that rides inside the CIGAR launches, through the host entry
    and through svx_collect_batch_dev (which hands the six parameters on by another route)."""
    prm = SC.PARAM_SETS[name]
    b, (segs, off, rl), exp_raw, exp_post = submission(name)
    assert {t[0] for recs in exp_post for t in recs} == {"TANDEM", "DUP_INT", "INV"}
    sig, raw, post, first = svx_ctx.collect_batch(b["parts"], b["aln_off"], b["ref_start"], 40, b["extra_cigar"], b["extra_off"],
                                                  b["seg_src"], b["seg_tid"], b["seg_pos"], b["seg_rev"], b["seg_qend"],
                                                  b["read_off"], b["rank"], prm)
    same_rows(rows8(raw), exp_raw, "host entry")
    assert helpers.post_records_as_tuples(post, first) == exp_post
    d_segs, d_rl, d_raw, d_post, d_first = collect_dev(svx_ctx, b, prm)
    assert np.array_equal(d_segs, segs.view(np.int32).reshape(-1, 6))  # the rows are the intended segments
    assert np.array_equal(d_rl, rl)
    same_rows(d_raw, exp_raw, "device entry")
    assert helpers.post_records_as_tuples(d_post, d_first) == exp_post
