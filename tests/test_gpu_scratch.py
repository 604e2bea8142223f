"""Every device entry point of a context on POISONED scratch (DESIGN.md "Scratch contract", include/svx.h).

An entry point carves its scratch out of two long-lived HBM regions of the context (and svx_collect_batch out of a
page-locked host block); nothing outside the 4 KiB workspace header is ever cleared, so a call sees what the call
before it — any entry point, any size — left there.  The other GPU tests cannot see an array that is read before it is
written (the memory happens to hold zeros or the right leftovers) nor a result that is not written at all (they run
the same input twice).  Here every case goes through `poisoned`:

  1. the call once, so that the regions have their size and the poisoned calls land on the memory that was filled;
  2. for 0x00, 0xFF, 0xA5 in that order: svx_ctx_scratch_fill, the call again, the result against the ORACLE (never
     against the first call), the workspace header against the table of DESIGN.md.

Entry points that write into the caller's device buffers get those pre-filled with the same byte: exactly the
documented rows are written, the bytes behind them stay as they were.  The last tests run the real pattern — one
family's call on what another family's bigger call left, a workspace that grows — on fresh contexts, without the hook.
"""
import functools
import random
import zlib

import numpy as np
import pytest

from oracle import orc, svim_oracle
from svim_asm_amd import _lib, synth
from tests import callable_cases, cover_cases, helpers, lift_restatement, match_cases, mismatch_restatement
from tests import sam_text_writer as stw, tabix_reader
from tests import test_gpu_callable as tcall
from tests import test_gpu_collect as tcol
from tests import test_gpu_editdist as ted
from tests import test_gpu_cover as tcov
from tests import test_gpu_inflate as tinf
from tests import test_gpu_lift as tlift
from tests import test_gpu_mismatch as tmis
from tests import test_gpu_pair as tpair
from tests import test_gpu_sam as tsam
from tests import test_gpu_segments as tseg
from tests.test_oracle_pins import _scipy_cut

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0xA5)
PARAMS = (40, 100000, 50, 50, 50, 50)
KEYS = ("aln", "ref_pos", "read_pos", "len", "type")

# ---------------------------------------------------------------------------------------------------------------
# The workspace header, word by word, as DESIGN.md "Scratch contract" states it (words of 4 bytes):
#   0    dense-tile counter of the streaming CIGAR path        0 between calls
#   1    ticket of the streaming path's descriptor scan        0 between calls
#   2    dense-tile count the scan published                   that of the context's latest streaming call
#   64   arrival counter of the multi-workgroup sweep          0 between calls
#   65   its leavers' counter                                  0 between calls
#   68+2s, 69+2s (s = 0, 1)  the two arrival counters of k_pair_single, set s: launch k of the context uses set k & 1
#        and leaves both at its workgroup count (1 .. 64, at most one per 1024 keys); the launch after it zeroes them
#   80   note of a wait between workgroups that ran out        0 (the host clears the header when it finds the note)
#   every other word is never written: 0
# A workspace that had to grow starts from a zeroed header.
W_PUBLISHED, W_PAIR = 2, 68
TILE = 4096   # ops per tile of the streaming path
SLAB = 128    # signatures a tile stages; a tile with more is walked again by the dense-tile launch


class Watch:
    """A context with its header held to the table around every call."""

    def __init__(self, ctx, fresh=False):
        self.ctx = ctx
        h = ctx.scratch_header()
        live = [s for s in (0, 1) if h[W_PAIR + 2 * s] or h[W_PAIR + 2 * s + 1]]
        assert len(live) <= 1 and not (fresh and h.any()), h[W_PAIR:W_PAIR + 4]
        # the set the context's next k_pair_single launch uses: set 0 on a new context, else the other one than the
        # latest launch's (unknown while the header shows none: the workspace may have grown since)
        self.next_set = 0 if fresh else (live[0] ^ 1 if live else None)

    def call(self, fn, event=None):
        """fn() with the header read before and after.  event: None (the call owns no header word between calls),
        ("streaming", lo, hi): a CIGAR call on the streaming path with lo .. hi dense tiles, ("pair_single", n): one
        launch of k_pair_single over n keys."""
        before = self.ctx.scratch_header()
        out = fn()
        after = self.ctx.scratch_header()
        self.check(before, after, event)
        return out

    def check(self, before, after, event):
        quiet = np.ones(1024, bool)
        quiet[[W_PUBLISHED, W_PAIR, W_PAIR + 1, W_PAIR + 2, W_PAIR + 3]] = False
        assert not after[quiet].any(), ("header words that are zero between calls", np.nonzero(after * quiet)[0], after[quiet.nonzero()[0]])
        kind = event[0] if event else None

        def kept(words):  # as the call found them, or zero: a workspace that grew starts from a zeroed header
            return np.array_equal(after[words], before[words]) or not after[words].any()
        if kind == "streaming":
            assert event[1] <= int(after[W_PUBLISHED]) <= event[2], (int(after[W_PUBLISHED]), event)
        else:
            assert kept([W_PUBLISHED]), (before[W_PUBLISHED], after[W_PUBLISHED])
        sets = [tuple(int(x) for x in after[W_PAIR + 2 * s:W_PAIR + 2 * s + 2]) for s in (0, 1)]
        if kind == "pair_single":
            n = event[1]
            live = [s for s in (0, 1) if sets[s] != (0, 0)]
            assert len(live) == 1, sets                                   # the launch cleaned the other set
            g = sets[live[0]][0]
            assert sets[live[0]] == (g, g) and 1 <= g <= min(64, (n + 1023) // 1024), (sets, n)
            if self.next_set is not None:
                assert live[0] == self.next_set, (sets, self.next_set)    # alternate launches, alternate sets
            self.next_set = live[0] ^ 1
        else:
            assert kept(list(range(W_PAIR, W_PAIR + 4))), (before[W_PAIR:W_PAIR + 4], sets)


def poisoned(ctx, run, check, event=None):
    """The helper every case goes through (module docstring).  run(byte) makes the call — byte: what the scratch was
    filled with (None on the sizing call), for the caller-owned device buffers —, check(result, byte) holds the result
    to the oracle."""
    w = ctx if isinstance(ctx, Watch) else Watch(ctx)
    w.call(lambda: run(None), event)
    for byte in FILLS:
        before = w.ctx.scratch_header()
        w.ctx.scratch_fill(byte)
        assert np.array_equal(w.ctx.scratch_header(), before), "svx_ctx_scratch_fill touched the header"
        check(w.call(lambda: run(byte), event), byte)


# ------------------------------------------------------------------------------------------------------- CIGAR
def _dense_bounds(cigar, n_ops, min_len):
    """Tiles of the streaming path that MUST be walked again (more signatures than a slab holds) and tiles that MAY be
    (a round that overflowed its queue also sends its tile there; a tile without a signature never goes)."""
    c = np.asarray(cigar[:n_ops], np.uint32)
    emits = np.isin(c & 15, (1, 2)) & ((c >> 4) >= min_len)
    per_tile = np.add.reduceat(emits.astype(np.int64), np.arange(0, n_ops, TILE)) if n_ops else np.zeros(0, np.int64)
    return int((per_tile > SLAB).sum()), int((per_tile > 0).sum()), int(emits.sum())


@functools.lru_cache(maxsize=None)
def _cigar_batches():
    rng = np.random.default_rng(7)  # the batches of test_dense_all_indel_tiles_take_the_direct_path
    cig, off, rs = synth.random_cigar_case(rng, 37, max_ops=3000, dense=True)
    c2, o2, r2 = synth.random_cigar_case(rng, 50, max_ops=5000)
    mixed = (np.concatenate([c2, cig, c2]),
             np.concatenate([o2, o2[-1] + off[1:], o2[-1] + off[-1] + o2[1:]]).astype(np.uint64), np.concatenate([r2, rs, r2]))
    # alignments of 1, 1025 and 4097 ops, the two long ones cut again at their ops 15, 16 and 17
    n = 1 + 1025 + 4097
    rng = np.random.default_rng(n)
    cuts = np.array([0, 1, 16, 17, 18, 1026, 1041, 1042, 1043, n], np.uint64)
    edges = (((rng.integers(30, 60, n) << 4) | rng.integers(0, 3, n)).astype(np.uint32), cuts,
             (np.arange(len(cuts) - 1) * 1000).astype(np.int32))
    out = {}
    for name, (c, o, r) in (("mixed_dense", mixed), ("edges", edges)):
        out[name] = (c, o, r, orc.cigar_extract(c, o, r, 40))
    return out


@pytest.mark.parametrize("batch", ["mixed_dense", "edges"])
@pytest.mark.parametrize("soa", [False, True], ids=["packed", "soa"])
@pytest.mark.parametrize("path", ["two_launch", "streaming"])
def test_cigar_extract(svx_ctx, path, soa, batch):
    cig, off, rs, exp = _cigar_batches()[batch]
    lo, hi, n_sig = _dense_bounds(cig, len(cig), 40)
    assert n_sig == len(exp["aln"]) and (batch != "mixed_dense" or lo > 0)
    op, ln = (cig & 15).astype(np.uint8), (cig >> 4).astype(np.uint32)

    def run(_):
        return svx_ctx.cigar_extract(ln, off, rs, 40, op=op) if soa else svx_ctx.cigar_extract(cig, off, rs, 40)

    def check(got, _):
        for k in KEYS:
            assert np.array_equal(got[k], exp[k]), k
    svx_ctx.set_small_batch_ops(0 if path == "streaming" else 1 << 23)
    try:
        poisoned(svx_ctx, run, check, ("streaming", lo, hi) if path == "streaming" else None)
    finally:
        svx_ctx.set_small_batch_ops(1 << 23)


def test_cigar_stats(svx_ctx):
    rng = np.random.default_rng(9)
    cig, off, _ = synth.random_cigar_case(rng, 300, max_ops=700)
    off = np.concatenate((off, off[-1:])).astype(np.uint64)  # ... and one alignment without ops behind them
    exp = orc.cigar_stats(cig, off)

    def check(got, _):
        for k in exp:
            assert np.array_equal(got[k], exp[k]), k
    poisoned(svx_ctx, lambda _: svx_ctx.cigar_stats(cig, off), check)


# ---------------------------------------------------------------------------------- segments and their post-passes
def test_segments_classify(svx_ctx):
    """Reads of 0 .. 40 segments: up to eight are ranked in registers, more are sorted in the HBM scratch slice."""
    rng = np.random.default_rng(40)
    segs, off, rl = tseg.random_reads(rng, 612, 40)
    off = np.concatenate((off, off[-1:])).astype(np.uint32)  # one empty read behind them
    rl = np.concatenate((rl, [1000])).astype(np.int32)
    assert (np.diff(off.astype(np.int64)) > 8).any() and (np.diff(off.astype(np.int64)) == 0).any()
    exp = orc.segments_classify(segs, off, rl, PARAMS)
    poisoned(svx_ctx, lambda _: svx_ctx.segments_classify(segs, off, rl, PARAMS),
             lambda got, _: np.testing.assert_array_equal(got.view(np.int32), exp.view(np.int32)))


def test_segments_postpass(svx_ctx):
    """The 600 + 12 reads of test_postpass_matches_record_level_oracle and one empty read: the 12 reads of 12-40 slots
    have inversion groups of more than 10 members, whose linkage state lives in the read's HBM scratch slice."""
    rng = np.random.default_rng(40)
    n_contigs = 12
    names = ["chr%d" % (i + 1) for i in range(n_contigs)]
    rank = np.zeros(n_contigs, np.int32)
    for k, i in enumerate(sorted(range(n_contigs), key=lambda i: names[i])):
        rank[i] = k
    reads = [tseg._random_raw_read(rng, int(rng.integers(0, 9)), n_contigs, bool(rng.random() < 0.7)) for _ in range(600)]
    reads += [tseg._random_raw_read(rng, int(rng.integers(12, 40)), n_contigs, True) for _ in range(12)]
    reads.append([])
    read_off = np.concatenate(([0], np.cumsum([len(r) for r in reads]))).astype(np.uint32)
    raw = np.zeros(int(read_off[-1]), dtype=_lib.RAW_DTYPE)
    k = 0
    for r in reads:
        for row in r:
            for name_, v in zip(("kind", "a0", "a1", "a2", "a3", "a4", "a5"), row):
                raw[k][name_] = v
            k += 1
    exp = [svim_oracle.postpass_records(r, rank.tolist(), PARAMS[0], PARAMS[1]) for r in reads]
    assert any(t[0] == "INV" and t[-1] for recs in exp for t in recs)

    def check(got, _):
        assert helpers.post_records_as_tuples(*got) == exp
    poisoned(svx_ctx, lambda _: svx_ctx.segments_postpass(raw, read_off, rank, PARAMS), check)


# -------------------------------------------------------------------------------------------------------- pair
@functools.lru_cache(maxsize=None)
def _pair_case(n, max_dist):
    keys = tpair.make_keys(np.random.default_rng(n), n, 6 * 24, 250_000_000)
    return keys, orc.pair_partition(keys, max_dist)


def _set_pair_plan(ctx, plan):
    ctx.set_pair_single_launch_max(0 if plan == "radix" else 131072)
    ctx.set_pair_wait_free(plan == "wait_free")


def _check_pair(exp):
    def check(got, _):
        assert got[2] == exp[2] and np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    return check


@pytest.mark.parametrize("max_dist", [0, 1000])
@pytest.mark.parametrize("n", [1000, 20000, 70001])  # 20 000: the multi-workgroup sweep of the radix plans (above 16 384)
@pytest.mark.parametrize("plan", ["single_launch", "radix", "wait_free"])
def test_pair_partition(svx_ctx, plan, n, max_dist):
    keys, exp = _pair_case(n, max_dist)
    _set_pair_plan(svx_ctx, plan)
    try:
        poisoned(svx_ctx, lambda _: svx_ctx.pair_partition(keys, max_dist), _check_pair(exp),
                 ("pair_single", n) if plan == "single_launch" else None)
    finally:
        _set_pair_plan(svx_ctx, "single_launch")


@pytest.mark.parametrize("first_set", [0, 1])
def test_pair_counter_sets_in_both_roles(svx_ctx, first_set):
    """The poisoned launches started on either set, i.e. behind an odd and behind an even number of k_pair_single
    launches of the context: each of the two counter sets is the launch's own (left at the workgroup count) and the
    stale one (zeroed by the launch) under every fill."""
    w = Watch(svx_ctx)
    keys, exp = _pair_case(20000, 1000)
    _set_pair_plan(svx_ctx, "single_launch")
    for _ in range(2):  # (one launch tells which set is next when the header does not, one more changes it)
        if w.next_set != first_set:
            _check_pair(exp)(w.call(lambda: svx_ctx.pair_partition(keys, 1000), ("pair_single", len(keys))), None)
    assert w.next_set == first_set
    poisoned(w, lambda _: svx_ctx.pair_partition(keys, 1000), _check_pair(exp), ("pair_single", len(keys)))
    assert w.next_set == first_set  # four launches later: the same set is next


# ------------------------------------------------------------------------------------- edit distance, haplotypes
@functools.lru_cache(maxsize=None)
def _edit_case():
    rng = np.random.default_rng(0)
    pairs = list(ted.make_pairs(rng, 200, 700, 60)[0])
    base = ted._rand_dna(rng, 21000)  # six strips of 4096 rows: the boundary `stream` words; ~3 % apart: the band widens
    pairs.append((base, ted._edited(rng, base, 600, 20, 30)))
    alpha = rng.permutation(256).astype(np.uint8)  # all 256 byte values: the second instantiation of the kernel
    a = alpha[rng.integers(0, 256, 700)].tobytes()
    b = bytearray(a)
    for _ in range(35):
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
    del b[233:240]
    pairs.append((a, bytes(b)))
    exp = np.array([orc.edit_distance(x, y) if max(len(x), len(y)) <= 10000 else orc.edit_distance_banded(x, y) for x, y in pairs],
                   dtype=np.int64)
    assert exp[-2] > 256 and len(set(pairs[-1][0])) > 16
    return ted._pool(pairs), exp


@pytest.mark.parametrize("k_max", [0, 200, 0xFFFFFFFF], ids=["k0", "k200", "exact"])
@pytest.mark.parametrize("cap", [1024, 48, 0], ids=["wavefront_1024", "wavefront_48", "bitvector_only"])
def test_edit_distance_batch(svx_ctx, cap, k_max):
    (pool, ao, al, bo, bl), exp = _edit_case()
    want = np.where(exp <= k_max, exp, 0xFFFFFFFF)
    svx_ctx.set_edit_wavefront_cap(cap)
    try:
        poisoned(svx_ctx, lambda _: svx_ctx.edit_distance_batch(pool, ao, al, bo, bl, k_max),
                 lambda got, _: np.testing.assert_array_equal(got.astype(np.int64), want))
    finally:
        svx_ctx.set_edit_wavefront_cap(1024)


@functools.lru_cache(maxsize=None)
def _haplotype_case():
    """50 pairs built as in test_haplotype_distance_batch_assembles_like_the_reference."""
    rng = np.random.default_rng(12)
    pool = np.frombuffer("".join(rng.choice(list("ACGTacgtNnRy"), size=60000)).encode(), dtype=np.uint8)
    n_pairs = 50
    pieces = np.zeros(n_pairs * 6, dtype=_lib.HAP_PIECE_DTYPE)
    for k in range(n_pairs * 6):
        if k % 3 == 1:  # middle: absent, reverse complement, repeated, or as it is
            mode = int(rng.integers(0, 4))
            ln = int(rng.integers(0, 900)) if mode else 0
            rep = [0, 1, int(rng.integers(1, 5)), 1][mode]
            flags = [0, 3, 1, 0][mode]
        else:
            ln, rep, flags = int(rng.integers(0, 300)), 1, 1
        if ln == 0 or rep == 0:
            ln = rep = flags = 0
        pieces[k] = (int(rng.integers(0, len(pool) - 1000)) if ln else 0, ln, rep, flags)
    exp = []
    for p in range(n_pairs):
        a = ted._assemble(pool, pieces[p * 6:p * 6 + 3].tolist())
        b = ted._assemble(pool, pieces[p * 6 + 3:p * 6 + 6].tolist())
        exp.append(orc.edit_distance(a.encode("latin-1"), b.encode("latin-1")))
    per_pair = rng.choice(np.array([0xFFFFFFFF, 200, 0, 37, 1 << 31], dtype=np.uint32), size=n_pairs)
    return pool, pieces, np.array(exp, np.int64), per_pair


@pytest.mark.parametrize("k_max", [200, 0xFFFFFFFF], ids=["k200", "exact"])
def test_haplotype_distance_batch(svx_ctx, k_max):
    pool, pieces, exp, _ = _haplotype_case()
    want = np.where(exp <= k_max, exp, 0xFFFFFFFF)
    poisoned(svx_ctx, lambda _: svx_ctx.haplotype_distance_batch(pool, pieces, k_max),
             lambda got, _: np.testing.assert_array_equal(got.astype(np.int64), want))


def test_haplotype_distance_batch_mixed(svx_ctx):
    pool, pieces, exp, per_pair = _haplotype_case()
    want = np.where(exp <= per_pair.astype(np.int64), exp, 0xFFFFFFFF)
    poisoned(svx_ctx, lambda _: svx_ctx.haplotype_distance_batch_mixed(pool, pieces, per_pair),
             lambda got, _: np.testing.assert_array_equal(got.astype(np.int64), want))


# ----------------------------------------------------------------------------------------------------- linkage
@functools.lru_cache(maxsize=None)
def _linkage_case(sizes, cutoff):
    rng = np.random.default_rng(sum(sizes))
    conds = [np.round(rng.random(n * (n - 1) // 2) * 6) / 2 for n in sizes]  # 0, 0.5 .. 3: ties everywhere
    exp = [l for n, c in zip(sizes, conds) for l in ([1] if n == 1 else [int(x) for x in _scipy_cut(c, cutoff)])]
    return np.concatenate(conds), np.array(sizes, np.uint32), exp


LINKAGE = {"lanes": ((1, 2, 10, 11, 25), _lib.LINKAGE_LANES_ONLY),   # up to 10: a lane's LDS slice; 11 and 25: its HBM slice
           # ... and the workgroup kernel for 17 and 65 (matrix in LDS) and for the first size whose matrix is in scratch
           "lanes_and_groups": ((1, 2, 10, 11, 17, 65, _lib.LINKAGE_GROUP_LDS_N + 1), 17)}


def _check_labels(exp):
    def check(got, _):
        assert got.tolist() == exp, "labels differ from scipy's"
    return check


@pytest.mark.parametrize("cutoff", [0.3, 2.5])
@pytest.mark.parametrize("case", list(LINKAGE))
def test_linkage_cut_batch(svx_ctx, case, cutoff):
    sizes, group_min = LINKAGE[case]
    dist, counts, exp = _linkage_case(sizes, cutoff)
    svx_ctx.set_linkage_group_min(group_min)
    try:
        poisoned(svx_ctx, lambda _: svx_ctx.linkage_cut_batch(dist, counts, cutoff), _check_labels(exp))
    finally:
        svx_ctx.set_linkage_group_min(0)


# ------------------------------------------------------------------------------------------ match, cover, lift, mismatch
def test_match_greedy_batch(svx_ctx):
    """Under the default threshold of nine pairs: 2 x 4 stays with the lane kernel, 33 x 65 goes to the group kernel."""
    dist, n_base, n_comp, want_base, want_comp = match_cases.batch([("ties", 2, 4), ("wide", 33, 65)])
    assert want_base.count(_lib.MATCH_NONE) < len(want_base)

    def check(got, _):
        assert got[0].tolist() == want_base and got[1].tolist() == want_comp
    svx_ctx.set_match_group_min(0)
    poisoned(svx_ctx, lambda _: svx_ctx.match_greedy_batch(dist, n_base, n_comp), check)


@functools.lru_cache(maxsize=None)
def _cover_case():
    """1025 lists — tests/callable_cases.many_lists: one more than a pass of the offsets kernel of svx_cover_single takes —,
    list 7 replaced by one of 1025 entries, one more than a pass of the scans takes: both carry once."""
    rng = random.Random(1025)
    n = cover_cases.CHUNK + 1
    lists = list(callable_cases.many_lists(n))
    lists[7] = [(s, e) for s, e in cover_cases.random_list(rng, n, contigs=(0,), contig_len=20000) if s < e]
    while len(lists[7]) < n:  # (svx_cover_single takes no empty interval)
        lists[7] = sorted(lists[7] + [(lists[7][0][0], lists[7][0][1] + len(lists[7]))])
    queries = cover_cases.random_queries(rng, 65, contigs=(0,), contig_len=20000, longest=200)
    callable_cases.check_inputs(lists)
    cover_cases.check_inputs(lists, queries)
    assert len(lists) == n and len(lists[7]) == n
    where = lift_restatement.locate(lists, queries)
    bits = [[int(i != lift_restatement.NONE) for i in row] for row in where]
    assert bits == cover_cases.R.cover(lists, queries) and 0 < sum(bits[7]) < len(queries) and any(any(r) for r in bits[8:])
    return lists, queries, bits, where, callable_cases.R.flat(callable_cases.R.single(lists))


def test_cover_query(svx_ctx):
    lists, queries, bits, _, _ = _cover_case()
    poisoned(svx_ctx, lambda _: svx_ctx.cover_query(*tcov.arrays(lists, queries)),
             lambda got, _: np.testing.assert_array_equal(got, np.array(bits, np.uint8)))


def test_cover_locate(svx_ctx):
    lists, queries, _, where, _ = _cover_case()
    poisoned(svx_ctx, lambda _: svx_ctx.cover_locate(*tcov.arrays(lists, queries)),
             lambda got, _: np.testing.assert_array_equal(got, np.array(where, np.uint32)))


def test_cover_single(svx_ctx):
    lists, _, _, _, segments = _cover_case()
    assert 0 < len(segments[0]) < sum(len(ivs) for ivs in lists)

    def check(got, _):
        assert tuple(x.tolist() for x in got) == tuple(segments)
    poisoned(svx_ctx, lambda _: svx_ctx.cover_single(*tcall.arrays(lists)), check)


@functools.lru_cache(maxsize=None)
def _lift_case():
    """Two alignments of 700 ops: the pool spans two chunks of the prefix scan, the second alignment lies across their border."""
    rng = random.Random(700)
    inputs = tlift.with_queries(rng, [(rng.randrange(0, 5000), tlift.random_ops(rng, 700)) for _ in range(2)])
    assert _lib.LIFT_CHUNK < len(inputs[0]) <= 2 * _lib.LIFT_CHUNK and int(inputs[1][1]) < _lib.LIFT_CHUNK
    query, state = lift_restatement.lift_batch(*inputs)
    assert {lift_restatement.OUTSIDE, lift_restatement.ALIGNED, lift_restatement.DELETED, lift_restatement.END} <= set(state)
    return inputs, query, state


def _with_pool_in_hbm(ctx, words, call):
    """call(pointer, n_ops) on the pool in HBM, words behind the alignments' last one included."""
    pool = ctx.dev_array(np.concatenate((words, np.full(7, (9 << 4) | 0, np.uint32))))
    try:
        return call(pool.ptr, len(words) + 7)
    finally:
        pool.free()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_cigar_lift(svx_ctx, form):
    inputs, query, state = _lift_case()

    def run(_):
        if form == "host":
            return svx_ctx.cigar_lift(*inputs)
        return _with_pool_in_hbm(svx_ctx, inputs[0], lambda ptr, n: svx_ctx.cigar_lift(ptr, *inputs[1:], n_ops=n))

    def check(got, _):
        assert got[1].tolist() == state and got[0].tolist() == query
    poisoned(svx_ctx, run, check)


@functools.lru_cache(maxsize=None)
def _mismatch_case():
    """Two alignments, of 1025 and 300 ops: two chunks of the prefix scan, and the first one's window is more than a tile."""
    inputs = tmis.pool_of((1025, 300), 1325)
    assert _lib.LIFT_CHUNK < len(inputs[0]) <= 2 * _lib.LIFT_CHUNK and tmis.T < int(inputs[5][0]) and int(inputs[5][1]) > 0
    expected = mismatch_restatement.mismatch_batch(*inputs)
    assert set(expected["aln"]) == {0, 1} and max(p - int(inputs[2][0]) for p, a in zip(expected["ref_pos"], expected["aln"]) if a == 0) >= tmis.T
    return inputs, expected


@pytest.mark.parametrize("form", ["host", "dev"])
def test_cigar_mismatch(svx_ctx, form):
    inputs, expected = _mismatch_case()

    def run(_):
        if form == "host":
            return svx_ctx.cigar_mismatch(*inputs)
        return _with_pool_in_hbm(svx_ctx, inputs[0], lambda ptr, n: svx_ctx.cigar_mismatch(ptr, *inputs[1:], n_ops=n))

    def check(got, _):
        for k in tmis.COLS:
            assert got[k].tolist() == expected[k], k
    poisoned(svx_ctx, run, check)


# ----------------------------------------------------------------------------------------------------- collect
@functools.lru_cache(maxsize=None)
def _collect_case(name):
    if name == "random":
        b = tcol.random_batch(np.random.default_rng(100), n_aln=300, n_parts=2, n_reads=60, long_read=True, long_aln=0.3, long_max=3000)
    else:  # reads whose segments tile the read: the post-passes emit derived records
        b = tcol.tiling_batch(np.random.default_rng(901), n_reads=50)
    exp = tcol.call(helpers.oracle_collect, b)
    if name == "tiling":
        assert {"TANDEM", "INV", "DUP_INT"} <= {t[0] for recs in exp[2] for t in recs}
    return b, exp


@pytest.mark.parametrize("batch", ["random", "tiling"])
@pytest.mark.parametrize("path", ["two_launch", "streaming"])
@pytest.mark.parametrize("chain", ["fused_chain", "split_chain"])
def test_collect_batch(svx_ctx, chain, path, batch):
    b, exp = _collect_case(batch)
    n_ops = int(b["aln_off"][-1])
    lo, hi, n_sig = _dense_bounds(np.concatenate(b["parts"]), n_ops, 40)
    assert n_sig == len(exp[0]["aln"])
    svx_ctx.set_split_chain(chain == "split_chain")
    svx_ctx.set_small_batch_ops(0 if path == "streaming" else 1 << 23)
    try:
        poisoned(svx_ctx, lambda _: tcol.call(svx_ctx.collect_batch, b), lambda got, _: tcol.same_as_oracle(got, exp),
                 ("streaming", lo, hi) if path == "streaming" else None)
    finally:
        svx_ctx.set_split_chain(False)
        svx_ctx.set_small_batch_ops(1 << 23)


# -------------------------------------------------------------------------------------------------- CIGAR text
GUARD = 64  # bytes behind every caller-owned output that no call may touch


def _filled(ctx, nbytes, byte):
    return ctx.dev_array(np.full(nbytes + GUARD, 0x5A if byte is None else byte, np.uint8))


def cigar_text_parse_dev(ctx, texts, byte):
    """svx_cigar_text_parse_dev on output buffers pre-filled with `byte`: dict(words, cigar_off, ref_len, status) and,
    under "untouched", whether every byte behind the documented rows is still the fill."""
    fill = 0x5A if byte is None else byte
    text, off = tsam._batch(texts)
    text = np.frombuffer(text, np.uint8)
    n, cap = len(off) - 1, len(text) // 2 + 1
    d_text, d_off = ctx.dev_array(np.concatenate((text, np.zeros(1, np.uint8)))), ctx.dev_array(off)
    d_words, d_coff = _filled(ctx, 4 * cap, byte), _filled(ctx, 8 * (n + 1), byte)
    d_rl, d_st = _filled(ctx, 4 * n, byte), _filled(ctx, 4 * n, byte)
    ctx._check(ctx.lib.svx_cigar_text_parse_dev(ctx.h, d_text.ptr, len(text), d_off.ptr, n, d_words.ptr, cap, d_coff.ptr, d_rl.ptr, d_st.ptr))
    ctx.sync()
    raw = {k: d.download(np.uint8) for k, d in (("words", d_words), ("cigar_off", d_coff), ("ref_len", d_rl), ("status", d_st))}
    for d in (d_text, d_off, d_words, d_coff, d_rl, d_st):
        d.free()
    coff = raw["cigar_off"][:8 * (n + 1)].view(np.uint64)
    total = int(coff[-1])
    assert total <= cap
    out = {"cigar_off": coff, "words": raw["words"][:4 * total].view(np.uint32), "ref_len": raw["ref_len"][:4 * n].view(np.int32),
           "status": raw["status"][:4 * n].view(np.uint32)}
    out["untouched"] = bool((raw["words"][4 * total:] == fill).all() and (raw["cigar_off"][8 * (n + 1):] == fill).all() and
                            (raw["ref_len"][4 * n:] == fill).all() and (raw["status"][4 * n:] == fill).all())
    return out


def _three_chunks():
    """2 500 bytes of records (three chunks of 1024 bytes), one bad record in the middle chunk."""
    rng = np.random.default_rng(6)
    texts, size = [], 0
    while size < 2500:
        if 1400 <= size and "12Q3M" not in texts:
            texts.append("12Q3M")
        else:
            texts.append("".join("%d%s" % (int(rng.integers(1, 5000)), "MIDNSHP=X"[int(rng.integers(0, 9))]) for _ in range(int(rng.integers(1, 6)))))
        size += len(texts[-1])
    at = sum(len(t) for t in texts[:texts.index("12Q3M")])
    assert 1024 <= at and at + 5 <= 2048 and 2048 < size < 3072
    return texts


CIGAR_TEXTS = {"every_form": tsam.GOOD + tsam.BAD, "three_chunks": _three_chunks()}


def check_cigar_text(texts, got, what=""):
    exp = stw.parse_batch(texts)
    for k in ("status", "cigar_off", "ref_len", "words"):
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), np.asarray(exp[k], dtype=np.int64)), (what, k)
    assert got["untouched"], (what, "bytes behind the documented rows were written")


@pytest.mark.parametrize("case", list(CIGAR_TEXTS))
def test_cigar_text_parse(svx_ctx, case):
    texts = CIGAR_TEXTS[case]
    assert any(stw.parse_cigar(t)[0] for t in texts) and not all(stw.parse_cigar(t)[0] for t in texts)
    poisoned(svx_ctx, lambda byte: cigar_text_parse_dev(svx_ctx, texts, byte),
             lambda got, byte: check_cigar_text(texts, got, "fill %#x" % byte))


# -------------------------------------------------------------------------------------------------------- BGZF
BAD_CRC = 8


@functools.lru_cache(maxsize=None)
def _members():
    """17 members of every kind of data, level and strategy; member BAD_CRC carries a wrong CRC32."""
    rng = np.random.default_rng(1)
    data = list(tinf.kinds(rng).values())
    plans = [(6, zlib.Z_DEFAULT_STRATEGY, 8), (1, zlib.Z_DEFAULT_STRATEGY, 8), (9, zlib.Z_HUFFMAN_ONLY, 9), (6, zlib.Z_RLE, 9),
             (4, zlib.Z_FILTERED, 1), (6, zlib.Z_FIXED, 8), (0, zlib.Z_DEFAULT_STRATEGY, 8)]
    expect = [data[k % len(data)][:65536] for k in range(17)]
    payloads = [tinf.deflate(d, *plans[(k // 2) % len(plans)]) for k, d in enumerate(expect)]
    crc = [zlib.crc32(d) & 0xFFFFFFFF for d in expect]
    crc[BAD_CRC] ^= 0x00010000
    return payloads, expect, crc


def bgzf_inflate_dev(ctx, payloads, isize, crc, byte):
    """svx_bgzf_inflate_dev with the output and the statuses pre-filled: (status, output bytes, output offsets)."""
    n = len(payloads)
    in_len = np.array([len(p) for p in payloads], np.uint32)
    in_off = np.zeros(n, np.uint64)
    np.cumsum(((in_len[:-1].astype(np.uint64) + 3) // 4) * 4, out=in_off[1:])
    blob = np.zeros(int(in_off[-1] + in_len[-1]) + 8, np.uint8)
    for p, o, l in zip(payloads, in_off.tolist(), in_len.tolist()):
        blob[o:o + l] = np.frombuffer(p, np.uint8)
    isize = np.asarray(isize, np.uint32)
    out_off = np.zeros(n, np.uint64)
    np.cumsum(((isize[:-1].astype(np.uint64) + 32 + 15) // 16) * 16, out=out_off[1:])  # 32 bytes and more between members
    total = int(out_off[-1] + isize[-1])
    d = [ctx.dev_array(x) for x in (blob, in_off, in_len, isize, np.asarray(crc, np.uint32), out_off)]
    d_out, d_st = _filled(ctx, total, byte), _filled(ctx, 4 * n, byte)
    ctx._check(ctx.lib.svx_bgzf_inflate_dev(ctx.h, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, n, d_out.ptr, d[5].ptr, d_st.ptr))
    ctx.sync()
    out, st = d_out.download(np.uint8), d_st.download(np.uint8)
    for x in d + [d_out, d_st]:
        x.free()
    return st, out, out_off


@pytest.mark.parametrize("form", list(tinf.FORMS))
def test_bgzf_inflate(svx_ctx, form):
    payloads, expect, crc = _members()
    n = len(payloads)
    isize = [len(e) for e in expect]
    assert n == 17 and {len(e) for e in expect} >= {0, 1, 65536} and len(expect[BAD_CRC]) > 1000

    def check(got, byte):
        st, out, out_off = got
        assert st[:4 * n].view(np.uint32).tolist() == [3 if m == BAD_CRC else 0 for m in range(n)]  # 3: CRC32 mismatch
        assert (st[4 * n:] == byte).all()
        ends = [int(o) + l for o, l in zip(out_off.tolist(), isize)]
        for m in range(n):
            if m != BAD_CRC:
                assert out[int(out_off[m]):ends[m]].tobytes() == expect[m], m
            # include/svx.h: a match copy may touch up to 7 bytes behind a member's end, nothing else outside it
            behind = out[ends[m] + 7:int(out_off[m + 1]) if m + 1 < n else len(out)]
            assert len(behind) >= GUARD - 7 or m + 1 < n
            assert (behind == byte).all(), (m, "bytes between the members were written")
    was = svx_ctx.lib.svx_bgzf_inflate_set_two_pass(tinf.FORMS[form])
    try:
        poisoned(svx_ctx, lambda byte: bgzf_inflate_dev(svx_ctx, payloads, isize, crc, byte), check)
    finally:
        svx_ctx.lib.svx_bgzf_inflate_set_two_pass(was)


@pytest.mark.parametrize("slices", ["one_slice", "slice_per_block"])
def test_bgzf_deflate(svx_ctx, slices):
    """Three blocks (two of 65 280 bytes and a short one) in one launch and in a launch per block: the zlib round trip
    with the container's structure, CRC32 and ISIZE (tabix_reader.check_bgzf), and the member lengths the call reports."""
    rng = np.random.default_rng(3)
    line = b"chr1\t%d\tsvim_asm.DEL.%d\tACGTNNNN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=%d;SVLEN=-55\tGT\t0/1\n"
    data = b"".join(line % (int(p), k, int(p) + 55) for k, p in enumerate(np.sort(rng.integers(1, 1 << 28, 2400))))[:2 * 65280 + 1000]
    assert len(data) == 2 * 65280 + 1000

    def check(got, _):
        blob, sizes = got
        assert tabix_reader.check_bgzf(blob, data) == list(sizes) and len(sizes) == 3
        assert sum(int(s) for s in sizes) + 28 == len(blob)
    was = svx_ctx.lib.svx_bgzf_deflate_set_slice(1) if slices == "slice_per_block" else None
    try:
        poisoned(svx_ctx, lambda _: svx_ctx.bgzf_deflate(data), check)
    finally:
        if was is not None:
            svx_ctx.lib.svx_bgzf_deflate_set_slice(was)


# ------------------------------------------------------------------- the real pattern, without the hook
@pytest.fixture
def fresh():
    """A context of its own: regions that are allocated, and grow, inside the test."""
    ctx = _lib.Context(0)
    yield Watch(ctx, fresh=True)
    ctx.close()


def test_small_linkage_after_a_big_cigar_extract(fresh):
    """2 M ops through svx_cigar_extract, then five small partitions through svx_linkage_cut_batch on what it left."""
    b = synth.synth_cigar_batch(seed=41, ops_target=2_000_000)
    assert 1_500_000 < len(b["cigar"]) < (1 << 23)  # (the two-launch path)
    got = fresh.call(lambda: fresh.ctx.cigar_extract(b["cigar"], b["aln_off"], b["ref_start"], 40))
    exp = orc.cigar_extract(b["cigar"], b["aln_off"], b["ref_start"], 40)
    for k in KEYS:
        assert np.array_equal(got[k], exp[k]), k
    fresh.ctx.set_linkage_group_min(_lib.LINKAGE_LANES_ONLY)
    dist, counts, want = _linkage_case(LINKAGE["lanes"][0], 2.5)
    assert fresh.call(lambda: fresh.ctx.linkage_cut_batch(dist, counts, 2.5)).tolist() == want


def test_small_cigar_text_after_a_big_pair_partition(fresh):
    """The largest one-launch sort (131 072 keys), then ten CIGAR strings through svx_cigar_text_parse_dev."""
    keys = tpair.make_keys(np.random.default_rng(5), 131072, 6 * 24, 250_000_000)
    _check_pair(orc.pair_partition(keys, 1000))(fresh.call(lambda: fresh.ctx.pair_partition(keys, 1000), ("pair_single", len(keys))), None)
    texts = (tsam.GOOD + tsam.BAD)[:10]
    assert any(stw.parse_cigar(t)[0] for t in texts)
    check_cigar_text(texts, fresh.call(lambda: cigar_text_parse_dev(fresh.ctx, texts, 0xA5)))


def test_small_collect_after_a_long_edit_distance(fresh):
    """The 21 000-base pair (boundary streams, a band widened on the way), then a small svx_collect_batch."""
    (pool, ao, al, bo, bl), exp = _edit_case()
    i = len(ao) - 2
    got = fresh.call(lambda: fresh.ctx.edit_distance_batch(pool, ao[i:i + 1], al[i:i + 1], bo[i:i + 1], bl[i:i + 1]))
    assert got.tolist() == [exp[i]]
    b, want = _collect_case("random")
    tcol.same_as_oracle(fresh.call(lambda: tcol.call(fresh.ctx.collect_batch, b)), want)


def test_pair_partition_workspace_grows(fresh):
    for n in (1000, 70001):
        keys, exp = _pair_case(n, 1000)
        _check_pair(exp)(fresh.call(lambda: fresh.ctx.pair_partition(keys, 1000), ("pair_single", n)), None)


def test_streaming_cigar_workspace_grows(fresh):
    fresh.ctx.set_small_batch_ops(0)
    small = _cigar_batches()["mixed_dense"][:3]
    big = synth.synth_cigar_batch(seed=33, mean_m=200, sv_frac=0.5, ops_target=3_000_000)  # satellite density: dense tiles
    for cig, off, rs in (small, (big["cigar"], big["aln_off"], big["ref_start"])):
        lo, hi, n_sig = _dense_bounds(cig, len(cig), 40)
        assert lo > 0
        got = fresh.call(lambda: fresh.ctx.cigar_extract(cig, off, rs, 40), ("streaming", lo, hi))
        exp = orc.cigar_extract(cig, off, rs, 40)
        assert n_sig == len(exp["aln"])
        for k in KEYS:
            assert np.array_equal(got[k], exp[k]), k
