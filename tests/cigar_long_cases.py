"""Batches with ONE alignment of 10^5 to 10^7 ops for the CIGAR walk's carry scans (tests/test_cigar_long_pins.py where
there is no GPU, tests/test_gpu_cigar_long.py on the device): seeded builders, the preconditions every case has to meet —
computed here with numpy from the arrays, asserted by both test modules — and a numpy restatement of the walk.

The walk passes the reference and read cursors "since the last alignment start" from tile to tile through segmented
scans over tile descriptors, and at every level of those scans one branch serves a unit that holds no alignment start at
all.  The units, at the default build macros (svx_cigar.hip):

  streaming path (k_desc_scan, cigar_finish_block, k_cigar_dense), tiles of 4096 ops
      row    65 536 ops    16 tiles, one DPP row of the scan
      wave   262 144       64 tiles, one wave of the scan
      block  4 194 304     1024 tiles, one scan workgroup (its aggregate goes through blk_agg / blk_prefix)
  two-launch path (k_cigar_finish_small), tiles of 1024 ops
      thread 32 768        the 8 folded descriptors (of 4 tiles each) one thread scans itself
      row    524 288       16 threads
      wave   2 097 152     64 threads; the whole batch holds at most 8 388 608 ops

A case is `P` ops of short alignments (0 to 3000 ops each, a few of them empty, the last trimmed), one long alignment of
`L` ops and a tail of short alignments of more than two tiles.  For a unit U the long alignment has L = 2 U + U / 2 ops
and P is U - 1, U, U + 1 or U / 2 + 7, so that it starts on the last op of a unit, on its first, on its second and in
the middle of one.  Behind P = U + 1 an alignment of 2 U + U / 2 ops covers ONE aligned unit, not the two every case has
to cover: those cases get one unit more, L = 3 U + U / 2.

Ops: every code from 0 to 15, lengths 1 to 2000; I and D below 40 except for about one in 300, so that a tile of 4096
ops carries some three signatures at min_len 40 and stays far below the slab of 128 records.  Planted inside the long
alignment: one D of 40 or more in the first tile behind every unit boundary and one in its last tile (the sparse finish
reads the carry there), and two stretches of 300 consecutive I / D ops of 40 or more, each inside one tile and behind at
least one fully covered unit (those tiles take the dense re-walk with the carried-in cursors)."""
import collections
import functools

import numpy as np

MIN_LEN = 40
SLAB = 128          # records of a tile's slab: a tile with more signatures is walked again
DENSE_RUN = 300     # consecutive qualifying ops of a planted stretch
STREAM_TILE, SMALL_TILE = 4096, 1024
SMALL_BATCH_MAX = 1 << 23

Case = collections.namedtuple("Case", "name path tile unit P L")


def _cases():
    out = []

    def add(path, tile, level, U, Ps, extra=0):
        for P in Ps:
            L = 2 * U + U // 2 + (U if P == U + 1 else 0) + extra
            tag = {U - 1: "U-1", U: "U", U + 1: "U+1", U // 2 + 7: "U/2+7"}[P]
            out.append(Case("%s-%s-%s%s" % (path, level, tag, "-ends-on-tile" if extra else ""), path, tile, U, P, L))

    for level, U in (("row", 65536), ("wave", 262144)):
        add("streaming", STREAM_TILE, level, U, (U - 1, U, U + 1, U // 2 + 7))
    add("streaming", STREAM_TILE, "block", 4194304, (4194304 - 1, 4194304 // 2 + 7))
    for level, U in (("thread", 32768), ("row", 524288)):
        add("small", SMALL_TILE, level, U, (U - 1, U, U + 1, U // 2 + 7))
    add("small", SMALL_TILE, "wave", 2097152, (2097152 - 1, 2097152 // 2 + 7))
    # the long alignment starts inside a tile and ends on a tile boundary: the next alignment starts at tile op 0
    add("small", SMALL_TILE, "thread", 32768, (32768 // 2 + 7,), extra=SMALL_TILE - 7)
    return out


CASES = collections.OrderedDict((c.name, c) for c in _cases())
STREAMING = [n for n, c in CASES.items() if c.path == "streaming"]
SMALL = [n for n, c in CASES.items() if c.path == "small"]
BLOCK_LEVEL = [n for n in STREAMING if "-block-" in n]
CAP_CASE = "streaming-wave-U/2+7"   # the one that also runs svx_cigar_extract_dev with half the capacity

# M, =, X advance both cursors: three ops in five, so that 10^7 ops of a mean length of 1000 move either cursor past 2^32
_OP_WEIGHTS = np.array([0.35, 0.10, 0.10, 0.01, 0.04, 0.01, 0.01, 0.15, 0.10, 0.01] + [0.02] * 6)


def _codes(*codes):
    """Lookup table over the 16 op codes: True for `codes`."""
    t = np.zeros(16, bool)
    t[list(codes)] = True
    return t


def random_ops(rng, n):
    """n packed ops: every code, lengths 1-2000; I / D are 1-39 long except for about one in 300."""
    op = np.searchsorted(np.cumsum(_OP_WEIGHTS)[:-1], rng.random(n, dtype=np.float32), side="right").astype(np.uint32)
    ln = rng.integers(1, 2001, size=n, dtype=np.uint32)
    indel = (op == 1) | (op == 2)
    short = indel & (rng.random(n) >= 1.0 / 300)
    ln[short] = 1 + ln[short] % (MIN_LEN - 1)
    ln[indel & ~short] = np.maximum(ln[indel & ~short], MIN_LEN)
    return (ln << 4) | op


def short_lengths(rng, total):
    """Op counts of short alignments that add up to `total`: 1 to 3000 each, the last trimmed, every fifth followed by
    an empty one and the first by two."""
    out, left = [], total
    while left > 0:
        n = min(int(rng.integers(1, 3001)), left)
        out.append(n)
        left -= n
        if len(out) % 6 == 1:
            out += [0] * (2 if len(out) == 1 else 1)
    return out


def _plant(cig, rng, at, op):
    cig[at] = (np.uint32(rng.integers(MIN_LEN, 2001)) << 4) | np.uint32(op)


@functools.lru_cache(maxsize=2)
def build(name):
    """-> dict(cigar, aln_off, ref_start, long): packed words, offsets (uint64), reference starts (int32) and the index
    of the long alignment.  The two latest cases stay cached: the tests share the arrays and leave them unchanged."""
    case = CASES[name]
    U, P, L, tile = case.unit, case.P, case.L, case.tile
    rng = np.random.default_rng([20261019, U, P, L])
    front = short_lengths(rng, P)
    tail = short_lengths(rng, 2 * tile + 1237)
    if case.path == "small":
        assert P + L + sum(tail) <= SMALL_BATCH_MAX
    lengths = front + [L] + tail
    aln_off = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    cig = random_ops(rng, int(aln_off[-1]))
    s, e = P, P + L
    b0 = -(-s // U) * U                       # first unit boundary at or behind the start
    for m in range(b0, e, U):                 # a D in the first tile behind every unit boundary inside the alignment
        _plant(cig, rng, m + min(17, e - m - 1), 2)
    _plant(cig, rng, e - 1, 2)                # and one in its last tile: its last op
    # dense stretches, each inside one tile: in the second covered unit, and behind it where the alignment goes on for
    # two more tiles (otherwise at the end of the second covered unit)
    first = b0 + U + 3 * tile + 100
    second = b0 + 2 * U + tile + 100 if b0 + 2 * U + 2 * tile <= e else b0 + 2 * U - 2 * tile + 100
    for at in (first, second):
        assert s <= at and at + DENSE_RUN <= e and at // tile == (at + DENSE_RUN - 1) // tile
        ops = rng.integers(1, 3, size=DENSE_RUN).astype(np.uint32)
        cig[at:at + DENSE_RUN] = (rng.integers(MIN_LEN, 2001, size=DENSE_RUN).astype(np.uint32) << 4) | ops
    # clips in front (query_alignment_start of the statistics): S on every third alignment, H S S on the long one
    lead = aln_off[:-1][np.diff(aln_off.astype(np.int64)) >= 2][::3].astype(np.int64)
    cig[lead] = (cig[lead] & ~np.uint32(15)) | np.uint32(4)
    cig[s:s + 3] = (rng.integers(1, 2001, size=3).astype(np.uint32) << 4) | np.array([5, 4, 4], np.uint32)
    ref_start = rng.integers(0, 1 << 28, size=len(lengths)).astype(np.int32)
    for a in (cig, aln_off, ref_start):
        a.setflags(write=False)
    return dict(cigar=cig, aln_off=aln_off, ref_start=ref_start, long=len(front))


def facts(name, batch):
    """What a case has to be, measured on its arrays."""
    case = CASES[name]
    cig, off = batch["cigar"], batch["aln_off"].astype(np.int64)
    n_ops, tile, U = int(off[-1]), case.tile, case.unit
    sizes = np.diff(off)
    a = int(np.argmax(sizes))
    s, e = int(off[a]), int(off[a + 1])
    op, ln = cig & 15, cig >> 4
    qualifying = np.nonzero(((op == 1) | (op == 2)) & (ln >= MIN_LEN))[0]
    per_tile = np.bincount(qualifying // tile, minlength=-(-n_ops // tile))
    inside = np.zeros(len(per_tile), bool)
    inside[-(-s // tile):e // tile] = True    # tiles that lie in the long alignment with all their ops
    adv_ref = np.where(_codes(0, 2, 7, 8)[op[s:e]], ln[s:e], 0).sum(dtype=np.uint64)
    adv_read = np.where(_codes(0, 1, 4, 7, 8)[op[s:e]], ln[s:e], 0).sum(dtype=np.uint64)
    boundaries = np.arange(-(-s // U) * U, e, U)
    planted = [bool(per_tile[m // tile]) and bool(np.any((qualifying >= m) & (qualifying < min(e, (m // tile + 1) * tile))
                                                          & (op[qualifying] == 2))) for m in boundaries.tolist()]
    return dict(long=a, long_ops=e - s, start=s, end=e, n_ops=n_ops, other_max=int(np.delete(sizes, a).max()),
                n_empty=int((sizes == 0).sum()), covered_units=max(0, e // U - -(-s // U)),
                dense_inside=int((per_tile[inside] > SLAB).sum()), dense_outside=int((per_tile[~inside] > SLAB).sum()),
                sparse_max=int(per_tile[per_tile <= SLAB].max()), boundary_signatures=all(planted) and len(planted) >= 2,
                last_tile_signature=bool(np.any((qualifying >= max(s, (e - 1) // tile * tile)) & (qualifying < e))),
                codes=set(np.unique(op).tolist()), max_len=int(ln.max()), min_len=int(ln.min()),
                tail_ops=n_ops - e, adv_ref=int(adv_ref), adv_read=int(adv_read),
                next_starts_on_tile=e % tile == 0 and e < n_ops)


def check_preconditions(name, batch):
    """The conditions of the module docstring, asserted on the arrays of one case."""
    case, f = CASES[name], facts(name, batch)
    assert f["long"] == batch["long"] and f["long_ops"] == case.L and f["start"] == case.P, f
    assert f["other_max"] <= 3000 and f["n_empty"] >= 1, f
    assert f["covered_units"] >= 2, f                       # two aligned units of the level hold no start at all...
    assert f["dense_inside"] >= 2 and f["dense_outside"] == 0, f   # ...two tiles behind them are walked again, no other is
    assert f["sparse_max"] <= SLAB // 4, f                  # (far below the slab)
    assert f["boundary_signatures"] and f["last_tile_signature"], f
    assert f["codes"] == set(range(16)) and f["min_len"] >= 1 and f["max_len"] == 2000, f
    assert f["tail_ops"] > 2 * case.tile, f
    if case.path == "small":
        assert f["n_ops"] <= SMALL_BATCH_MAX, f
    if name in BLOCK_LEVEL:
        assert f["adv_ref"] > 1 << 32 and f["adv_read"] > 1 << 32, f  # both cursors wrap
    if name.endswith("-ends-on-tile"):
        assert f["next_starts_on_tile"] and f["start"] % case.tile != 0, f
    return f


# ------------------------------------------------------------------------------ the walk, restated
# analyze_cigar_indel (SVIM_intra.py:8-30): M, = and X advance both cursors, I and S the read cursor, D the
# reference cursor, every other code nothing; an I or a D of min_length or more is reported with the cursors in front of
# it.  analyze_alignment_indel adds reference_start (:36-43).  The cursors are 32-bit in the library's output.
def restated_extract(cigar, aln_off, ref_start, min_len):
    op, ln = cigar & 15, (cigar >> 4).astype(np.uint64)
    off = np.asarray(aln_off).astype(np.int64)
    before_ref = np.zeros(len(cigar) + 1, np.uint64)
    before_read = np.zeros(len(cigar) + 1, np.uint64)
    np.cumsum(np.where(_codes(0, 2, 7, 8)[op], ln, np.uint64(0)), dtype=np.uint64, out=before_ref[1:])
    np.cumsum(np.where(_codes(0, 1, 4, 7, 8)[op], ln, np.uint64(0)), dtype=np.uint64, out=before_read[1:])
    at = np.nonzero(((op == 1) | (op == 2)) & (ln >= np.uint64(min_len)))[0]
    aln = np.searchsorted(off, at, side="right") - 1   # the last alignment that starts at or before the op
    first = off[aln]
    wrap = np.uint64(0xFFFFFFFF)
    ref = ((before_ref[at] - before_ref[first]) & wrap) + np.asarray(ref_start).astype(np.int64)[aln].astype(np.uint64)
    return {"aln": aln.astype(np.uint32), "ref_pos": (ref & wrap).astype(np.uint32),
            "read_pos": ((before_read[at] - before_read[first]) & wrap).astype(np.uint32),
            "len": ln[at].astype(np.uint32), "type": (op[at] == 2).astype(np.uint8)}


# pysam's per-alignment quantities: reference_end - reference_start sums M, D, N, = and X;
# query_alignment_start the S ops in front of the first op that is neither S nor H; query_alignment_end adds M, I, = and
# X to it; infer_read_length sums M, I, S, =, X and H; the hard-clipped bases are the H ops.
def restated_stats(cigar, aln_off):
    op, ln = cigar & 15, (cigar >> 4).astype(np.uint64)
    off = np.asarray(aln_off).astype(np.int64)

    def per_alignment(codes, last=None):
        """Sum of the lengths of the ops of `codes`, from an alignment's first op to its last (or up to `last`)."""
        total = np.zeros(len(cigar) + 1, np.uint64)
        np.cumsum(np.where(_codes(*codes)[op], ln, np.uint64(0)), dtype=np.uint64, out=total[1:])
        return ((total[off[1:] if last is None else last] - total[off[:-1]]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)

    body = np.zeros(len(cigar) + 1, np.int64)          # ops that are no clip, counted in front of every op
    np.cumsum(~_codes(4, 5)[op], out=body[1:])
    first_body = np.minimum(np.searchsorted(body, body[off[:-1]], side="right") - 1, off[1:])  # per alignment (or its end)
    q_start = per_alignment((4,), last=first_body)
    return {"ref_len": per_alignment((0, 2, 3, 7, 8)), "q_start": q_start,
            "q_end": q_start + per_alignment((0, 1, 7, 8)), "read_len": per_alignment((0, 1, 4, 5, 7, 8)),
            "n_hard": per_alignment((5,))}
