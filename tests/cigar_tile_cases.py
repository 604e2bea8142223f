"""A case table for the CIGAR tile walk (process_tile in svx_cigar.hip): the per-round LDS queue, the stage buffer and its
drains to the slab, the slab bound, the `prec` / `own` flags, the start mask with the alignment index derived from it,
and the descriptor that sends a tile to the dense re-walk.  tests/test_cigar_tile_cases.py holds the table to its own
preconditions where there is no GPU, tests/test_gpu_cigar_tiles.py runs it on the device.

Builder.  A case is described per round of 1024 ops by how many ops qualify (I or D with len >= MIN_LEN), where they sit
(`place`) and where alignments start.  The k-th qualifying op of a case is MIN_LEN + k long and the ops alternate I, D,
so that a misplaced or swapped record shows; every other op is M, =, X, S, N, H, P or a short I / D of length 1-9, so
that the two cursors differ from each other and from the op index.  The same arrays run on both paths: a round is a
tile of the two-launch path, four consecutive rounds are a tile of the streaming path.

Facts.  facts(cigar, aln_off, path) computes, from the arrays and the constants K alone (never from an output), per
tile: the counts per round and in all, whether the tile goes dense (count > SLAB, or a round with count > QUEUE), the
drains of the stage buffer (by the rule tile_cnt + C - stage_base > STAGE), the second flush pass, the records that go
past the stage buffer straight to the slab, `prec`, `own`, the starts and the passes of the mask loop, `dup`, and per
round whether every length is below 2^24.

Classes.  CLASSES names every situation the table has to show, per path; a case lists the classes it shows (`shows`)
and, where its name promises numbers, those numbers (`expect`).  check_preconditions holds every case to both and every
class to at least one case on each path it applies to.  The constants are literals HERE (K): a retune of svx_cigar.hip
has to move the table with it (the CPU module compares K with the #define lines), and a literal moved by one makes
check_preconditions fail (the CPU module's mutation test)."""
import collections
import functools
import types
import zlib

import numpy as np

MIN_LEN = 40
# The thresholds of svx_cigar.hip, as literals: SVX_LANE_OPS, SVX_ROUNDS, SVX_QUEUE, SVX_QUEUE_SMALL, SVX_STAGE,
# SVX_SLAB, kFinLanes, kFinTiles.  (The one place the table can be moved from: facts() and the classes read K.)
K = dict(LANE_OPS=16, ROUNDS=4, QUEUE=64, QUEUE_SMALL=96, STAGE=64, SLAB=128, FIN_LANES=16, FIN_TILES=16)
DEFINES = dict(SVX_LANE_OPS="LANE_OPS", SVX_ROUNDS="ROUNDS", SVX_QUEUE="QUEUE", SVX_QUEUE_SMALL="QUEUE_SMALL",
               SVX_STAGE="STAGE", SVX_SLAB="SLAB")
WAVE = 64               # lanes: alignments per pass of the start-mask loop, records per flush pass
ROUND = 1024            # ops per round at 16 ops per lane
TILE = 4096             # ops per tile of the streaming path; the cases are laid out in these
FOLD = 4                # tiles per folded descriptor of the two-launch path (= waves of a tile workgroup)
PATHS = ("streaming", "two_launch")
MAX_LEN = (1 << 28) - 1

Case = collections.namedtuple("Case", "name family cigar aln_off ref_start shows expect")


# ------------------------------------------------------------------------------------------------------ builder
def place(count, how="spread"):
    """Positions (0 .. 1023) of a round's `count` qualifying ops."""
    if how == "packed0":        # the fewest lanes, from lane 0: all 16 ops of a lane emit
        return list(range(count))
    if how == "packed63":       # ... ending with lane 63
        return list(range(ROUND - count, ROUND))
    if count > WAVE or how == "even":   # more than one per lane: evenly over the round
        return [(k * ROUND) // count for k in range(count)]
    lanes = [(k * WAVE) // count + (WAVE // count) // 2 for k in range(count)]
    if how == "spread":         # one per lane over the whole wave, the slot differs from lane to lane
        return [16 * l + (5 * k + 3) % 16 for k, l in enumerate(lanes)]
    if how == "slot0":
        return [16 * l for l in lanes]
    if how == "slot15":
        return [16 * l + 15 for l in lanes]
    if how == "ends":           # lanes 0 and 63 only
        assert count <= 32
        h = count // 2
        return list(range(h)) + list(range(ROUND - (count - h), ROUND))
    raise ValueError(how)


def rounds_at(first_round, profile, how="spread"):
    """Global positions of the qualifying ops of consecutive rounds with the counts of `profile`."""
    out = []
    for r, c in enumerate(profile):
        out += [(first_round + r) * ROUND + p for p in place(c, how)]
    return out


_FILL_OPS = np.array([0, 7, 8, 4, 3, 5, 6, 1, 2], np.uint32)
_FILL_P = np.array([.30, .15, .10, .05, .05, .05, .05, .125, .125])


def make(name, family, n_ops, qual, starts, shows, expect=(), overrides=None):
    """One case: `qual` the positions of the qualifying ops, `starts` the alignment offsets (the first is 0; equal
    offsets are empty alignments; n_ops may occur), `overrides` {position: (op, len)} placed last."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    cig = (rng.integers(1, 10, size=n_ops).astype(np.uint32) << 4) | rng.choice(_FILL_OPS, size=n_ops, p=_FILL_P)
    qual = np.array(sorted(set(qual)), np.int64)
    assert len(qual) == 0 or (0 <= qual[0] and qual[-1] < n_ops), name
    k = np.arange(len(qual), dtype=np.uint32)
    cig[qual] = ((MIN_LEN + k) << 4) | (1 + (k & 1))
    for pos, (op, ln) in (overrides or {}).items():
        cig[pos] = (np.uint32(ln) << 4) | np.uint32(op)
    starts = sorted(starts)
    assert starts[0] == 0 and starts[-1] <= n_ops, name
    aln_off = np.array(starts + [n_ops], np.uint64)
    ref_start = (rng.permutation(len(starts)) * 1009 + rng.integers(0, 1 << 27)).astype(np.int32)
    for a in (cig, aln_off, ref_start):
        a.setflags(write=False)
    return Case(name, family, cig, aln_off, ref_start, tuple(shows), tuple(expect))


# -------------------------------------------------------------------------------------------------------- facts
def facts(cigar, aln_off, path, k=None, min_len=MIN_LEN):
    """Every quantity of the module docstring for `path`, from the input arrays and the constants `k` alone."""
    k = k or K
    rnd = WAVE * k["LANE_OPS"]
    lane_ops = k["LANE_OPS"]
    rpt = k["ROUNDS"] if path == "streaming" else 1
    q = k["QUEUE"] if path == "streaming" else k["QUEUE_SMALL"]
    T, stage, slab = rnd * rpt, k["STAGE"], k["SLAB"]
    off = np.asarray(aln_off).astype(np.int64)
    n_ops = int(off[-1])
    cig = np.asarray(cigar[:n_ops], np.uint32)
    op, ln = cig & 15, cig >> 4
    emit = ((op == 1) | (op == 2)) & (ln >= min_len)
    all_starts = off[:-1][off[:-1] < n_ops]
    n_tiles = -(-n_ops // T)
    # cursor sums since the alignment's first op, in 64 bits: do they pass 2^32 in front of a signature?
    adv_r = np.concatenate(([0], np.cumsum(np.where(np.isin(op, (0, 2, 7, 8)), ln, 0).astype(np.uint64), dtype=np.uint64)))
    adv_d = np.concatenate(([0], np.cumsum(np.where(np.isin(op, (0, 1, 4, 7, 8)), ln, 0).astype(np.uint64), dtype=np.uint64)))
    at = np.nonzero(emit)[0]
    first = off[np.searchsorted(off, at, side="right") - 1]
    tiles, last_start_tile = [], -1
    for t in range(n_tiles):
        g0, g1 = t * T, min(t * T + T, n_ops)
        e = np.nonzero(emit[g0:g1])[0]
        s = all_starts[(all_starts >= g0) & (all_starts < g1)] - g0
        su, mult = np.unique(s, return_counts=True)
        n_rounds = -(-(g1 - g0) // rnd)
        rc = [int(((e // rnd) == r).sum()) for r in range(n_rounds)]
        x = types.SimpleNamespace(index=t, tile_len=g1 - g0, rounds=rc, total=len(e))
        # the stage buffer: tile_cnt, stage_base and the drains, round by round as process_tile keeps them
        cnt = base = direct = 0
        x.drains, x.overflow_rounds, x.second_pass = [], [], False
        for r, c in enumerate(rc):
            if not c:
                continue
            if cnt + c - base > stage:
                x.drains.append((r, cnt - base))
                base = cnt
            n_here = min(c, q)
            x.second_pass |= n_here > WAVE
            if q > stage:   # records past the stage buffer's room go straight to the slab
                direct += sum(1 for rank in range(cnt, cnt + n_here) if rank - base >= stage and rank < slab)
            if c > q:
                x.overflow_rounds.append(r)
            cnt += c
        x.last_drain = cnt - base if cnt - base < stage else stage
        x.dense = cnt > slab or bool(x.overflow_rounds)
        x.direct_slab = direct
        x.beyond_slab = max(0, cnt - slab)
        # flags of the records
        x.prec = int((e < (su[0] if len(su) else T)).sum())
        i = np.searchsorted(su, e, side="right") - 1
        x.own = int(((i >= 0) & (su[np.maximum(i, 0)] >= e - e % lane_ops)).sum()) if len(su) else 0
        x.starts, x.dup, x.passes = len(s), bool((mult > 1).any()), len(s) // WAVE + 1
        x.start_on_emit = int(emit[g0 + su].sum())
        x.emit_before_start = int(emit[(g0 + su - 1)[g0 + su > 0]].sum())
        x.since_start = t - last_start_tile if not len(s) and last_start_tile >= 0 else 0
        if len(s):
            last_start_tile = t
        x.around = set()
        if len(s) == 1 and s[0] != 0:   # one start inside the tile: where the signatures lie around it
            p = int(s[0])
            lb, rb = p - p % lane_ops, p - p % rnd
            for tag, lo, hi in (("lane_before", lb, p), ("lane_after", p + 1, lb + lane_ops), ("lanes_before", rb, lb),
                                ("lanes_after", lb + lane_ops, rb + rnd), ("rounds_before", 0, rb), ("rounds_after", rb + rnd, T)):
                if ((e >= lo) & (e < hi)).any():
                    x.around.add(tag)
        is_start = np.zeros(g1 - g0, bool)
        is_start[su] = True
        full = is_start[:(g1 - g0) // lane_ops * lane_ops].reshape(-1, lane_ops).all(axis=1)
        per_round = [is_start[r * rnd:(r + 1) * rnd] for r in range(n_rounds)]
        x.lane_of_starts = any(bool(full[r * WAVE:(r + 1) * WAVE].any()) and not bool(per_round[r].all()) for r in range(n_rounds))
        x.round_of_starts = [r for r in range(n_rounds) if len(per_round[r]) == rnd and per_round[r].all()]
        x.empties = set()
        for p, m in zip(su[mult > 1].tolist(), mult[mult > 1].tolist()):
            x.empties.add((m, "emit" if emit[g0 + p] else ("op0" if p == 0 else "inside")))
        x.fast24 = [bool((ln[g0 + r * rnd:min(g0 + (r + 1) * rnd, g1)] < (1 << 24)).all()) for r in range(n_rounds)]
        x.place = []
        for r in range(n_rounds):
            pr = e[(e // rnd) == r] % rnd
            lanes, slots, f = pr // lane_ops, pr % lane_ops, set()
            if len(pr) >= 2 and len(set(lanes.tolist())) == len(pr):
                if len(set(slots.tolist())) > 1 and lanes.max() - lanes.min() >= WAVE // 2:
                    f.add("one_per_lane")
                if (slots == 0).all():
                    f.add("slot0")
                if (slots == lane_ops - 1).all():
                    f.add("slot15")
                    if len(pr) == WAVE:
                        f.add("full_ballot15")
            if len(pr) >= lane_ops and len(set(lanes.tolist())) == -(-len(pr) // lane_ops):
                f.add("packed")
                if lanes.min() == 0:
                    f.add("packed_lane0")
                if lanes.max() == WAVE - 1:
                    f.add("packed_lane63")
            if set(lanes.tolist()) == {0, WAVE - 1}:
                f.add("ends")
            x.place.append(f)
        tiles.append(x)
    wrapped = (adv_r[at] - adv_r[first] >= (1 << 32)), (adv_d[at] - adv_d[first] >= (1 << 32))
    return types.SimpleNamespace(
        path=path, tile_ops=T, queue=q, n_ops=n_ops, n_tiles=n_tiles, tiles=tiles, n_sig=int(emit.sum()),
        dense=[x.index for x in tiles if x.dense], last_op_emits=bool(emit[n_ops - 1]),
        empties_at_end=int((off[:-1] == n_ops).sum()), max_emit_len=int(ln[at].max()) if len(at) else 0,
        wrap_ref=bool(wrapped[0].any()), wrap_read=bool(wrapped[1].any()))


# ------------------------------------------------------------------------------------------------------ classes
def _any(f):
    return lambda F, k: any(f(x, k) for x in F.tiles)


def _staged(x):
    return x.total > 0 and not x.dense


def _classes():
    """id -> (paths, predicate(facts, k)).  's': streaming, 't': two-launch."""
    c = collections.OrderedDict()

    def add(cid, paths, pred):
        assert cid not in c
        c[cid] = (tuple({"s": "streaming", "t": "two_launch"}[p] for p in paths), pred)

    # ---- count profiles of a streaming tile (four rounds)
    add("s.tile.empty", "s", _any(lambda x, k: x.total == 0 and len(x.rounds) == k["ROUNDS"]))
    add("s.round.0", "s", _any(lambda x, k: _staged(x) and 0 in x.rounds))
    add("s.round.1", "s", _any(lambda x, k: _staged(x) and 1 in x.rounds))
    add("s.round.queue-1", "s", _any(lambda x, k: _staged(x) and k["QUEUE"] - 1 in x.rounds))
    add("s.round.queue", "s", _any(lambda x, k: _staged(x) and k["QUEUE"] in x.rounds))
    add("s.round.queue+1.alone", "s", _any(lambda x, k: x.dense and x.total == k["QUEUE"] + 1 and max(x.rounds) == x.total))
    add("s.total.slab-1", "s", _any(lambda x, k: x.total == k["SLAB"] - 1 and not x.dense))
    add("s.total.slab", "s", _any(lambda x, k: x.total == k["SLAB"] and not x.dense and len([r for r in x.rounds if r]) == 4))
    add("s.total.slab+1", "s", _any(lambda x, k: x.total == k["SLAB"] + 1 and x.dense and not x.overflow_rounds
                                    and len([r for r in x.rounds if r]) == 4))
    add("s.profile.q-q-0-0", "s", _any(lambda x, k: x.rounds == [k["QUEUE"], k["QUEUE"], 0, 0] and not x.dense))
    add("s.profile.q-q-1-0", "s", _any(lambda x, k: x.rounds == [k["QUEUE"], k["QUEUE"], 1, 0] and x.dense and not x.overflow_rounds))
    add("s.profile.q-0-0-q", "s", _any(lambda x, k: x.rounds == [k["QUEUE"], 0, 0, k["QUEUE"]] and not x.dense))
    add("s.drain.before_rounds_1_and_2", "s", _any(lambda x, k: [r for r, _ in x.drains] == [1, 2] and x.total == k["SLAB"] and not x.dense))
    add("s.drain.one_record_then_a_full_round", "s", _any(lambda x, k: x.drains == [(1, 1)] and x.last_drain == k["STAGE"] and not x.dense))
    add("s.drain.full_buffer_mid_tile", "s", _any(lambda x, k: x.drains == [(2, k["STAGE"])] and not x.dense))
    add("s.drain.last.stage", "s", _any(lambda x, k: x.drains and x.last_drain == k["STAGE"] and x.total == k["SLAB"] and not x.dense))
    add("s.drain.last.stage-1", "s", _any(lambda x, k: x.drains and x.last_drain == k["STAGE"] - 1 and not x.dense))
    add("s.drain.none", "s", _any(lambda x, k: _staged(x) and not x.drains and x.total == x.last_drain > 1))
    add("s.beyond_slab.without_overflow", "s", _any(lambda x, k: x.beyond_slab >= k["SLAB"] and not x.overflow_rounds))
    add("s.beyond_slab.with_overflow", "s", _any(lambda x, k: x.beyond_slab > 0 and len(x.overflow_rounds) >= 2))
    add("s.overflow.round0", "s", _any(lambda x, k: x.overflow_rounds == [0] and x.total <= k["SLAB"]))
    add("s.overflow.round3", "s", _any(lambda x, k: x.overflow_rounds == [k["ROUNDS"] - 1] and x.total <= k["SLAB"]))
    # ---- count profiles of a two-launch tile (one round)
    for tag, n in (("stage-1", lambda k: k["STAGE"] - 1), ("stage", lambda k: k["STAGE"]), ("stage+1", lambda k: k["STAGE"] + 1),
                   ("queue-1", lambda k: k["QUEUE_SMALL"] - 1), ("queue", lambda k: k["QUEUE_SMALL"]),
                   ("queue+1", lambda k: k["QUEUE_SMALL"] + 1)):
        add("t.count." + tag, "t", _any(lambda x, k, n=n, tag=tag: x.total == n(k) and x.dense == (tag == "queue+1")))
    add("t.second_flush_pass", "t", _any(lambda x, k: _staged(x) and x.second_pass))
    add("t.one_flush_pass", "t", _any(lambda x, k: _staged(x) and not x.second_pass and x.total == WAVE))
    add("t.past_the_stage_buffer", "t", _any(lambda x, k: _staged(x) and x.direct_slab == k["QUEUE_SMALL"] - k["STAGE"]))
    add("t.count.above_slab_without_overflow", "t", _any(lambda x, k: x.total > k["SLAB"] and not x.overflow_rounds))
    # ---- placement of a round's signatures
    for tag in ("one_per_lane", "packed_lane0", "packed_lane63", "slot0", "slot15", "full_ballot15", "ends"):
        add("p." + tag, "st", _any(lambda x, k, tag=tag: _staged(x) and any(tag in f for f in x.place)))
    # ---- alignment starts
    add("a.none.began_one_tile_earlier", "st", _any(lambda x, k: x.since_start == 1 and _staged(x) and x.prec == x.total))
    add("a.none.began_two_tiles_earlier", "st", _any(lambda x, k: x.since_start == 2 and _staged(x) and x.prec == x.total))
    add("a.only_at_op0", "st", _any(lambda x, k: x.starts == 1 and x.prec == 0 and _staged(x) and x.total > x.own > 0))
    for tag in ("lane_before", "lane_after", "lanes_before", "lanes_after"):
        add("a.single." + tag, "st", _any(lambda x, k, tag=tag: tag in x.around and _staged(x)))
    for tag in ("rounds_before", "rounds_after"):
        add("a.single." + tag, "s", _any(lambda x, k, tag=tag: tag in x.around and _staged(x)))
    add("a.start_on_a_qualifying_op", "st", _any(lambda x, k: x.start_on_emit > 0 and _staged(x)))
    add("a.qualifying_op_before_a_start", "st", _any(lambda x, k: x.emit_before_start > 0 and _staged(x)))
    add("a.sixteen_starts_in_a_lane", "st", _any(lambda x, k: x.lane_of_starts and _staged(x)))
    for n in (63, 64, 65, 129):
        add("a.starts.%d" % n, "st", _any(lambda x, k, n=n: x.starts == n and x.passes == n // WAVE + 1 and not x.dup and x.total > 0))
    add("a.every_op_of_a_round_starts", "st", _any(lambda x, k: any(x.rounds[r] == WAVE for r in x.round_of_starts) and not x.dup))
    for m in (2, 3):
        for where in ("inside", "op0", "emit"):
            add("e.%d.%s.staged" % (m, where), "st", _any(lambda x, k, m=m, where=where: (m, where) in x.empties and _staged(x)))
            add("e.%d.%s.dense" % (m, where), "st", _any(lambda x, k, m=m, where=where: (m, where) in x.empties and x.dense))
    add("e.at_n_ops", "st", lambda F, k: F.empties_at_end >= 2 and F.n_sig > 0)
    # ---- the last tile
    for n in (1, 15, 16, 17, 1023):
        add("tail.%d" % n, "st", lambda F, k, n=n: F.tiles[-1].tile_len == n and F.last_op_emits and F.n_tiles > 1)
    add("tail.1025", "s", lambda F, k: F.tiles[-1].tile_len == 1025 and F.last_op_emits and F.n_tiles > 1)
    # ---- lengths
    add("len.one_generic_round_beside_three_24bit", "s", _any(lambda x, k: x.fast24.count(False) == 1 and len(x.fast24) == 4
                                                             and min(x.rounds) > 0 and _staged(x)))
    add("len.generic_round", "t", _any(lambda x, k: x.fast24 == [False] and _staged(x)))
    add("len.2^28-1_qualifies", "st", lambda F, k: F.max_emit_len == MAX_LEN)
    add("len.cursors_wrap", "st", lambda F, k: F.wrap_ref and F.wrap_read)
    # ---- the finish kernel of the two-launch path: FIN_TILES tiles per workgroup, FOLD descriptors folded into one
    for n in (1, 3, 4, 5, 15, 16, 17, 33):
        add("f.tiles.%d" % n, "t", lambda F, k, n=n: F.n_tiles == n and F.n_sig > 0)

    def dense_at(mod, rem):
        def pred(F, k):
            m = mod(k)
            r = rem(k)
            for t in F.dense:   # ... beside sparse tiles that carry signatures in the same unit
                unit = [x for x in F.tiles if x.index // m == t // m and x.index != t]
                if t % m == r and len(unit) == m - 1 and all(_staged(x) for x in unit):
                    return True
            return False
        return pred
    add("f.dense.first_of_a_fold", "t", dense_at(lambda k: FOLD, lambda k: 0))
    add("f.dense.last_of_a_fold", "t", dense_at(lambda k: FOLD, lambda k: FOLD - 1))
    add("f.dense.first_of_a_workgroup", "t", dense_at(lambda k: k["FIN_TILES"], lambda k: 0))
    add("f.dense.last_of_a_workgroup", "t", dense_at(lambda k: k["FIN_TILES"], lambda k: k["FIN_TILES"] - 1))

    def wg_all_dense(F, k):
        n = k["FIN_TILES"]
        wgs = [F.tiles[i:i + n] for i in range(0, F.n_tiles, n)]
        return (any(len(w) == n and all(x.dense for x in w) for w in wgs)
                and any(len(w) == n and all(_staged(x) for x in w) for w in wgs))
    add("f.workgroup_all_dense_beside_a_sparse_one", "t", wg_all_dense)
    add("f.more_dense_tiles_than_workgroups", "t", lambda F, k: len(F.dense) > -(-F.n_tiles // k["FIN_TILES"])
        and len(F.dense) < F.n_tiles)
    return c


CLASSES = _classes()
# the one class no input reaches, and why
EXEMPT = {"t.count.above_slab_without_overflow": "a one-round tile above the slab (128) is above its queue (96): the round overflows"}


# --------------------------------------------------------------------------------------------------------- table
def _table():
    out = []

    def add(*a, **kw):
        out.append(make(*a, **kw))

    S, T2 = "streaming", "two_launch"
    # ---- count profiles: tile 0 sparse with the batch's only start, tile 1 the profile (every record of it lacks the
    # carry-in), tile 2 a tail of 40 ops whose signature needs the carry ACROSS the profile tile
    lead = rounds_at(0, (2, 1, 0, 1))
    tail = [2 * TILE + 20]
    n3 = 2 * TILE + 40

    def profile(prof, shows, expect=(), how="spread", behind=True):
        name = "profile-" + "-".join(str(c) for c in prof) + ("" if how == "spread" else "-" + how)
        tot, over = sum(prof), [r for r, c in enumerate(prof) if c > K["QUEUE"]]
        exp = [(S, 1, "rounds", list(prof)), (S, 1, "total", tot), (S, 1, "prec", tot), (S, 1, "own", 0),
               (S, 1, "dense", tot > 128 or any(c > 64 for c in prof)), (S, 1, "overflow_rounds", over)]
        exp += [(T2, 4 + r, "total", c) for r, c in enumerate(prof)] + [(T2, 4 + r, "dense", c > 96) for r, c in enumerate(prof)]
        add(name, "counts", n3 if behind else 2 * TILE, lead + rounds_at(4, prof, how) + (tail if behind else []), [0], shows,
            exp + list(expect))

    profile((0, 0, 0, 0), ["s.tile.empty", "a.none.began_two_tiles_earlier@streaming"])
    profile((1, 0, 0, 0), ["s.round.0", "s.round.1", "a.none.began_one_tile_earlier@streaming"],
            [(S, 1, "drains", []), (S, 1, "last_drain", 1)])
    profile((63, 0, 0, 0), ["s.round.queue-1", "t.count.stage-1", "s.drain.none", "p.one_per_lane"], [(S, 1, "last_drain", 63)])
    profile((64, 0, 0, 0), ["s.round.queue", "t.count.stage", "t.one_flush_pass", "a.none.began_one_tile_earlier@two_launch"],
            [(S, 1, "drains", []), (S, 1, "last_drain", 64), (T2, 4, "second_pass", False)])
    profile((65, 0, 0, 0), ["s.round.queue+1.alone", "s.overflow.round0", "t.count.stage+1", "t.second_flush_pass"],
            [(T2, 4, "second_pass", True), (T2, 4, "direct_slab", 1)])
    profile((0, 0, 0, 65), ["s.overflow.round3"])
    profile((32, 32, 32, 31), ["s.total.slab-1"], [(S, 1, "drains", [(2, 64)]), (S, 1, "last_drain", 63)])
    profile((32, 32, 32, 32), ["s.total.slab"], [(S, 1, "drains", [(2, 64)]), (S, 1, "last_drain", 64)])
    profile((33, 32, 32, 32), ["s.total.slab+1"])
    profile((64, 64, 0, 0), ["s.profile.q-q-0-0"], [(S, 1, "drains", [(1, 64)]), (S, 1, "last_drain", 64)])
    profile((64, 64, 1, 0), ["s.profile.q-q-1-0"])
    profile((64, 0, 0, 64), ["s.profile.q-0-0-q"], [(S, 1, "drains", [(3, 64)]), (S, 1, "last_drain", 64)])
    profile((40, 30, 40, 18), ["s.drain.before_rounds_1_and_2"], [(S, 1, "drains", [(1, 40), (2, 30)]), (S, 1, "last_drain", 58)])
    profile((1, 64, 0, 0), ["s.drain.one_record_then_a_full_round"], [(S, 1, "drains", [(1, 1)]), (S, 1, "last_drain", 64)])
    profile((63, 1, 1, 63), ["s.drain.full_buffer_mid_tile", "s.drain.last.stage"], [(S, 1, "drains", [(2, 64)]), (S, 1, "last_drain", 64)])
    profile((63, 1, 1, 62), ["s.drain.last.stage-1"], [(S, 1, "drains", [(2, 64)]), (S, 1, "last_drain", 63)])
    profile((64, 64, 64, 64), ["s.beyond_slab.without_overflow"], [(S, 1, "beyond_slab", 128)])
    profile((97, 96, 95, 0), ["s.beyond_slab.with_overflow", "t.count.queue+1", "t.count.queue", "t.count.queue-1",
                              "t.past_the_stage_buffer"],
            [(S, 1, "beyond_slab", 160), (T2, 5, "direct_slab", 32), (T2, 6, "direct_slab", 31), (T2, 5, "second_pass", True)])
    # ---- the profiles at the thresholds once more, packed into the fewest lanes from lane 0 and up to lane 63 (the queue
    # then fills slot by slot from few lanes, a lane's sixteen records take sixteen consecutive ranks)
    for prof in ((64, 0, 0, 0), (65, 0, 0, 0), (32, 32, 32, 32), (33, 32, 32, 32), (63, 1, 1, 63), (40, 30, 40, 18), (64, 64, 0, 0)):
        for how in ("packed0", "packed63"):
            profile(prof, [], how=how, behind=False)
    # ---- placements, at a count the staged walk keeps (and, packed, at the queue's edge of the two-launch path)
    for how, cnt, cls in (("packed0", 48, ["p.packed_lane0"]), ("packed63", 48, ["p.packed_lane63"]), ("packed0", 64, ["p.packed_lane0"]),
                          ("packed63", 96, ["p.packed_lane63@two_launch"]), ("slot0", 37, ["p.slot0"]), ("slot15", 37, ["p.slot15"]),
                          ("slot15", 64, ["p.full_ballot15"]), ("slot0", 64, ["p.slot0"]), ("ends", 32, ["p.ends"]), ("ends", 7, ["p.ends"])):
        # rounds 1 and 2 of a tile whose round 0 holds the start and three signatures
        prof = (3, cnt, min(cnt, 128 - 3 - cnt), 0)
        q = rounds_at(0, (3,)) + rounds_at(1, prof[1:3], how) + [TILE + 5]
        exp = [(S, 0, "rounds", list(prof)), (S, 0, "dense", cnt > 64), (T2, 1, "total", cnt), (T2, 1, "dense", cnt > 96)]
        add("place-%s-%d" % (how, cnt), "placement", TILE + 9, q, [0, 700], cls, exp)
    # ---- alignment starts
    sparse = (5, 9, 4, 7)
    add("starts-none-for-two-tiles", "starts", 3 * TILE, rounds_at(0, (2, 3, 1, 0)) + rounds_at(4, sparse) + rounds_at(8, sparse, "slot0"),
        [0], ["a.none.began_one_tile_earlier", "a.none.began_two_tiles_earlier"],
        [(S, 1, "prec", 25), (S, 2, "prec", 25), (S, 2, "since_start", 2), (T2, 2, "since_start", 2)])
    add("starts-only-at-op0", "starts", 2 * TILE + 100, rounds_at(0, sparse) + rounds_at(4, (20, 6, 6, 6), "packed0") + [2 * TILE + 99],
        [0, TILE, 2 * TILE], ["a.only_at_op0"], [(S, 1, "own", 16), (S, 1, "prec", 0), (T2, 4, "own", 16), (T2, 4, "total", 20)])
    # one start in round 1, lane 20, slot 7 of the tile (tile 1 of three), signatures all around it
    p0 = TILE + ROUND + 20 * 16 + 7
    around = [p0 - 5, p0 - 2, p0 + 1, p0 + 6,                       # same lane, before and after
              TILE + ROUND + 3 * 16 + 9, TILE + ROUND + 19 * 16 + 15, TILE + ROUND + 21 * 16, TILE + ROUND + 63 * 16 + 15,
              TILE + 100, TILE + 1023, TILE + 2 * ROUND, TILE + 3 * ROUND + 1000]
    add("starts-one-mid-lane", "starts", 2 * TILE + 300, [50, 3000] + around + [2 * TILE + 299], [0, p0],
        ["a.single." + t for t in ("lane_before", "lane_after", "lanes_before", "lanes_after")]
        + ["a.single.rounds_before", "a.single.rounds_after"],
        [(S, 1, "prec", 6), (S, 1, "own", 2), (S, 1, "total", 12), (T2, 5, "prec", 4), (T2, 5, "own", 2)])
    # the start op qualifies itself (its record: positions 0 and 0), and so does the op in front of a start
    add("starts-on-qualifying-ops", "starts", TILE + 50, [0, 99, 100, 101, 1024, 2047, 2048, 2500, 2501, TILE - 1, TILE, TILE + 49],
        [0, 100, 1024, 2048, 2501, TILE], ["a.start_on_a_qualifying_op", "a.qualifying_op_before_a_start"],
        [(S, 0, "start_on_emit", 5), (S, 0, "emit_before_start", 3), (S, 1, "start_on_emit", 1), (S, 1, "emit_before_start", 1)])
    lane = ROUND + 33 * 16
    add("starts-sixteen-in-a-lane", "starts", TILE + 50, [lane - 1, lane, lane + 3, lane + 15, lane + 16, 3000, TILE + 1],
        [0] + list(range(lane, lane + 16)), ["a.sixteen_starts_in_a_lane"], [(S, 0, "starts", 17), (T2, 1, "starts", 16), (T2, 1, "own", 3)])
    for n in (63, 64, 65, 129):
        # n starts in tile 1 (none at its op 0 ... except for the first), every 31st op, and a signature per 50 ops
        st = [TILE + 7 + 31 * i for i in range(n)]
        q = list(range(TILE + 3, 2 * TILE, 50)) + [st[5], st[n - 1], 10, 2 * TILE + 3]
        add("starts-%d-in-a-tile" % n, "starts", 2 * TILE + 20, q, [0] + st, ["a.starts.%d@streaming" % n],
            [(S, 1, "starts", n), (S, 1, "passes", n // 64 + 1)])
        # the same for the one-round tiles of the two-launch path: every 7th op of round 2
        st = [2 * ROUND + 1 + 7 * i for i in range(n)]
        q = list(range(2 * ROUND, 3 * ROUND, 19)) + [st[n - 1], 10, TILE + 3]
        add("starts-%d-in-a-round" % n, "starts", TILE + 20, q, [0] + st, ["a.starts.%d@two_launch" % n],
            [(T2, 2, "starts", n), (T2, 2, "passes", n // 64 + 1)])
    add("starts-every-op-of-a-round", "starts", TILE + 20, rounds_at(1, (64,)) + [5, 3000, TILE + 1],
        [0] + list(range(ROUND, 2 * ROUND)), ["a.every_op_of_a_round_starts"], [(S, 0, "own", 65), (S, 0, "starts", 1025), (T2, 1, "own", 64), (T2, 1, "starts", 1024)])
    # ---- empty alignments: two and three equal offsets inside a tile, at a tile's op 0, in front of a qualifying op
    for kind, prof in (("staged", (9, 7, 8, 5)), ("dense", (100, 100, 100, 100))):
        q = rounds_at(0, prof) + rounds_at(4, prof) + rounds_at(8, prof)
        free = [p for p in range(ROUND + 1, ROUND + 200) if p not in set(q)][:2]
        e2, e3 = q[len(q) // 3 + 2], q[2 * len(q) // 3 + 3]     # qualifying ops of tiles 1 and 2 (not at op 0)
        st = [0, 0, free[0], free[0], free[1], free[1], free[1], e2, e2, e3, e3, e3, TILE, TILE, TILE,
              2 * TILE + 3 * ROUND, 2 * TILE + 3 * ROUND]
        q = [p for p in q if p not in (0, TILE, 2 * TILE + 3 * ROUND)]
        add("empties-" + kind, "empties", 3 * TILE, q, st,
            ["e.%d.%s.%s" % (m, w, kind) for m in (2, 3) for w in ("inside", "op0", "emit")],
            [(S, 0, "dup", True), (S, 1, "dup", True), (S, 2, "dup", True), (S, 0, "dense", kind == "dense")])
    add("empties-at-n-ops", "empties", TILE + 300, rounds_at(0, sparse) + [TILE + 299], [0, 2000, TILE + 300, TILE + 300, TILE + 300],
        ["e.at_n_ops"])
    # ---- the last tile: 1, 15, 16, 17, 1023 or 1025 ops, and the very last op qualifies
    for n in (1, 15, 16, 17, 1023, 1025):
        n_ops = TILE + n
        add("tail-%d" % n, "tail", n_ops, rounds_at(0, sparse) + [n_ops - 1], [0, TILE - 3],
            ["tail.%d" % n] if n != 1025 else ["tail.1025", "tail.1@two_launch"])
    # ---- lengths
    q = rounds_at(0, (6, 5, 7, 4))
    add("length-one-generic-round", "lengths", TILE + 10, q + [TILE + 2], [0, 1500],
        ["len.one_generic_round_beside_three_24bit", "len.generic_round"], overrides={2 * ROUND + 77: (0, 1 << 24), 2 * ROUND + 500: (2, 1 << 24)})
    add("length-2^28-1", "lengths", TILE + 10, q + [TILE + 2], [0, 1500], ["len.2^28-1_qualifies"],
        overrides={ROUND + 300: (1, MAX_LEN), 3 * ROUND + 9: (2, MAX_LEN), 3 * ROUND + 10: (4, MAX_LEN)})
    big = {p: ((0, 7, 8)[i % 3], MAX_LEN - i) for i, p in enumerate(range(40, 40 + 3 * 24, 3))}
    add("length-cursors-wrap", "lengths", 2 * TILE + 10, q + rounds_at(4, sparse) + [2 * TILE + 2], [0, 30], ["len.cursors_wrap"], overrides=big)
    # ---- the finish kernel of the two-launch path: batches of n one-round tiles, an alignment every 1500 ops, the
    # tiles sparse (a few signatures each) except the dense ones (100 > 96)
    def finish(name, n_tiles, dense, shows, sparse_of=lambda t: 2 + (t * 5) % 9, cut=24):
        n_ops = n_tiles * ROUND - cut
        q = []
        for t in range(n_tiles):
            q += rounds_at(t, (100 if t in dense else sparse_of(t),), "even" if t in dense else "spread")
        q = [p for p in q if p < n_ops] + [n_ops - 1]
        exp = [(T2, t, "dense", t in dense) for t in range(n_tiles)]
        add(name, "finish", n_ops, q, [0] + list(range(1500, n_ops, 1500)), shows, exp)

    for n in (1, 3, 4, 5, 15, 16, 17, 33):
        finish("finish-%d-tiles" % n, n, {n // 2} if n >= 3 else set(), ["f.tiles.%d" % n])
    finish("finish-dense-at-fold-edges", 12, {0, 7}, ["f.dense.first_of_a_fold", "f.dense.last_of_a_fold"])
    finish("finish-dense-at-workgroup-edges", 33, {15, 16}, ["f.dense.first_of_a_workgroup", "f.dense.last_of_a_workgroup"], cut=0)
    finish("finish-a-workgroup-all-dense", 33, set(range(16, 32)), ["f.workgroup_all_dense_beside_a_sparse_one", "f.more_dense_tiles_than_workgroups"],
           cut=1000)
    return collections.OrderedDict((c.name, c) for c in out)


CASES = _table()
FAMILIES = ("counts", "placement", "starts", "empties", "tail", "lengths", "finish")
CAPACITY_CASES = ("profile-40-30-40-18", "profile-33-32-32-32", "profile-97-96-95-0")   # staged, dense, past the stage buffer


def family(name):
    return [c for c in CASES.values() if c.family == name]


@functools.lru_cache(maxsize=None)
def case_facts(name, path):
    c = CASES[name]
    return facts(c.cigar, c.aln_off, path)


@functools.lru_cache(maxsize=1)
def combined():
    """All cases as ONE batch, each at an offset that is a multiple of 4096 so that it keeps its tiles (the filler in
    front of the next case belongs to the case's last alignment).  -> dict(cigar, aln_off, ref_start, bases)."""
    rng = np.random.default_rng(20261020)
    cig, off, rs, bases, at = [], [], [], {}, 0
    for c in CASES.values():
        n = len(c.cigar)
        pad = -n % TILE
        bases[c.name] = at
        cig += [c.cigar, (rng.integers(1, 10, size=pad).astype(np.uint32) << 4) | rng.choice(_FILL_OPS[:7], size=pad)]
        off.append(c.aln_off[:-1] + np.uint64(at))
        rs.append(c.ref_start)
        at += n + pad
    out = dict(cigar=np.concatenate(cig), aln_off=np.concatenate(off + [np.array([at], np.uint64)]).astype(np.uint64),
               ref_start=np.concatenate(rs), bases=bases)
    for a in (out["cigar"], out["aln_off"], out["ref_start"]):
        a.setflags(write=False)
    return out


def split_shows(entry):
    cid, _, path = entry.partition("@")
    return cid, ((path,) if path else CLASSES[cid][0])


def check_preconditions(k=None, cases=None):
    """Every case shows what it lists and holds the numbers its name promises; every class of CLASSES is shown on each
    path it applies to; the exemption is the one of EXEMPT and nothing reaches it.  `k`: the constants (default K)."""
    k = k or K
    cases = list((cases or CASES).values())
    shown = set()
    for c in cases:
        F = {p: facts(c.cigar, c.aln_off, p, k) for p in PATHS}
        for entry in c.shows:
            cid, paths = split_shows(entry)
            for p in paths:
                assert p in CLASSES[cid][0], (c.name, entry)
                assert CLASSES[cid][1](F[p], k), "%s does not show %s on the %s path" % (c.name, cid, p)
                shown.add((cid, p))
        for path, tile, attr, value in c.expect:
            got = getattr(F[path].tiles[tile], attr)
            assert got == value, "%s: %s of tile %d on the %s path is %r, not %r" % (c.name, attr, tile, path, got, value)
        for cid in EXEMPT:
            assert not CLASSES[cid][1](F[PATHS[1]], k), (c.name, cid)
    missing = [(cid, p) for cid, (paths, _) in CLASSES.items() for p in paths if (cid, p) not in shown and cid not in EXEMPT]
    assert not missing, missing
    assert list(EXEMPT) == ["t.count.above_slab_without_overflow"] and k["SLAB"] >= k["QUEUE_SMALL"]
    return shown
