"""The device BGZF encoder (svx_bgzf_deflate_dev, svim_asm_amd/csrc/svx_deflate.hip) at the places where a hand-written
DEFLATE encoder breaks — tests/test_gpu_vcf_bgzf.py round-trips natural data; here every input is built for one seam of
the kernel: the 256-position match chunks, the 64-lane parse steps, the block's last bytes (where hash3 reads padding),
the 258 / 32 768 / 4 096 limits, the one-code and no-code distance trees, the switch to a stored block.

Every case goes through `oracle`: zlib inflate with the container's structure, CRC32, ISIZE and EOF member
(tabix_reader.check_bgzf), members of at most 65 536 bytes and never larger than a stored block, the same bytes on a
second call — and, with the tokens read back by tests/deflate_tokens.py, the rules svx_deflate.hip documents: lengths
3-258, distances 1-32 768, no match from before the block's first byte, no 3-byte match farther than 4 096 back.

Inputs that must hold NO accidental match are cut from a de Bruijn sequence B(41, 3) — every 3-byte string over 41 values
exactly once, so a DEFLATE match (3 bytes at least) is impossible in it — with the planted repeats written in byte values
the filler does not use; what the tokens must then be follows from the documented rules alone (longest match, ties to the
smallest distance; the first position whose match the next position does not beat takes its match)."""
import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import deflate_tokens, tabix_reader

pytestmark = pytest.mark.gpu
BLOCK = 65280
TOO_FAR = 4096


def de_bruijn(k, n):
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)
    db(1, 1)
    return seq


_DB = de_bruijn(41, 3)
_DB = bytes(x + 1 for x in _DB + _DB[:2])  # 68 923 bytes of values 1..41: no 3 bytes occur twice, 0 and 42..255 are free


def filler(n, at=0):
    assert at + n <= len(_DB)
    return bytearray(_DB[at:at + n])


def acgt(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def rand(rng, n, values=256):
    return rng.integers(0, values, n).astype(np.uint8).tobytes()


def positioned(tokens):
    """[(position in the block, token)]"""
    out, p = [], 0
    for t in tokens:
        out.append((p, t))
        p += 1 if isinstance(t, int) else t[0]
    return out


def oracle(ctx, data, seen=None):
    """All checks every case gets; returns per member (btype, block dict of deflate_tokens.read, the block's bytes)."""
    blob, sizes = ctx.bgzf_deflate(data)
    assert tabix_reader.check_bgzf(blob, data) == list(sizes)
    ms = tabix_reader.members(blob)[:-1]
    out = []
    for k, (_, size, payload, _, isize) in enumerate(ms):
        block = data[k * BLOCK:(k + 1) * BLOCK]
        assert isize == len(block) and size <= 65536 and size <= len(block) + 31
        blocks, used = deflate_tokens.read(payload)
        assert used == len(payload) and len(blocks) == 1 and blocks[0]["final"] and blocks[0]["btype"] in (0, 2)
        b = blocks[0]
        assert deflate_tokens.replay(blocks) == block
        for p, t in positioned(b["tokens"]):
            if isinstance(t, int):
                continue
            length, dist = t
            assert 3 <= length <= 258, (p, t)
            assert 1 <= dist <= 32768, (p, t)
            assert dist <= p, ("a match from before the block's first byte", p, t)
            assert not (length == 3 and dist > TOO_FAR), ("a 3-byte match farther than 4 096 back", p, t)
        if b["btype"] == 2 and seen is not None:
            seen["ll"] = max(seen.get("ll", 0), max(b["ll_lens"]))
            seen["d"] = max(seen.get("d", 0), max(b["d_lens"]))
            seen["cl"] = max(seen.get("cl", 0), max(b["cl_lens"]))
        out.append((b["btype"], b, block))
    assert ctx.bgzf_deflate(data)[0] == blob  # the same bytes on a second call
    return out


def matches(b):
    return [t for t in b["tokens"] if not isinstance(t, int)]


# ------------------------------------------------------------------------------------------------------ the inputs
# Every input of the module by name, built once: the tests look theirs up, and the launch-split test takes them all.

def plant(buf, at, what):
    buf[at:at + len(what)] = what


def seam_case(dst):
    """A 40-byte repeat whose second copy starts at `dst`, the first match of the block: filler, with a byte that occurs
    nowhere else in front of the copy and another behind it, so the longest match at dst is exactly 40 bytes and no
    match can start or end beside it."""
    src = (dst // 256 - 2) * 256 + 250
    buf = filler(dst + 400)
    plant(buf, dst, buf[src:src + 40])
    buf[dst - 1], buf[dst + 40] = 0xF0, 0xF1
    return bytes(buf), src


def lazy_case(p):
    """Position p has a 4-byte match and p + 1 a 20-byte match: A = u t0 t1 t2 v at a1, B = t0 t1 t2 + 17 filler bytes at
    b1 < a1, and u t0 t1 t2 + B's 17 bytes at p."""
    b1, a1 = 256 + 250, 2 * 256 + 250
    assert p > a1 + 300
    buf = filler(p + 400)
    t = bytes([0x81, 0x82, 0x83])
    plant(buf, b1, t)
    plant(buf, a1, bytes([0x90]) + t + bytes([0x91]))
    plant(buf, p, bytes([0x90]) + bytes(buf[b1:b1 + 20]))
    buf[p - 1], buf[p + 21] = 0xF0, 0xF1
    return bytes(buf), a1, b1


def too_far_case(dist, length):
    """Thirty strings of `length` bytes (values the filler does not use, each string its own) that recur once, `dist`
    bytes on, the bytes before and behind the two copies different."""
    buf = filler(3 * 4200)
    sites = []
    for k in range(30):
        a = 300 + 131 * k
        while buf[a - 1] == buf[a + dist - 1] or buf[a + length] == buf[a + dist + length]:
            a += 1
        s = bytes([0x80 + k, 0xB0 + k, 0xD0 + k, 0x40 + k][:length])
        plant(buf, a, s)
        plant(buf, a + dist, s)
        sites.append((a + dist, s))
    return bytes(buf), sites


def tail_case(n, back, keep):
    """A block of n bytes that ends with the first `keep` bytes of a 3-byte string seen about `back` bytes earlier, where
    a zero byte follows it: a finder that compared into the zero padding behind the block would find one byte more.
    Returns the block and the distance between the two."""
    buf = filler(n)
    s = bytes([0x81, 0x82, 0x83])
    a = n - keep - back
    while buf[a - 1] == buf[n - keep - 1]:
        a += 1
    plant(buf, a, s + b"\x00")
    plant(buf, n - keep, s[:keep])
    return bytes(buf), n - keep - a


def build_inputs():
    rng = np.random.default_rng(2024)
    I = {}
    for n in SIZES:
        I["size_acgt_%d" % n] = acgt(rng, n)
        I["size_zero_%d" % n] = bytes(n)
    for n, back in TAIL_BACK.items():
        I["tail3_%d" % n] = tail_case(n, back, 3)[0]
        I["tail2_%d" % n] = tail_case(n, back, 2)[0]
    for k, r, where in RUNS:
        n = 258 * k + r
        room = BLOCK - n
        if where == "alone":
            I["run_%d_%d_alone" % (k, r)] = b"G" * n
        elif where == "middle":
            pre = min(1000, room // 2)
            I["run_%d_%d_middle" % (k, r)] = rand(rng, pre, 16) + b"G" * n + rand(rng, min(500, room - pre), 16)
        else:
            I["run_%d_%d_end" % (k, r)] = rand(rng, room, 16) + b"G" * n
    once = rng.permutation(256).astype(np.uint8).tobytes()
    I["distinct256"] = once
    I["distinct256_after_one"] = once[77:78] + once
    I["no_match_filler"] = bytes(filler(20000, 1234))
    for p in PERIODS:
        unit = rand(rng, p)
        I["period_%d" % p] = (unit * (3 + 131 // p))[:2 * p + 131]
    for dist, length in ((4096, 3), (4097, 3), (4097, 4)):
        I["too_far_%d_%d" % (dist, length)] = too_far_case(dist, length)[0]
    for dst in SEAMS:
        I["seam_%d" % dst] = seam_case(dst)[0]
    for p in LAZY:
        I["lazy_%d" % p] = lazy_case(p)[0]
    I["cut_at_block_end"] = seam_case(1990)[0][:2000]
    # the ring of earlier positions per bucket: six later chunks hold the same 3 bytes, only the oldest the long match
    buf = filler(9 * 256)
    t = bytes([0x81, 0x82, 0x83])
    plant(buf, 100, t)
    for c in range(1, 7):
        plant(buf, c * 256 + 100, t + bytes([0x90 + c]))
    plant(buf, 8 * 256 + 100, buf[100:130])
    I["bucket_ring"] = bytes(buf)
    noise = rand(rng, BLOCK)
    for k in STORED_SWEEP:
        I["stored_switch_%d" % k] = b"A" * k + noise[:BLOCK - k]
    # 24 byte values with Fibonacci-proportional probabilities; 200 byte values once each under one dominant value
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    w = np.array(fib, float)
    I["skewed_fibonacci"] = rng.choice(rng.permutation(256)[:24].astype(np.uint8), BLOCK, p=w / w.sum()).tobytes()
    dom = np.full(BLOCK, 0x41, np.uint8)
    dom[rng.choice(BLOCK, 200, replace=False)] = np.delete(np.arange(256), 0x41)[:200].astype(np.uint8)
    I["skewed_singletons"] = dom.tobytes()
    return I


TAIL_BACK = {1000: 897, BLOCK: 2000}
SIZES = [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 65279, 65280, 65281, 2 * BLOCK - 1, 2 * BLOCK + 1]
RUNS = [(k, r, where) for k in (1, 2, 253) for r in range(5) for where in ("alone", "middle", "end")]
PERIODS = [1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 32767, 32768, 32769]
SEAMS = [3 * 256 + r for r in (250, 255, 256, 257)] + [3 * 256 + 64 + r for r in (60, 63, 64, 65)]
LAZY = [5 * 256 + 255, 5 * 256 + 63, 5 * 256 + 127]
STORED_SWEEP = list(range(0, 4001, 200))
INPUTS = build_inputs()
assert all(0 < len(v) <= 200_000 for v in INPUTS.values())


# ------------------------------------------------------------------------------------------------------- the tests

@pytest.mark.parametrize("n", SIZES)
def test_block_sizes(svx_ctx, n):
    """1-4 bytes; 63-65 (a parse step); 255-257, 511-513 (match chunks); 1023-1025 (CRC pieces); one and two blocks +- 1."""
    for fill in ("acgt", "zero"):
        got = oracle(svx_ctx, INPUTS["size_%s_%d" % (fill, n)])
        assert len(got) == (n + BLOCK - 1) // BLOCK
        if fill == "zero" and n >= 300:
            # a run of one byte: a literal, then matches at distance 1, 258 bytes each but for the last
            for _, b, block in got:
                if len(block) < 300:
                    continue
                assert b["btype"] == 2 and b["tokens"][0] == 0
                assert matches(b).count((258, 1)) == (len(block) - 1) // 258 and all(t[1] == 1 for t in matches(b))


@pytest.mark.parametrize("n", sorted(TAIL_BACK))
def test_block_tail_is_not_matched_from_padding(svx_ctx, n):
    """The block's last 3 / 2 bytes repeat a string that a zero byte followed: the last three are one 3-byte match (or
    three literals), never longer; the last two are literals — positions whose hash3 would read padding have no match."""
    (_, b, block), = oracle(svx_ctx, INPUTS["tail3_%d" % n])
    back = tail_case(n, TAIL_BACK[n], 3)[1]
    assert b["tokens"][-1] == (3, back) or b["tokens"][-3:] == [0x81, 0x82, 0x83]
    (_, b, block), = oracle(svx_ctx, INPUTS["tail2_%d" % n])
    assert b["tokens"][-2:] == [0x81, 0x82]


@pytest.mark.parametrize("k,r", [(k, r) for k in (1, 2, 253) for r in range(5)])
def test_runs_of_258k_plus_r(svx_ctx, k, r):
    """A run of 258 k + r equal bytes alone, between random bytes (of 16 values, none the run's, so that the block stays
    a dynamic one) and behind 65 280 - run of them at the block's end: behind its first byte every
    position's longest match is min(258, what is left) at distance 1, so the run is one literal, (run - 1) // 258 matches
    of 258 and the rest.  Alone, distance code 0 is the only one used: the tree carries a second 1-bit code on code 1."""
    n = 258 * k + r
    for where in ("alone", "middle", "end"):
        (_, b, block), = oracle(svx_ctx, INPUTS["run_%d_%d_%s" % (k, r, where)])
        assert b["btype"] == 2
        at = block.index(b"G" * n)
        inside = [t for p, t in positioned(b["tokens"]) if at <= p < at + n]
        assert inside[0] == ord("G") and inside.count((258, 1)) == (n - 1) // 258, (where, inside[:4], len(inside))
        assert all(isinstance(t, int) or t[1] == 1 for t in inside)
        if where == "alone":
            assert b["hdist"] == 2 and b["d_lens"] == [1, 1]


def test_no_matches_at_all(svx_ctx):
    """Every byte value once: no match is possible.  (Its 256 literals of 8 bits and the header exceed a stored block,
    so that is what the member must be.)  The same with no repeated 3 bytes over 41 values, which does compress: all
    literals, every literal's code used, and the unused distance tree still carries its two 1-bit codes (HDIST 2)."""
    for name in ("distinct256", "distinct256_after_one"):
        (btype, b, block), = oracle(svx_ctx, INPUTS[name])
        assert not matches(b)
        if btype == 2:
            assert b["hdist"] == 2 and b["d_lens"] == [1, 1] and all(b["ll_lens"][x] for x in set(block))
    (btype, b, block), = oracle(svx_ctx, INPUTS["no_match_filler"])
    assert btype == 2 and not matches(b) and b["hdist"] == 2 and b["d_lens"] == [1, 1] and b["hlit"] == 257
    assert [x for x in range(257) if b["ll_lens"][x]] == sorted(set(block)) + [256]


@pytest.mark.parametrize("p", PERIODS)
def test_periodic(svx_ctx, p):
    """Random bytes of period p, two periods and a tail: a distance of exactly 32 768 is used when that is the period;
    one byte more and no match reaches back (the generic distance rule) — and the block still round-trips."""
    got = oracle(svx_ctx, INPUTS["period_%d" % p])
    dists = {t[1] for _, b, _ in got for t in matches(b)}
    if p <= 32768:
        assert p in dists
    if p == 32768:
        assert max(dists) == 32768
    if p == 32769:
        assert all(d <= 32768 for d in dists)


def test_too_far(svx_ctx):
    """3 bytes that recur once 4 096 back may be a match (and some of the thirty are: the limit is inclusive); 4 097
    back they are three literals; 4 bytes 4 097 back may be a match again."""
    for dist, length in ((4096, 3), (4097, 3), (4097, 4)):
        (_, b, block), = oracle(svx_ctx, INPUTS["too_far_%d_%d" % (dist, length)])
        at = dict(positioned(b["tokens"]))
        _, sites = too_far_case(dist, length)
        n_match = 0
        for q, s in sites:
            if at.get(q) == (length, dist):
                n_match += 1
            else:
                assert [at.get(q + j) for j in range(length)] == list(s), (dist, length, q)
        print("recurrence of %d bytes %d back: %d of %d sites are matches" % (length, dist, n_match, len(sites)))
        assert (n_match == 0) if (dist, length) == (4097, 3) else (n_match > 0)
        assert len(matches(b)) == n_match


@pytest.mark.parametrize("dst", SEAMS)
def test_repeat_starting_on_a_chunk_or_step_seam(svx_ctx, dst):
    """A 40-byte repeat whose second copy starts at 250 / 255 / 256 / 257 of a 256-position chunk, or at 60 / 63 / 64 / 65
    of a 64-lane parse step (steps start at the chunk's first position while everything before is a literal): the block's
    only match, exactly there."""
    data, src = seam_case(dst)
    (_, b, _), = oracle(svx_ctx, INPUTS["seam_%d" % dst])
    assert b["tokens"][:dst] == list(data[:dst]) and b["tokens"][dst] == (40, dst - src)
    assert matches(b) == [(40, dst - src)]


@pytest.mark.parametrize("p", LAZY)
def test_lazy_decision_on_a_seam(svx_ctx, p):
    """p has a 4-byte match and p + 1 a 20-byte one, p the last position of a chunk / of a parse step: p is a literal."""
    data, a1, b1 = lazy_case(p)
    (_, b, _), = oracle(svx_ctx, INPUTS["lazy_%d" % p])
    at = dict(positioned(b["tokens"]))
    assert at.get(p) == 0x90 and at.get(p + 1) == (20, p + 1 - b1)
    assert matches(b) == [(3, a1 + 1 - b1), (20, p + 1 - b1)]


def test_match_is_cut_at_the_block_end(svx_ctx):
    """The 40-byte repeat with only 10 bytes left in the block."""
    _, src = seam_case(1990)
    (_, b, _), = oracle(svx_ctx, INPUTS["cut_at_block_end"])
    assert matches(b) == [(10, 1990 - src)] and b["tokens"][-1] == (10, 1990 - src)


def test_bucket_ring_round_trips(svx_ctx):
    """More than four later occurrences of the 3 bytes in other chunks than the long match's: only the oracle."""
    oracle(svx_ctx, INPUTS["bucket_ring"])


def test_stored_switch(svx_ctx):
    """k bytes of "A" in front of 65 280 - k random ones, k = 0, 200, ... 4 000 (zlib level 6 changes from stored to
    deflated inside this range too: between 0 and 200): both kinds of member occur, none larger than a stored one; the
    all-random block is stored."""
    kinds = []
    for k in STORED_SWEEP:
        (btype, b, block), = oracle(svx_ctx, INPUTS["stored_switch_%d" % k])
        kinds.append(btype)
    print("stored-switch sweep: " + ", ".join("%d:%s" % (k, "stored" if t == 0 else "dynamic") for k, t in zip(STORED_SWEEP, kinds)))
    assert set(kinds) == {0, 2}
    assert kinds[0] == 0


def test_skewed_literals(svx_ctx):
    """Literal statistics that push the code lengths up; whether 15 bits are reached depends on what the LZ77 leaves, so
    the limiter itself is asserted on the CPU (tests/test_deflate_huff.py) and this prints what the device came to."""
    for name in ("skewed_fibonacci", "skewed_singletons"):
        seen = {}
        (btype, b, _), = oracle(svx_ctx, INPUTS[name], seen)
        assert btype == 2
        print("%s: longest literal/length code %d, distance code %d, code-length code %d bits"
              % (name, seen["ll"], seen["d"], seen["cl"]))


def test_launch_split(svx_ctx):
    """Every input of this module in one stream: the same bytes from one launch, from a launch per block
    (svx_bgzf_deflate_set_slice(1)) and from a call per 65 280-byte piece."""
    data = b"".join(INPUTS[k] for k in sorted(INPUTS))
    seen = {}
    oracle(svx_ctx, data, seen)
    print("all inputs, %d blocks: longest literal/length code %d, distance code %d, code-length code %d bits"
          % ((len(data) + BLOCK - 1) // BLOCK, seen["ll"], seen["d"], seen["cl"]))
    blob = svx_ctx.bgzf_deflate(data)[0]
    lib = _lib.load()
    was = lib.svx_bgzf_deflate_set_slice(1)
    try:
        assert svx_ctx.bgzf_deflate(data)[0] == blob
    finally:
        lib.svx_bgzf_deflate_set_slice(was)
    pieces = [svx_ctx.bgzf_deflate(data[k:k + BLOCK])[0] for k in range(0, len(data), BLOCK)]
    assert all(p.endswith(tabix_reader.EOF_MEMBER) for p in pieces)
    assert b"".join(p[:-28] for p in pieces) + tabix_reader.EOF_MEMBER == blob
