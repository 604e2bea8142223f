"""A DEFLATE (RFC 1951) bit writer for tests, written from the RFC alone — it imports NOTHING from svim_asm_amd, so a
stream it writes is not the product's own idea of the format.  Test infrastructure only (like spec_bam_writer.py).

It writes what zlib's and libdeflate's compressors never do — an end-of-block code among the shortest, codes of 15 bits,
a literal/length code that holds only end-of-block, one or no distance codes, length 258 spelled as code 284 with 31
extra bits, code-length runs across the HLIT / HDIST boundary, 16 straight after 17 / 18, HLIT / HDIST / HCLEN larger than
needed, empty blocks of every type, bytes behind the final block — and, on request, streams that break the format in one
chosen way, each with the bytes a lenient decoder would produce, so that a test can hand over a CONSISTENT ISIZE / CRC32
and only a structural check can refuse the member.

A stream is a list of blocks; a block is a dict:
    kind     "stored" | "fixed" | "dynamic" | "type3"
    final    bool (default False; encode() does not set it for you)
    tokens   literals (int 0..255) and matches (length, distance); and for malformed streams
             ("ll", sym)           the literal/length code of `sym`, nothing else (produces no bytes)
             ("match_d", length, dsym)  a length, then the distance code of `dsym` with no extra bits (no bytes)
             ("bits", value, n)    n raw bits, first bit = value's bit 0
             ("lenient", token)    nothing written; the bytes `token` would produce (what a lenient decoder makes of the
                                   raw bits in front of it)
stored:   len (LEN written; default the number of bytes), nlen (default LEN ^ 0xFFFF)
dynamic:  ll_lens / d_lens  explicit code lengths (else Huffman lengths of the block's symbol counts, `limit` bits at most,
                            default 15); hlit / hdist: the counts written (257..288 / 1..32; default: as few as hold every
                            code); rle: how the code lengths are run-length coded — "zlib" (each alphabet on its own, what
                            zlib's deflate does), "cross" (one sequence over both alphabets: runs cross the boundary),
                            "zero16" (zero runs as 17 followed by 16s), "none" (every length spelled out) — or cl_syms, an
                            explicit list of (code-length symbol, extra value); cl_lens: the code-length code's lengths
                            (19, by symbol; default Huffman, 7 bits at most); hclen: the count written (4..19)
          eob (default True): write the end-of-block code
all coded blocks: len258 "285" (default) or "284": how a match of length 258 is spelled
"""
import struct
import zlib

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8   # RFC 1951 §3.2.6, all 288 symbols
FIXED_D = [5] * 32                                      # codes 30 / 31 exist in the fixed code, never valid in a stream


def len_code(length, spell284=False):
    """(symbol, extra value, extra bits) of a match length 3..258."""
    assert 3 <= length <= 258
    if length == 258 and spell284:
        return 284, 31, 5
    if length == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, length - LEN_BASE[k], LEN_EXTRA[k]


def dist_code(dist):
    assert 1 <= dist <= 32768
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, dist - DIST_BASE[k], DIST_EXTRA[k]


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):  # LSB first (§3.1.1)
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):  # Huffman codes go most significant bit first
        self.bits(int(format(code, "0%db" % length)[::-1], 2) if length else 0, length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    @property
    def pos(self):
        return len(self.out) * 8 + self.n

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """§3.2.2: the code of every symbol with a non-zero length (over-subscribed sets get codes anyway: a malformed stream
    still needs bits to write)."""
    max_len = max(lens) if lens else 0
    count = [0] * (max_len + 2)
    for l in lens:
        if l:
            count[l] += 1
    code, nxt = 0, [0] * (max_len + 2)
    for bits in range(1, max_len + 1):
        code = (code + count[bits - 1]) << 1 if bits > 1 else 0
        nxt[bits] = code
    codes = [None] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return codes


def kraft(lens):
    """sum 2^-l scaled by 2^15: 32768 complete, less incomplete, more over-subscribed."""
    return sum(1 << (15 - l) for l in lens if l)


def huffman_lengths(freqs, limit):
    """Length-limited Huffman code lengths (package-merge).  One used symbol: length 1; none: all 0."""
    used = sorted((f, s) for s, f in enumerate(freqs) if f > 0)
    lens = [0] * len(freqs)
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0][1]] = 1
        return lens
    assert len(used) <= (1 << limit)
    leaves = [(f, (s,)) for f, s in used]
    cur = list(leaves)
    for _ in range(limit - 1):
        pk = [(cur[k][0] + cur[k + 1][0], cur[k][1] + cur[k + 1][1]) for k in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda x: x[0])
    for _, ss in cur[:2 * len(used) - 2]:
        for s in ss:
            lens[s] += 1
    return lens


def chain_lengths(n_top):
    """A complete code of n_top + 1 symbols that reaches 15 bits: lengths 1, 2, ..., 14, 15, 15 (n_top = 15)."""
    return list(range(1, n_top + 1)) + [n_top]


def rle_lengths(seq, mode):
    """Code-length symbols (sym, extra) for the sequence `seq`."""
    out = []
    i = 0
    while i < len(seq):
        v = seq[i]
        run = 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if mode == "none":
            out.extend((v, 0) for _ in range(run))
        elif v == 0 and mode == "zero16" and run >= 6:
            out.append((17, 0))                       # three zeros
            left = run - 3
            while left >= 3:                          # then 16: repeat the previous length — which is 0 after a 17
                k = min(left, 6)
                out.append((16, k - 3))
                left -= k
            out.extend((0, 0) for _ in range(left))
        elif v == 0 and run >= 3:
            left = run
            while left >= 11:
                k = min(left, 138)
                out.append((18, k - 11))
                left -= k
            if left >= 3:
                out.append((17, left - 3))
                left = 0
            out.extend((0, 0) for _ in range(left))
        elif v != 0 and run >= 4:
            out.append((v, 0))
            left = run - 1
            while left >= 3:
                k = min(left, 6)
                out.append((16, k - 3))
                left -= k
            out.extend((v, 0) for _ in range(left))
        else:
            out.extend((v, 0) for _ in range(run))
        i += run
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def _symbols(tokens, len258):
    """literal/length and distance symbol counts of a token list (end-of-block not included)."""
    ll, d = [0] * 288, [0] * 32
    for t in tokens:
        if isinstance(t, int):
            ll[t] += 1
        elif t[0] == "ll":
            ll[t[1]] += 1
        elif t[0] == "match_d":
            ll[len_code(t[1], len258 == "284")[0]] += 1
            d[t[2]] += 1
        elif t[0] in ("bits", "lenient"):
            pass
        else:
            ll[len_code(t[0], len258 == "284")[0]] += 1
            d[dist_code(t[1])[0]] += 1
    return ll, d


def apply_tokens(tokens, out):
    """The bytes a decoder produces for `tokens` behind `out` (a distance before the start of the output reads zeros —
    what a lenient decoder with an all-zero window would do)."""
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t[0] == "lenient":
            apply_tokens([t[1]], out)
        elif isinstance(t[0], int):
            length, dist = t
            start = len(out) - dist
            if start >= 0 and dist >= length:
                out += out[start:start + length]
            else:
                for _ in range(length):
                    out.append(out[start] if start >= 0 else 0)
                    start += 1
    return out


def _write_tokens(w, tokens, ll_codes, d_codes, len258, marks):
    for t in tokens:
        if marks is not None:
            marks.append(w.pos)
        if isinstance(t, int):
            w.code(*ll_codes[t])
        elif t[0] == "ll":
            w.code(*ll_codes[t[1]])
        elif t[0] == "bits":
            w.bits(t[1], t[2])
        elif t[0] == "lenient":
            pass
        elif t[0] == "match_d":
            s, e, n = len_code(t[1], len258 == "284")
            w.code(*ll_codes[s])
            w.bits(e, n)
            w.code(*d_codes[t[2]])
        else:
            s, e, n = len_code(t[0], len258 == "284")
            w.code(*ll_codes[s])
            w.bits(e, n)
            s, e, n = dist_code(t[1])
            w.code(*d_codes[s])
            w.bits(e, n)


def _dynamic_header(w, b, ll_lens, d_lens):
    hlit = b.get("hlit") or max(257, max((i + 1 for i, l in enumerate(ll_lens) if l), default=0))
    hdist = b.get("hdist") or max(1, max((i + 1 for i, l in enumerate(d_lens) if l), default=0))
    seq_ll = (list(ll_lens) + [0] * 288)[:hlit]
    seq_d = (list(d_lens) + [0] * 32)[:hdist]
    if b.get("cl_syms") is not None:
        cl = list(b["cl_syms"])
    else:
        mode = b.get("rle", "zlib")
        if mode == "zlib":
            cl = rle_lengths(seq_ll, "zlib") + rle_lengths(seq_d, "zlib")
        else:
            cl = rle_lengths(seq_ll + seq_d, "zlib" if mode == "cross" else mode)
    cl_lens = b.get("cl_lens")
    if cl_lens is None:
        freq = [0] * 19
        for s, _ in cl:
            freq[s] += 1
        if sum(1 for f in freq if f) < 2:  # the code-length code must be complete: give it a second symbol
            freq[0 if not freq[0] else 1] += 1
        cl_lens = huffman_lengths(freq, 7)
    hclen = b.get("hclen") or max(4, max((k + 1 for k, s in enumerate(CL_ORDER) if cl_lens[s]), default=0))
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lens[CL_ORDER[k]], 3)
    cl_codes = canonical(cl_lens)
    for s, e in cl:
        w.code(*cl_codes[s])
        if s in CL_EXTRA:
            w.bits(e, CL_EXTRA[s])


def encode(blocks, trailing=b"", marks=None):
    """(payload, bytes a lenient decoder produces).  `marks`: a list that receives the bit position of every token and of
    every end-of-block code (symbol boundaries, for truncation tests)."""
    w = BitWriter()
    out = bytearray()
    for b in blocks:
        kind = b["kind"]
        tokens = list(b.get("tokens", ()))
        w.bits(1 if b.get("final") else 0, 1)
        if kind == "stored":
            data = bytes(tokens)
            w.bits(0, 2)
            w.align()
            ln = b.get("len", len(data))
            w.bits(ln, 16)
            w.bits(b.get("nlen", ln ^ 0xFFFF), 16)
            for x in data:
                w.bits(x, 8)
            out += data
            continue
        if kind == "type3":
            w.bits(3, 2)
            continue
        len258 = b.get("len258", "285")
        if kind == "fixed":
            w.bits(1, 2)
            ll_lens, d_lens = FIXED_LL, FIXED_D
        else:
            assert kind == "dynamic"
            w.bits(2, 2)
            ll_f, d_f = _symbols(tokens, len258)
            if b.get("eob", True):
                ll_f[256] += 1
            ll_lens = b.get("ll_lens") or huffman_lengths(ll_f[:286], b.get("limit", 15))
            d_lens = b.get("d_lens") if b.get("d_lens") is not None else huffman_lengths(d_f[:30], b.get("limit", 15))
            _dynamic_header(w, b, ll_lens, d_lens)
        ll_codes, d_codes = canonical(ll_lens), canonical(d_lens)
        _write_tokens(w, tokens, ll_codes, d_codes, len258, marks)
        apply_tokens(tokens, out)
        if b.get("eob", True):
            if marks is not None:
                marks.append(w.pos)
            w.code(*ll_codes[256])
    return w.getvalue() + bytes(trailing), bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# The seeded corpus: members of a BGZF file's shape (at most 65 536 bytes in and out) in every category above.

OK, BAD, SIZE, CRC = 0, 1, 2, 3
TRUNC = -1  # a stream cut short: refused (status 4, or 1 / 2 where the zero bits behind the cut decode as such), not pinned


class Member(tuple):
    """(payload, expected bytes or None for a malformed stream, isize, crc, expected status) and the category's name."""
    __slots__ = ()
    name = property(lambda self: self[5])

    def __new__(cls, payload, expect, isize, crc, status, name):
        return tuple.__new__(cls, (payload, expect, isize, crc, status, name))

    payload = property(lambda self: self[0])
    expect = property(lambda self: self[1])
    isize = property(lambda self: self[2])
    crc = property(lambda self: self[3])
    status = property(lambda self: self[4])


def crc32(b):
    return zlib.crc32(b) & 0xFFFFFFFF


def _valid(name, blocks, trailing=b""):
    p, out = encode(blocks, trailing)
    return Member(p, out, len(out), crc32(out), OK, name)


def _bad(name, blocks, trailing=b""):
    p, out = encode(blocks, trailing)  # the lenient decoder's bytes: a consistent trailer, only the structure is wrong
    return Member(p, None, len(out), crc32(out), BAD, name)


def _lits(r, n, alphabet=None):
    return [r.choice(alphabet) if alphabet else r.randrange(256) for _ in range(n)]


def _tokens(r, n, have, lsyms=None, dsyms=None, p_match=0.4, alphabet=None, max_len=258, budget=60000):
    """Up to n random tokens behind `have` bytes of output, the output kept within `budget` bytes; lengths / distances only
    of the symbols lsyms / dsyms when given."""
    toks = []
    for _ in range(n):
        if have >= budget:
            break
        max_len = min(max_len, budget - have)
        if have >= 1 and max_len >= 3 and r.random() < p_match:
            ds = [s for s in (dsyms if dsyms is not None else range(30)) if DIST_BASE[s] <= have]
            ls = [s for s in (lsyms if lsyms is not None else range(257, 286)) if LEN_BASE[s - 257] <= max_len]
            if ds and ls:
                s = r.choice(ls)
                length = LEN_BASE[s - 257] + (r.randrange(1 << LEN_EXTRA[s - 257]) if s != 285 else 0)
                length = min(length, max_len, 257 if lsyms is not None and s == 284 else 258)
                d = r.choice(ds)
                dist = min(DIST_BASE[d] + r.randrange(1 << DIST_EXTRA[d]), have)
                if dist_code(dist)[0] != d:
                    dist = DIST_BASE[d]
                if lsyms is not None and len_code(length)[0] not in lsyms:
                    length = LEN_BASE[s - 257]
                toks.append((length, dist))
                have += length
                continue
        toks.append(r.choice(alphabet) if alphabet else r.randrange(256))
        have += 1
    return toks, have


def _edge_block(k, end_at_eob_start=False):
    """A fixed block whose symbols take exactly 256 * k bits behind its header: its end-of-block code ends (or starts) on
    a 256-bit stretch edge of the wave parse's first window."""
    if end_at_eob_start:
        return dict(kind="fixed", tokens=[0x41] * (32 * k))
    return dict(kind="fixed", tokens=[0x41] * (32 * k - 2) + [0xC1])  # 8 (32k - 2) + 9 + 7 = 256 k


def spec_corpus(seed=0):
    """Members of every category, then randomised ones: a list of Member."""
    import random
    r = random.Random(seed)
    M = []
    text = b"chr1\t12345\tsvim_asm.DEL.7\tACGTNNNN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=12400\n"
    seq = [0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88]

    # ---- valid encodings no common compressor writes -------------------------------------------------------------
    # end-of-block among the shortest codes, in every block of the member
    for eob_len, lens in ((1, {256: 1, 65: 2, 67: 3, 71: 3}), (2, {256: 2, 65: 2, 66: 2, 67: 3, 68: 3})):
        ll = [0] * 257
        for s, l in lens.items():
            ll[s] = l
        syms = [s for s in lens if s != 256]
        blocks = [dict(kind="dynamic", ll_lens=ll, d_lens=[0], tokens=_lits(r, n, syms)) for n in (0, 1, 40, 3000, 7)]
        blocks[-1]["final"] = True
        M.append(_valid("eob_shortest_%d" % eob_len, blocks))
    # a literal/length code of end-of-block alone (one 1-bit code), no distance code: empty blocks around real ones
    only_eob = dict(kind="dynamic", ll_lens=[0] * 256 + [1], d_lens=[0], tokens=[])
    M.append(_valid("only_eob", [only_eob, dict(kind="fixed", tokens=list(text)), dict(only_eob, final=True)]))
    M.append(_valid("only_eob_alone", [dict(only_eob, final=True)]))
    # distance codes: a single 1-bit code (every match uses it), none at all
    for dsym in (0, 3, 17, 29):
        toks, have = _tokens(r, 30, 0, dsyms=[], p_match=0)
        more, _ = _tokens(r, 400, max(have, DIST_BASE[dsym] + (1 << DIST_EXTRA[dsym])), dsyms=[dsym], p_match=0.5)
        toks += _lits(r, DIST_BASE[dsym] + (1 << DIST_EXTRA[dsym]) - len(toks)) + more
        d = [0] * (dsym + 1)
        d[dsym] = 1
        M.append(_valid("dist_single_1bit_%d" % dsym, [dict(kind="dynamic", d_lens=d, tokens=toks, final=True)]))
    M.append(_valid("dist_none", [dict(kind="dynamic", d_lens=[0], tokens=_lits(r, 5000, seq), final=True)]))
    M.append(_valid("dist_none_hdist32", [dict(kind="dynamic", d_lens=[0], hdist=30, tokens=_lits(r, 300), final=True)]))
    # length 258 as 284 + 31 extra bits, fixed and dynamic, overlapping and not
    for kind in ("fixed", "dynamic"):
        toks = list(text) + [(258, 1), (258, 3), (258, 70)] + _tokens(r, 2000, 400)[0] + [(258, 258), (258, 259)]
        M.append(_valid("len258_as_284_%s" % kind, [dict(kind=kind, tokens=toks, len258="284", final=True)]))
        M.append(_valid("len258_as_285_%s" % kind, [dict(kind=kind, tokens=toks, final=True)]))
    # code-length runs: 16 straight after 17 / 18 (repeats 0), runs across HLIT / HDIST, every length spelled out
    for rle in ("zero16", "cross", "none"):
        for kind_toks in (_tokens(r, 3000, 0)[0], _lits(r, 2000, seq)):
            M.append(_valid("rle_%s" % rle, [dict(kind="dynamic", rle=rle, hlit=286, hdist=30, tokens=kind_toks, final=True)]))
    ll = [0] * 286
    ll[256], ll[65], ll[66] = 1, 2, 2
    M.append(_valid("rep16_after_18", [dict(kind="dynamic", ll_lens=ll, d_lens=[0] * 30, hlit=286, hdist=30, tokens=_lits(r, 999, [65, 66]),
                                            # 65 zeros, 2, 2; 189 zeros as 18 (138) 16 (6) 17 (10) 16 x 6 (35); end-of-block 1;
                                            # 59 zeros across the boundary
                                            cl_syms=[(18, 65 - 11), (2, 0), (2, 0), (18, 127), (16, 3), (17, 7)] + [(16, 3)] * 5 +
                                                    [(16, 2), (1, 0), (18, 59 - 11)],
                                            final=True)]))
    # HCLEN larger than needed, and the smallest valid one (lengths 0, 8 and 7 only: HCLEN 6)
    M.append(_valid("hclen19", [dict(kind="dynamic", hclen=19, tokens=_tokens(r, 1500, 0)[0], final=True)]))
    ll = [8] * 252 + [0] * 4 + [7, 7]
    M.append(_valid("hclen6", [dict(kind="dynamic", ll_lens=ll, d_lens=[0], hclen=6, tokens=_lits(r, 4000, list(range(252))), final=True)]))
    M.append(_valid("hlit_hdist_larger", [dict(kind="dynamic", hlit=288 - 2, hdist=30, tokens=_tokens(r, 2000, 0)[0], final=True)]))
    # distances zlib's deflate never reaches (32 506 .. 32 768)
    base = bytes(_lits(r, 33000))
    far = [(258, 32768), (100, 32767), (3, 32506), (258, 32600), (7, 24577), (40, 32768)]
    M.append(_valid("dist_far_fixed", [dict(kind="stored", tokens=base), dict(kind="fixed", tokens=far, final=True)]))
    M.append(_valid("dist_far_dynamic", [dict(kind="dynamic", tokens=list(base) + far + _tokens(r, 200, 33000)[0], final=True)]))
    # empty stored / fixed / dynamic blocks in the middle of a member
    mid, have = [dict(kind="fixed", tokens=list(text))], len(text)
    for empty in (dict(kind="stored", tokens=[]), dict(kind="fixed", tokens=[]), dict(kind="dynamic", tokens=[]), only_eob):
        toks, have = _tokens(r, 300, have)
        mid += [dict(empty), dict(kind="dynamic", tokens=toks)]
    mid.append(dict(kind="stored", tokens=[], final=True))
    M.append(_valid("empty_blocks_mid", mid))
    M.append(_valid("empty_member_stored", [dict(kind="stored", tokens=[], final=True)]))
    M.append(_valid("empty_member_fixed", [dict(kind="fixed", tokens=[], final=True)]))
    # bytes behind the final block
    for tail in (b"\x00", b"\xff" * 3, bytes(_lits(r, 100))):
        M.append(_valid("trailing_bytes_%d" % len(tail), [dict(kind="dynamic", tokens=_tokens(r, 500, 0)[0], final=True)], tail))
    # stored LEN 0 .. 65 535, stored next to coded blocks
    for ln in (0, 1, 2, 255, 4096, 65531):  # (65 531: 65 536 bytes of input)
        M.append(_valid("stored_len_%d" % ln, [dict(kind="stored", tokens=_lits(r, ln), final=True)]))
    M.append(_valid("stored_mixed", [dict(kind="stored", tokens=_lits(r, 500)), dict(kind="fixed", tokens=_tokens(r, 500, 500)[0]),
                                     dict(kind="stored", tokens=_lits(r, 3)), dict(kind="dynamic", tokens=_tokens(r, 900, 1003)[0]),
                                     dict(kind="stored", tokens=_lits(r, 7000), final=True)]))
    # codes whose decode from a wrong bit never resynchronises: 255 literals of 8 bits, two 9-bit codes (literal 255 and
    # end-of-block); literals < 0x40 never put eight 1 bits in a row, so a stretch started off the byte grid stays off it —
    # the wave parse's sync passes give up and the member goes to the lane parse
    ll = [8] * 255 + [9, 9]
    for n in (4000, 9000, 60000):
        M.append(_valid("never_resync_%d" % n, [dict(kind="dynamic", ll_lens=ll, d_lens=[0], tokens=_lits(r, n, list(range(0x40))), final=True)]))
    M.append(_valid("never_resync_then_fixed", [dict(kind="dynamic", ll_lens=ll, d_lens=[0], tokens=_lits(r, 8000, list(range(0x40)))),
                                                dict(kind="fixed", tokens=_tokens(r, 3000, 8000)[0], final=True)]))
    # 15-bit codes in both alphabets
    for rep in range(3):
        ll_syms = r.sample(range(256), 8) + [256] + r.sample(range(257, 285), 7)
        d_syms = [0, 1, 2, 3] + r.sample(range(4, 30), 12)
        ll, d = [0] * 286, [0] * 30
        for s, l in zip(r.sample(ll_syms, 16), chain_lengths(15)):
            ll[s] = l
        for s, l in zip(r.sample(d_syms, 16), chain_lengths(15)):
            d[s] = l
        lits = [s for s in ll_syms if s < 256]
        toks = [lits[0]] * 4 + _tokens(r, 6000, 4, lsyms=[s for s in ll_syms if s > 256], dsyms=d_syms, alphabet=lits, p_match=0.3)[0]
        out_len = len(apply_tokens(toks, bytearray()))
        if out_len > 65536:
            toks = toks[:len(toks) // 2]
        M.append(_valid("codes_15bit_%d" % rep, [dict(kind="dynamic", ll_lens=ll, d_lens=d, tokens=toks, final=True)]))
    # overlapping copies: distances 1-3 and 63-65 with length 258
    for d0 in (1, 2, 3, 63, 64, 65):
        toks = _lits(r, 70) + [(258, d0)] * 20 + _tokens(r, 200, 70 + 20 * 258)[0] + [(258, d0), (257, d0), (255, d0)]
        for kind in ("fixed", "dynamic"):
            M.append(_valid("overlap_d%d_%s" % (d0, kind), [dict(kind=kind, tokens=toks, final=True)]))
    # blocks ending exactly on 256-bit stretch edges
    for k in (1, 2, 3, 64, 65):
        for at_start in (False, True):
            M.append(_valid("edge_%d_%s" % (k, "eob_start" if at_start else "eob_end"), [_edge_block(k, at_start), _edge_block(k, not at_start),
                                                           dict(kind="fixed", tokens=list(text), final=True)]))

    # ---- valid streams with a wrong trailer ---------------------------------------------------------------------
    for k, m in enumerate([x for x in M if x.status == OK and x.isize > 0][:12]):
        M.append(Member(m.payload, m.expect, m.isize - 1 - (k % 3) * 50 if m.isize > 101 else m.isize - 1, m.crc, SIZE, "isize_short"))
        M.append(Member(m.payload, m.expect, m.isize + 1 + k, m.crc, SIZE, "isize_long"))
        M.append(Member(m.payload, m.expect, m.isize, m.crc ^ (1 << (k % 32)), CRC, "crc_wrong"))
    small = M[0]
    for big in (65537, 70000, 0xFFFFFFFF):
        M.append(Member(small.payload, small.expect, big, small.crc, SIZE, "isize_over_65536"))

    # ---- malformed streams with consistent trailers -------------------------------------------------------------
    toks = list(text) + _tokens(r, 500, len(text))[0]
    # over-subscribed literal/length, distance and code-length codes
    ll = [0] * 256 + [1, 1, 1]
    M.append(_bad("oversubscribed_ll", [dict(kind="dynamic", ll_lens=ll, d_lens=[0], tokens=[], final=True)]))
    M.append(_bad("oversubscribed_d", [dict(kind="dynamic", d_lens=[1, 1, 1], tokens=list(text) + [(5, 3)], final=True)]))
    M.append(_bad("oversubscribed_cl", [dict(kind="dynamic", ll_lens=FIXED_LL[:286], d_lens=[5] * 30, tokens=list(text), final=True,
                                             cl_lens=[2] * 19)]))
    # incomplete codes that never use their missing codes (other than the one-1-bit-code exception)
    ll = [0] * 257
    ll[65], ll[66], ll[256] = 2, 2, 3   # 1/4 + 1/4 + 1/8: incomplete
    M.append(_bad("incomplete_ll", [dict(kind="dynamic", ll_lens=ll, d_lens=[0], tokens=_lits(r, 300, [65, 66]), final=True)]))
    M.append(_bad("incomplete_ll_eob_2bit", [dict(kind="dynamic", ll_lens=[0] * 256 + [2], d_lens=[0], tokens=[], final=True)]))
    d = [2, 2, 0, 0]                     # two 2-bit distance codes
    M.append(_bad("incomplete_d", [dict(kind="dynamic", d_lens=d, tokens=list(text) + [(4, 1), (9, 2)], final=True)]))
    d = [0, 0, 2]                        # ONE code, but of 2 bits
    M.append(_bad("incomplete_d_single_2bit", [dict(kind="dynamic", d_lens=d, tokens=list(text) + [(4, 3)], final=True)]))
    ll = [0] * 257
    for s, l in zip([256] + list(range(65, 79)), range(1, 16)):  # 1, 2, ..., 15 bits: one 15-bit code short of complete
        ll[s] = l
    M.append(_bad("incomplete_ll_15bit", [dict(kind="dynamic", ll_lens=ll, d_lens=[0], tokens=_lits(r, 3000, list(range(65, 79))), final=True)]))
    cl = huffman_lengths([1] * 19, 7)
    cl[CL_ORDER[-1]] = 0                 # one code-length code left out: incomplete code-length code (zlib: must be complete)
    M.append(_bad("incomplete_cl", [dict(kind="dynamic", tokens=list(text), rle="none", cl_lens=cl, final=True)]))
    # no end-of-block code
    ll = [0] * 257
    ll[65], ll[66] = 1, 1
    M.append(_bad("no_eob", [dict(kind="dynamic", ll_lens=ll, d_lens=[0], eob=False, tokens=_lits(r, 100, [65, 66]), final=True)]))
    M.append(_bad("hclen4_no_eob", [dict(kind="dynamic", ll_lens=[0] * 257, d_lens=[0], eob=False, hclen=4, tokens=[], final=True,
                                         cl_syms=[(18, 138 - 11), (18, 119 - 11), (0, 0)], cl_lens=[1] + [0] * 15 + [0, 2, 2])]))
    # HLIT 287 / 288, HDIST 31 / 32
    for hlit in (287, 288):
        M.append(_bad("hlit_%d" % hlit, [dict(kind="dynamic", hlit=hlit, tokens=toks, final=True)]))
    for hdist in (31, 32):
        M.append(_bad("hdist_%d" % hdist, [dict(kind="dynamic", hdist=hdist, tokens=toks, final=True)]))
    # repeat 16 as the first code length; a repeat that runs past HLIT + HDIST
    ll = [0] * 257
    ll[65], ll[256] = 1, 1
    # (65 zeros, 1, 190 zeros, 1: the 257 literal/length lengths)
    M.append(_bad("rep16_first", [dict(kind="dynamic", ll_lens=ll, d_lens=[0], tokens=_lits(r, 10, [65]), final=True,
                                       cl_syms=[(16, 0), (18, 65 - 11 - 3), (1, 0), (18, 127), (18, 41), (1, 0), (0, 0)])]))
    M.append(_bad("rep_past_end", [dict(kind="dynamic", ll_lens=ll, d_lens=[0], tokens=_lits(r, 10, [65]), final=True,
                                        cl_syms=[(18, 65 - 11), (1, 0), (18, 127), (18, 41), (1, 0), (18, 0)])]))
    M.append(_bad("rep_past_end_by_one", [dict(kind="dynamic", ll_lens=ll, d_lens=[0, 0], hdist=2, tokens=_lits(r, 10, [65]), final=True,
                                               cl_syms=[(18, 65 - 11), (1, 0), (18, 127), (18, 41), (1, 0), (17, 0)])]))
    M.append(_bad("rep_past_end_across", [dict(kind="dynamic", ll_lens=ll, d_lens=[0], tokens=_lits(r, 10, [65]), final=True,
                                               cl_syms=[(18, 65 - 11), (1, 0), (18, 127), (18, 40), (16, 0)])]))
    # fixed block: literal/length 286 / 287, distance 30 / 31
    for s in (286, 287):
        M.append(_bad("fixed_ll_%d" % s, [dict(kind="fixed", tokens=list(text) + [("ll", s)] + list(text), final=True)]))
    for s in (30, 31):
        M.append(_bad("fixed_d_%d" % s, [dict(kind="fixed", tokens=list(text) + [("match_d", 10, s)] + list(text), final=True)]))
    # a distance one byte before the start of the output (and in a later block, at the member's start)
    for n in (0, 1, 5, 300):
        M.append(_bad("dist_before_start_%d" % n, [dict(kind="fixed", tokens=_lits(r, n) + [(3, n + 1)], final=True)]))
    M.append(_bad("dist_before_start_later_block", [dict(kind="stored", tokens=_lits(r, 40)),
                                                     dict(kind="dynamic", tokens=_tokens(r, 50, 40)[0] + [(258, 32768)], final=True)]))
    # stored LEN / NLEN mismatch, block type 3
    M.append(_bad("stored_nlen", [dict(kind="stored", tokens=_lits(r, 20), nlen=20 ^ 0xFFFF ^ 0x100, final=True)]))
    M.append(_bad("stored_nlen_len0", [dict(kind="stored", tokens=[], nlen=0, final=True)]))
    M.append(_bad("type3", [dict(kind="fixed", tokens=list(text)), dict(kind="type3", final=True)]))
    M.append(_bad("type3_first", [dict(kind="type3", final=True)]))
    # a single 1-bit distance code whose missing code the stream uses — with the distance lengths spelled as 17 then 16
    # (a decoder that kept the previous length through a 17 would read four 3-bit codes there and accept the stream)
    ll = [0] * 259
    for s in (65, 66, 67, 68, 256):
        ll[s] = 3
    ll[258], ll[69], ll[70] = 3, 3, 3   # eight 3-bit codes; 258 = length 4
    cl_syms = [(18, 65 - 11), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (18, 127), (18, 36), (3, 0), (0, 0),
               (3, 0), (17, 0), (16, 1), (1, 0)]   # distances: 17 (3 zeros), 16 (4 more), then symbol 7 with 1 bit
    lead = _lits(r, 20, [65, 66, 67, 68, 69, 70])
    # the missing code "100": what the four 3-bit codes of a 16 that repeated the 3 would make distance symbol 3 (distance 4)
    M.append(_bad("dist_missing_code_used", [dict(kind="dynamic", ll_lens=ll, d_lens=[0] * 7 + [1], hlit=259, hdist=8, cl_syms=cl_syms,
                                                  tokens=lead + [(4, 13), ("ll", 258), ("bits", 1, 3), ("lenient", (4, 4)), 69, 70],
                                                  final=True)]))

    # ---- streams cut short --------------------------------------------------------------------------------------
    for k in range(4):
        marks = []
        blocks = [dict(kind="fixed", tokens=_tokens(r, 400, 0)[0] + [0xC8, 0x41, 0x41]), dict(kind="fixed", tokens=list(text), final=True)]
        p, out = encode(blocks, marks=marks)
        at = [m for m in marks if m % 8 == 0 and 0 < m < 8 * len(p) - 8]
        cut = at[r.randrange(len(at))] // 8 if k else max(at) // 8
        M.append(Member(p[:cut], None, len(out), crc32(out), TRUNC, "cut_at_symbol"))
    p, out = encode([dict(kind="dynamic", tokens=toks, final=True)])
    for cut in (1, 2, 10, 30):
        M.append(Member(p[:cut], None, len(out), crc32(out), TRUNC, "cut_in_header"))
    p, out = encode([dict(kind="fixed", tokens=list(text)), dict(kind="stored", tokens=_lits(r, 1000), final=True)])
    for back in (1, 500, 1003):
        M.append(Member(p[:len(p) - back], None, len(out), crc32(out), TRUNC, "cut_in_stored"))
    p, out = encode([dict(kind="stored", tokens=_lits(r, 65535), final=True)])  # LEN 65 535, the input cut to 65 536 bytes
    M.append(Member(p[:65536], None, len(out), crc32(out), TRUNC, "cut_in_stored"))
    M.append(Member(b"", None, 0, 0, TRUNC, "cut_empty"))

    # ---- randomised members -----------------------------------------------------------------------------------
    for k in range(160):
        M.append(_valid("random", _random_member(r, k)))
    return M


def _random_member(r, k):
    """Random block splits (blocks of 0, 1, 2, ... symbols and long ones), block types mixed inside one member, random
    code limits, run-length modes, HLIT / HDIST sizes and spellings of length 258; outputs up to 64 KiB."""
    big = k % 8 == 0
    budget = r.choice([65536, 40000, 20000]) if big else r.choice([0, 1, 3, 100, 1000, 5000])
    n_blocks = 1 if k % 5 == 0 else r.randrange(1, 7)
    blocks, have = [], 0
    style = r.randrange(4)
    alphabet = [None, [0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88],
                list(b"ACGT"), list(range(0x20, 0x7F))][style]
    for b in range(n_blocks):
        room = budget - have
        n = r.choice([0, 1, 2, 3, r.randrange(0, 50), r.randrange(0, max(1, room // 3 + 1))])
        kind = r.choice(["stored", "fixed", "dynamic", "dynamic"])
        if kind == "stored":
            n = min(n, room, 65535)
            toks = _lits(r, n, alphabet)
            have += n
            blocks.append(dict(kind="stored", tokens=toks))
            continue
        toks, new_have = _tokens(r, n, have, alphabet=alphabet, p_match=r.choice([0.0, 0.2, 0.5, 0.8]))
        while new_have > budget and toks:  # keep the member within its budget
            toks = toks[:len(toks) // 2]
            new_have = len(apply_tokens(toks, bytearray(have)))
        have = new_have
        blk = dict(kind=kind, tokens=toks, len258=r.choice(["284", "285"]))
        if kind == "dynamic":
            blk.update(limit=r.choice([15, 15, 12, 10, 9]), rle=r.choice(["zlib", "cross", "zero16", "none"]))
            if r.random() < 0.3:
                blk["hlit"] = 286
            if r.random() < 0.3:
                blk["hdist"] = 30
            if r.random() < 0.2:
                blk["hclen"] = 19
        blocks.append(blk)
    blocks[-1]["final"] = True
    return blocks


def corpus_digest(members):
    import hashlib
    h = hashlib.sha256()
    for m in members:
        h.update(struct.pack("<III", len(m.payload), m.isize, m.crc) + m.payload + m.name.encode())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# Compressors of whole payloads in those encodings (spec_bam_writer.write_bam(compress=...)): any bytes in, a valid stream out.

def _runs(payload):
    """A literal per byte, runs of one byte value as that byte and matches at distance 1 (lengths up to 258)."""
    toks, i, n = [], 0, len(payload)
    while i < n:
        j = i + 1
        while j < n and payload[j] == payload[i] and j - i < 1 + 258 * 8:
            j += 1
        toks.append(payload[i])
        left = j - i - 1
        while left >= 3:
            k = min(left, 258)
            toks.append((k, 1))
            left -= k
        toks.extend([payload[i]] * left)
        i = j
    return toks


def _split(items, parts):
    step = max(1, -(-len(items) // parts))
    return [items[k:k + step] for k in range(0, len(items), step)] or [[]]


def compress_short_eob(payload):
    """Dynamic blocks whose end-of-block code is among the shortest, matches as 284 + 31 for length 258."""
    blocks = []
    for toks in _split(_runs(payload), 4):
        ll, _ = _symbols(toks, "284")
        ll[256] = max(ll) * 4 + 1
        blocks.append(dict(kind="dynamic", tokens=toks, ll_lens=huffman_lengths(ll[:286], 15), len258="284"))
    blocks[-1]["final"] = True
    return encode(blocks)[0]


def compress_15bit(payload):
    """Codes that reach 15 bits: the symbols' counts replaced by weights that halve from one symbol to the next."""
    blocks = []
    for toks in _split(_runs(payload), 2):
        ll, d = _symbols(toks, "285")
        ll[256] = 1
        w = [0] * 286
        for rank, s in enumerate(sorted((s for s in range(286) if ll[s]), key=lambda s: -ll[s])):
            w[s] = 1 << max(0, 20 - rank)
        blocks.append(dict(kind="dynamic", tokens=toks, ll_lens=huffman_lengths(w, 15), rle="cross", hclen=19))
    blocks[-1]["final"] = True
    return encode(blocks)[0]


def compress_stored(payload):
    """Stored blocks of uneven sizes, an empty one in the middle, a fixed block at the end."""
    cut = [0, len(payload) // 3, len(payload) // 3, len(payload) * 3 // 4, len(payload)]
    blocks = [dict(kind="stored", tokens=list(payload[a:b])) for a, b in zip(cut, cut[1:])]
    blocks.append(dict(kind="fixed", tokens=[], final=True))
    return encode(blocks)[0]


def compress_never_resync(payload):
    """Literals only, 255 of them at 8 bits and literal 255 + end-of-block at 9: a stretch decoded from a wrong bit stays
    on its wrong grid for as long as no eight 1 bits come by."""
    ll = [8] * 255 + [9, 9]
    return encode([dict(kind="dynamic", tokens=list(payload), ll_lens=ll, d_lens=[0], final=True)], b"\x00\x01")[0]


COMPRESSORS = (compress_short_eob, compress_15bit, compress_stored, compress_never_resync)


def compress_cycling():
    """A compress= callable that hands the members to COMPRESSORS in turn."""
    state = [0]

    def compress(payload):
        f = COMPRESSORS[state[0] % len(COMPRESSORS)]
        state[0] += 1
        return f(payload)
    return compress
