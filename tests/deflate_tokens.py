"""A DEFLATE (RFC 1951) token reader for tests, the counterpart of deflate_writer.py: it walks a raw stream and hands back
what a compressor DECIDED — per block BTYPE, HLIT / HDIST / HCLEN, the code lengths, and the tokens (a literal, or a
length and a distance) — which zlib's inflate keeps to itself.  Written from the RFC; it imports nothing from
svim_asm_amd.  Test infrastructure only: the judge of decoded bytes stays zlib (tests/test_deflate_tokens.py pins this
reader against zlib's own streams)."""
from tests.deflate_writer import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_D, FIXED_LL, LEN_BASE, LEN_EXTRA


class Bits:
    def __init__(self, data):
        self.data, self.at, self.acc, self.n = data, 0, 0, 0

    def need(self, n):
        while self.n < n:
            assert self.at < len(self.data), "the stream ends inside a block"
            self.acc |= self.data[self.at] << self.n
            self.at += 1
            self.n += 8

    def take(self, n):
        if not n:
            return 0
        self.need(n)
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.n -= n
        return v

    def peek(self, n):
        """n bits without consuming them; zeros behind the end of the data (a code may be shorter than n)."""
        while self.n < n and self.at < len(self.data):
            self.acc |= self.data[self.at] << self.n
            self.at += 1
            self.n += 8
        return self.acc & ((1 << n) - 1)

    def drop(self, n):
        assert n <= self.n, "the stream ends inside a code"
        self.acc >>= n
        self.n -= n

    def align(self):
        """To the next byte boundary, the bytes read ahead handed back."""
        self.drop(self.n % 8)
        self.at -= self.n // 8
        self.acc = self.n = 0

    @property
    def pos(self):
        return self.at * 8 - self.n


def table(lens):
    """(peek table, peek width) of the canonical code with these lengths (§3.2.2); the code must not be over-subscribed.
    Entries no code reaches (an incomplete code) stay None."""
    width = max(lens) if lens and max(lens) else 1
    count = [0] * (width + 2)
    for l in lens:
        if l:
            count[l] += 1
    code, nxt = 0, [0] * (width + 2)
    for bits in range(1, width + 1):
        code = (code + count[bits - 1]) << 1 if bits > 1 else 0
        nxt[bits] = code
    tab = [None] * (1 << width)
    for sym, l in enumerate(lens):
        if not l:
            continue
        c = nxt[l]
        nxt[l] += 1
        assert c < (1 << l), "over-subscribed code lengths"
        rev = int(format(c, "0%db" % l)[::-1], 2)  # Huffman codes are packed most significant bit first
        for k in range(rev, 1 << width, 1 << l):
            tab[k] = (sym, l)
    return tab, width


def _symbol(bits, tab, width):
    e = tab[bits.peek(width)]
    assert e is not None, "bits that are no code of an incomplete code"
    bits.drop(e[1])
    return e[0]


def read(stream):
    """The blocks of a raw DEFLATE stream up to and including the final one: a list of dicts with
        final, btype                    as written
        hlit, hdist, hclen              dynamic blocks: the COUNTS (257.., 1.., 4..)
        cl_lens, ll_lens, d_lens        dynamic blocks: the code lengths read (19 by symbol; hlit; hdist)
        tokens                          literals as int, matches as (length, distance); stored blocks: their bytes as literals
        bits                            (first bit, one past the last bit) of the block in the stream
    and the number of bytes the stream uses."""
    bits, blocks = Bits(stream), []
    while True:
        start = bits.pos
        final, btype = bits.take(1), bits.take(2)
        blk = dict(final=bool(final), btype=btype, tokens=[])
        assert btype != 3, "block type 3"
        if btype == 0:
            bits.align()
            ln, nlen = bits.take(16), bits.take(16)
            assert ln ^ nlen == 0xFFFF, "stored LEN / NLEN"
            bits.align()
            assert bits.at + ln <= len(stream), "the stream ends inside a stored block"
            blk["tokens"] = list(stream[bits.at:bits.at + ln])
            bits.at += ln
        else:
            if btype == 1:
                ll_lens, d_lens = FIXED_LL, FIXED_D
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl_lens = [0] * 19
                for k in range(hclen):
                    cl_lens[CL_ORDER[k]] = bits.take(3)
                tab, width = table(cl_lens)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, tab, width)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        assert lens, "16 with nothing to repeat"
                        lens += [lens[-1]] * (3 + bits.take(2))
                    else:
                        lens += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
                assert len(lens) == hlit + hdist, "a run past HLIT + HDIST"
                ll_lens, d_lens = lens[:hlit], lens[hlit:]
                assert ll_lens[256], "no end-of-block code"
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, ll_lens=ll_lens, d_lens=d_lens)
            ll_tab, ll_w = table(ll_lens)
            d_tab, d_w = table(d_lens)
            toks = blk["tokens"]
            # the hot loop, with the bit buffer in locals: 48 bits hold any whole token (15 + 5 + 15 + 13)
            data, at, acc, n = bits.data, bits.at, bits.acc, bits.n
            ll_mask, d_mask = (1 << ll_w) - 1, (1 << d_w) - 1
            while True:
                if n < 48:
                    chunk = data[at:at + 8]
                    acc |= int.from_bytes(chunk, "little") << n
                    at += len(chunk)
                    n += 8 * len(chunk)
                e = ll_tab[acc & ll_mask]
                assert e is not None, "bits that are no code of an incomplete code"
                s, l = e
                assert l <= n, "the stream ends inside a code"
                acc >>= l
                n -= l
                if s < 256:
                    toks.append(s)
                elif s == 256:
                    break
                else:
                    assert s <= 285, "literal/length symbol %d" % s
                    x = LEN_EXTRA[s - 257]
                    length = LEN_BASE[s - 257] + (acc & ((1 << x) - 1))
                    acc >>= x
                    e = d_tab[acc & d_mask]
                    assert e is not None, "bits that are no code of an incomplete code"
                    d, l = e
                    assert d <= 29, "distance symbol %d" % d
                    acc >>= l
                    y = DIST_EXTRA[d]
                    toks.append((length, DIST_BASE[d] + (acc & ((1 << y) - 1))))
                    acc >>= y
                    n -= x + l + y
                    assert n >= 0, "the stream ends inside a token"
            bits.at, bits.acc, bits.n = at, acc, n
        blk["bits"] = (start, bits.pos)
        blocks.append(blk)
        if final:
            return blocks, (bits.pos + 7) // 8


def replay(blocks):
    """The bytes the tokens stand for; a distance before the start of the output is an error."""
    out = bytearray()
    for b in blocks:
        for t in b["tokens"]:
            if isinstance(t, int):
                out.append(t)
                continue
            length, dist = t
            assert 1 <= dist <= len(out), "a distance of %d with %d bytes of output" % (dist, len(out))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                unit = bytes(out[len(out) - dist:])
                out += (unit * (length // dist + 1))[:length]
    return bytes(out)
