"""An independent reader of bgzip-compressed, tabix-indexed VCFs, written from the hts-specs (SAMv1 §4.1 BGZF, tabix,
CSIv1) for the tests of `--bgzip_output`: the BGZF member chain with its structure checks, .tbi / .csi parsing, and
region queries answered the way htslib's iterator does (bins overlapping the region, chunks behind the minimum offset,
records read from the virtual offsets until the first one with beg >= end)."""
import gzip
import struct
import zlib

BLOCK = 65280
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def members(blob):
    """[(offset, size, payload, crc, isize)] of a BGZF file, every header field checked."""
    out, p = [], 0
    while p < len(blob):
        assert blob[p:p + 4] == b"\x1f\x8b\x08\x04", "member %d: bad magic / flags" % len(out)
        mtime, xfl, os_, xlen = struct.unpack_from("<IBBH", blob, p + 4)
        assert (mtime, xfl, os_, xlen) == (0, 0, 0xFF, 6)
        assert blob[p + 12:p + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", blob, p + 16)[0] + 1
        assert p + size <= len(blob) and size <= 65536
        crc, isize = struct.unpack_from("<II", blob, p + size - 8)
        out.append((p, size, blob[p + 18:p + size - 8], crc, isize))
        p += size
    return out


def check_bgzf(blob, text):
    """The structure bgzip writes for `text`: members of 65 280 input bytes (the last data member shorter), each with a
    right CRC32 and ISIZE, then exactly the EOF member.  Returns the data members' sizes."""
    assert blob.endswith(EOF_MEMBER)
    ms = members(blob)
    assert ms[-1][0] == len(blob) - 28
    data = ms[:-1]
    assert len(data) == (len(text) + BLOCK - 1) // BLOCK
    got = bytearray()
    for k, (_, size, payload, crc, isize) in enumerate(data):
        raw = zlib.decompressobj(-15).decompress(payload)
        assert len(raw) == isize and isize == (BLOCK if k < len(data) - 1 else len(text) - BLOCK * (len(data) - 1))
        assert zlib.crc32(raw) == crc
        got += raw
    assert bytes(got) == text
    assert gzip.decompress(blob) == text
    return [m[1] for m in data]


def reg2bin(beg, end, min_shift, depth):
    end -= 1
    s, t = min_shift, ((1 << depth * 3) - 1) // 7
    for l in range(depth, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 1 << (l - 1) * 3
    return 0


def reg2bins(beg, end, min_shift, depth):
    end -= 1
    out, s, t = [], min_shift + depth * 3, 0
    for l in range(depth + 1):
        b, e = t + (beg >> s), t + (end >> s)
        out.extend(range(b, e + 1))
        s -= 3
        t += 1 << l * 3
    return out


class Index:
    """A parsed .tbi or .csi (the decompressed bytes)."""

    def __init__(self, raw):
        self.csi = raw[:4] == b"CSI\x01"
        assert self.csi or raw[:4] == b"TBI\x01"
        p = 4
        if self.csi:
            self.min_shift, self.depth, l_aux = struct.unpack_from("<iii", raw, p)
            p += 12
            aux = raw[p:p + l_aux]
            p += l_aux
            (self.n_ref,) = struct.unpack_from("<i", raw, p)
            p += 4
            conf = aux
        else:
            self.min_shift, self.depth = 14, 5
            (self.n_ref,) = struct.unpack_from("<i", raw, p)
            conf = raw[p + 4:]
        fmt, cs, cb, ce, meta, skip, l_nm = struct.unpack_from("<7i", conf, 0)
        assert (fmt, cs, cb, ce, meta, skip) == (2, 1, 2, 0, 35, 0)
        self.names = conf[28:28 + l_nm].split(b"\0")[:-1]
        if not self.csi:
            p += 4 + 28 + l_nm
        self.meta_bin = ((1 << (3 * self.depth + 3)) - 1) // 7 + 1
        self.refs = []
        for _ in range(self.n_ref):
            (n_bin,) = struct.unpack_from("<i", raw, p)
            p += 4
            bins, loff, pseudo = {}, {}, None
            for _ in range(n_bin):
                (b,) = struct.unpack_from("<I", raw, p)
                p += 4
                if self.csi:
                    loff[b] = struct.unpack_from("<Q", raw, p)[0]
                    p += 8
                (n_chunk,) = struct.unpack_from("<i", raw, p)
                p += 4
                ch = [struct.unpack_from("<QQ", raw, p + 16 * i) for i in range(n_chunk)]
                p += 16 * n_chunk
                if b == self.meta_bin:
                    pseudo = ch
                else:
                    bins[b] = ch
            ioff = []
            if not self.csi:
                (n_intv,) = struct.unpack_from("<i", raw, p)
                p += 4
                ioff = list(struct.unpack_from("<%dQ" % n_intv, raw, p))
                p += 8 * n_intv
            self.refs.append({"bins": bins, "loff": loff, "ioff": ioff, "pseudo": pseudo})
        rest = raw[p:]
        assert rest in (b"", b"\0" * 8)

    def record_count(self, name):
        r = self.refs[self.names.index(name.encode())]
        return r["pseudo"][1][0]

    def chunks(self, name, beg, end):
        """htslib hts_itr_query: the chunks to read for [beg, end), merged and sorted."""
        if name.encode() not in self.names:
            return []
        r = self.refs[self.names.index(name.encode())]
        if self.csi:
            min_off = 0
            b = reg2bin(beg, beg + 1, self.min_shift, self.depth)
            while True:  # the finest bin containing beg that exists, or its nearest ancestor that does
                if b in r["loff"]:
                    min_off = r["loff"][b]
                    break
                if b == 0:
                    break
                b = (b - 1) >> 3
        else:
            ioff = r["ioff"]
            w = beg >> self.min_shift
            min_off = (ioff[w] if w < len(ioff) else ioff[-1]) if ioff else 0
        out = []
        for b in reg2bins(beg, end, self.min_shift, self.depth):
            for cb, ce in r["bins"].get(b, []):
                if ce > min_off:
                    out.append((cb, ce))
        return sorted(out)


class Reader:
    """Region queries over a .vcf.gz and its index."""

    def __init__(self, gz_bytes, index_bytes):
        self.blob = gz_bytes
        self.ms = {m[0]: m for m in members(gz_bytes)}
        self.index = Index(gzip.decompress(index_bytes))
        self._cache = {}

    def _block(self, coff):
        if coff not in self._cache:
            self._cache[coff] = zlib.decompressobj(-15).decompress(self.ms[coff][2])
        return self._cache[coff]

    def _read_from(self, voff, stop):
        """Lines from virtual offset voff until the virtual offset `stop` is reached (yields (line, voff_after))."""
        coff, uoff = voff >> 16, voff & 0xFFFF
        buf = b""
        while True:
            if (coff << 16 | uoff) >= stop and not buf:
                return
            if coff not in self.ms:
                return
            data = self._block(coff)
            if uoff >= len(data):
                coff += self.ms[coff][1]
                uoff = 0
                continue
            nl = data.find(b"\n", uoff)
            if nl < 0:
                buf += data[uoff:]
                coff += self.ms[coff][1]
                uoff = 0
                continue
            line = buf + data[uoff:nl]
            buf = b""
            uoff = nl + 1
            yield line, coff << 16 | uoff

    def query(self, name, beg, end):
        """Lines of contig `name` overlapping [beg, end) (0-based, half-open) in file order."""
        out, seen = [], set()
        for cb, ce in self.index.chunks(name, beg, end):
            for line, _ in self._read_from(cb, ce):
                f = line.split(b"\t")
                if f[0].decode() != name:
                    continue
                rb, re_ = interval(line)
                if rb >= end:
                    break
                if re_ > beg and line not in seen:
                    seen.add(line)
                    out.append(line)
        return out


def interval(line):
    """tbx_parse1 for the VCF preset: (beg, end) of a record line (bytes)."""
    f = line.split(b"\t")
    beg = int(f[1]) - 1
    end = beg + len(f[3])
    info = f[7] if len(f) > 7 else b""
    for kv in info.split(b";"):
        if kv.startswith(b"END="):
            v = kv[4:]
            if v != b"." and v.isdigit() and int(v) > beg:
                end = int(v)
            break
    if end <= beg:
        end = beg + 1
    return beg, end


def brute(text, name, beg, end):
    out = []
    for line in text.split(b"\n"):
        if not line or line.startswith(b"#"):
            continue
        if line.split(b"\t")[0].decode() == name:
            b, e = interval(line)
            if b < end and e > beg:
                out.append(line)
    return out
