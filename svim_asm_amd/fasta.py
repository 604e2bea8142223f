"""Indexed FASTA access (.fai) for the host side: the subset of pysam.FastaFile the reference
uses (svim-asm:124; SVIM_COMBINE.py:45-99,467; SVCandidate.py:57-58,105,155,210,301-302):
0-based half-open `fetch`, `get_reference_length`, `close`, and the two error conditions
main() distinguishes (missing file → IOError, missing index → ValueError).

A bgzip-compressed FASTA (`ref.fa.gz` + `.fai` + `.gzi`, what `bgzip` and `samtools faidx` write) is read as
htslib's faidx reads it: recognised by its content (gzip magic, FLG.FEXTRA, the BC subfield), the `.fai` offsets
counting uncompressed bytes, the `.gzi` mapping them to members.  Every fetch goes through libsvx.so
(svx_fasta_open_bgzf), which inflates and checks the members under the windows on the host threads or, with a
`device`, on the GPU."""
import mmap
import os
import struct

import numpy as np


class MissingGziError(ValueError):
    """A bgzip-compressed FASTA without its `.gzi` (faidx refuses it too)."""


class BgzfFormatError(ValueError):
    """A compressed FASTA that cannot be read: plain gzip (not BGZF), a malformed `.gzi` or member chain."""


DEVICE_MIN_MEMBERS = 64  # batch calls under this many distinct members stay on the host threads
# Whether a compressed genome opened with a device inflates its members there: SVX_FASTA_DEVICE=1 / =0 decide, else this
# default, chosen from tools/fasta_bgzf_probe.py's measurements
DEVICE_DEFAULT = True


def device_path_wanted():
    v = os.environ.get("SVX_FASTA_DEVICE")
    if v in ("0", "1"):
        return v == "1"
    return DEVICE_DEFAULT


def bgzf_kind(path):
    """'bgzf', 'gzip' or None (not gzip-compressed), from the file's first bytes."""
    with open(path, "rb") as fh:
        head = fh.read(18)
    if len(head) < 2 or head[:2] != b"\x1f\x8b":
        return None
    if len(head) < 12 or head[2] != 8 or not head[3] & 4:
        return "gzip"
    xlen = struct.unpack_from("<H", head, 10)[0]
    with open(path, "rb") as fh:
        fh.seek(12)
        extra = fh.read(xlen)
    q = 0
    while q + 4 <= len(extra):
        slen = struct.unpack_from("<H", extra, q + 2)[0]
        if extra[q:q + 2] == b"BC" and slen == 2:
            return "bgzf"
        q += 4 + slen
    return "gzip"


def read_gzi(path):
    """(compressed offsets, uncompressed offsets) of a `.gzi` as uint64 arrays."""
    raw = open(path, "rb").read()
    if len(raw) < 8:
        raise BgzfFormatError("%s: truncated .gzi index" % path)
    n = struct.unpack_from("<Q", raw, 0)[0]
    if len(raw) != 8 + 16 * n:
        raise BgzfFormatError("%s: .gzi index of %d entries has %d bytes" % (path, n, len(raw)))
    pairs = np.frombuffer(raw, dtype="<u8", offset=8).reshape(-1, 2) if n else np.zeros((0, 2), np.uint64)
    return np.ascontiguousarray(pairs[:, 0], dtype=np.uint64), np.ascontiguousarray(pairs[:, 1], dtype=np.uint64)


class FastaFile(object):
    def __init__(self, path, device=None):
        if not os.path.exists(path):
            raise IOError("file `%s` not found" % path)
        if not os.path.exists(path + ".fai"):
            raise ValueError("no index (.fai) for %s" % path)
        kind = bgzf_kind(path)
        if kind == "gzip":
            raise BgzfFormatError("%s is gzip-compressed but not BGZF: recompress it with bgzip" % path)
        self.compressed = kind == "bgzf"
        if self.compressed and not os.path.exists(path + ".gzi"):
            raise MissingGziError("no .gzi index for the bgzip-compressed %s" % path)
        self.filename = path
        self._idx = {}
        self.references, self.lengths = [], []
        with open(path + ".fai") as fh:
            for line in fh:
                f = line.rstrip("\n").split("\t")
                if len(f) < 5:
                    continue
                self._idx[f[0]] = (int(f[1]), int(f[2]), int(f[3]), int(f[4]))
                self.references.append(f[0])
                self.lengths.append(int(f[1]))
        self._native = None  # svx_fasta handle (libsvx.so), opened by the first batch fetch (a compressed file: here)
        if self.compressed:
            self._fh, self._map = None, None
            self._handle()
            if device is not None and device_path_wanted():
                lib, h = self._native
                lib.svx_fasta_set_device(h, int(device), DEVICE_MIN_MEMBERS)
            return
        self._fh = open(path, "rb")
        # fetches are tens of thousands of short windows (haplotype flanks, VCF alleles): slices of a
        # read-only mapping instead of a seek + read pair each
        try:
            self._map = mmap.mmap(self._fh.fileno(), 0, access=mmap.ACCESS_READ) if os.path.getsize(path) else None
        except (OSError, ValueError):
            self._map = None

    def _handle(self):
        if getattr(self, "_closed", False):
            raise ValueError("I/O operation on closed file")
        if self._native is None:
            import ctypes as C
            from svim_asm_amd import _lib
            lib = _lib.load()
            rows = [self._idx[name] for name in self.references]
            cols = [np.array([r[k] for r in rows], dtype=dt) for k, dt in ((0, np.int64), (1, np.int64), (2, np.int32), (3, np.int32))]
            h, err = C.c_void_p(), C.create_string_buffer(256)
            if self.compressed:
                coff, uoff = read_gzi(self.filename + ".gzi")
                rc = lib.svx_fasta_open_bgzf(os.fsencode(self.filename), len(rows), cols[0].ctypes.data, cols[1].ctypes.data,
                                             cols[2].ctypes.data, cols[3].ctypes.data, coff.ctypes.data, uoff.ctypes.data,
                                             len(coff), C.byref(h), err, len(err))
                if rc != 0:
                    raise BgzfFormatError("%s: %s" % (self.filename, err.value.decode(errors="replace")))
            else:
                rc = lib.svx_fasta_open(os.fsencode(self.filename), len(rows), cols[0].ctypes.data, cols[1].ctypes.data,
                                        cols[2].ctypes.data, cols[3].ctypes.data, C.byref(h), err, len(err))
            if rc != 0:
                raise IOError(err.value.decode(errors="replace"))
            self._native = (lib, h)
            self._ref_index = {}
            for i, name in enumerate(self.references):
                self._ref_index.setdefault(name, i)
        return self._native

    def fetch_batch(self, contigs, start, end, upper=True, ids=None):
        """fetch(contigs[i], start[i], end[i]) for all i in one native call (threads, no str objects):
        (uint8 pool, int64 offsets [n + 1]); `upper` applies str.upper() to every slice.  With `ids`, interval i
        lies on contigs[ids[i]] (a table's contig names and its id column: names are looked up once each)."""
        lib, h = self._handle()
        if ids is not None:
            ids = np.asarray(ids, dtype=np.int64)
            n = len(ids)
            used = np.unique(ids) if n else ids
            table = np.full(len(contigs), -1, dtype=np.int32)
            for c in used.tolist():
                table[c] = self._ref_index[contigs[c]]   # KeyError for a contig the FASTA does not have, as fetch()
            ref = np.ascontiguousarray(table[ids])
        else:
            n = len(contigs)
            ref = np.fromiter((self._ref_index[c] for c in contigs), dtype=np.int32, count=n)
        start = np.ascontiguousarray(start, dtype=np.int64)
        end = np.ascontiguousarray(end, dtype=np.int64)
        if n and (bool((start < 0).any()) or bool((end < start).any())):
            raise ValueError("fetch coordinates out of range")
        length = np.asarray(self.lengths, dtype=np.int64)[ref] if n else np.zeros(0, np.int64)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.maximum(np.minimum(end, length) - start, 0), out=off[1:])
        out = np.empty(int(off[-1]), dtype=np.uint8)
        rc = lib.svx_fasta_fetch_batch(h, ref.ctypes.data, start.ctypes.data, end.ctypes.data, n, 1 if upper else 0,
                                       off.ctypes.data, out.ctypes.data, 0)
        if rc != 0:
            if self.compressed:
                raise ValueError("%s: %s" % (self.filename, lib.svx_fasta_last_error(h).decode(errors="replace")))
            raise ValueError("reference windows shorter than the index says (%s)" % self.filename)
        return out, off.astype(np.int64)

    def fetch_oriented(self, contigs, start, end, reverse, bam_alphabet=True):
        """fetch_batch with a direction per window (svx_fasta_fetch_oriented, include/svx_text.h): window i is written as
        its reverse complement where reverse[i] is set, and with `bam_alphabet` every byte goes through the 16 letters of a
        BAM record's SEQ (lower case -> upper, anything else -> N).  (uint8 pool, int64 offsets [n + 1])."""
        lib, h = self._handle()
        n = len(contigs)
        ref = np.fromiter((self._ref_index[c] for c in contigs), dtype=np.int32, count=n)
        start = np.ascontiguousarray(start, dtype=np.int64)
        end = np.ascontiguousarray(end, dtype=np.int64)
        reverse = np.ascontiguousarray(np.asarray(reverse).astype(bool), dtype=np.uint8)
        if len(start) != n or len(end) != n or len(reverse) != n:
            raise ValueError("fetch_oriented: columns of different lengths")
        if n and (bool((start < 0).any()) or bool((end < start).any())):
            raise ValueError("fetch coordinates out of range")
        length = np.asarray(self.lengths, dtype=np.int64)[ref] if n else np.zeros(0, np.int64)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.maximum(np.minimum(end, length) - start, 0), out=off[1:])
        out = np.empty(int(off[-1]), dtype=np.uint8)
        rc = lib.svx_fasta_fetch_oriented(h, ref.ctypes.data, start.ctypes.data, end.ctypes.data, reverse.ctypes.data, n,
                                          1 if bam_alphabet else 0, off.ctypes.data, out.ctypes.data, 0)
        if rc != 0:
            if self.compressed:
                raise ValueError("%s: %s" % (self.filename, lib.svx_fasta_last_error(h).decode(errors="replace")))
            raise ValueError("windows shorter than the index says (%s)" % self.filename)
        return out, off.astype(np.int64)

    def stats(self):
        """Counters of a compressed file's fetches (all 0 for a plain one): members inflated on the host and on the
        device, compressed bytes staged for the device, cache hits, device calls, host calls."""
        import ctypes as C
        if getattr(self, "_closed", False):
            return dict(getattr(self, "_last_stats", {}))
        lib, h = self._handle()
        v = np.zeros(6, dtype=np.uint64)
        lib.svx_fasta_stats(h, v.ctypes.data_as(C.c_void_p))
        keys = ("host_members", "device_members", "bytes_staged", "cache_hits", "device_calls", "host_calls")
        return {k: int(x) for k, x in zip(keys, v.tolist())}

    def get_reference_length(self, name):
        return self._idx[name][0]

    def fetch(self, reference, start=None, end=None):
        return self.fetch_bytes(reference, start, end).decode("ascii")

    def fetch_bytes(self, reference, start=None, end=None):
        """fetch() without the str round trip (the GPU path uploads reference windows as bytes)."""
        if getattr(self, "_closed", False):
            raise ValueError("I/O operation on closed file")
        length, offset, line_bases, line_width = self._idx[reference]
        start = 0 if start is None else start
        end = length if end is None else end
        if start < 0:
            raise ValueError("start out of range (%i)" % start)
        if end < start:
            raise ValueError("end out of range (%i)" % end)
        end = min(end, length)
        if start >= end:
            return b""
        if self.compressed:
            out, _ = self.fetch_batch([reference], np.array([start], np.int64), np.array([end], np.int64), upper=False)
            return out.tobytes()
        b0 = offset + (start // line_bases) * line_width + start % line_bases
        b1 = offset + ((end - 1) // line_bases) * line_width + (end - 1) % line_bases + 1
        if self._map is not None:
            raw = self._map[b0:b1]
        else:
            self._fh.seek(b0)
            raw = self._fh.read(b1 - b0)
        if line_width != line_bases:
            raw = raw.replace(b"\n", b"").replace(b"\r", b"")
        return raw

    def close(self):
        """The object is closed at once (fetches fail from here on); its mappings are released by release_deferred().
        Unmapping a genome-sized file whose pages were touched all over is tens of milliseconds of page-table work
        under the process's mapping lock (57 ms for the 3.1 GB of the full-size sample) — in the middle of
        write_final_vcf, where the reference closes its FastaFile (SVIM_COMBINE.py:466-467), it would stall the threads
        that format the record lines; a command that exits right after the VCF never needs it at all."""
        if getattr(self, "_native", None) is not None and not getattr(self, "_closed", False):
            self._last_stats = self.stats()  # (what the fetches did stays readable behind close)
        self._closed = True
        if getattr(self, "_native", None) is not None:
            _DEFERRED.append(("native",) + tuple(self._native))
            self._native = None
        if getattr(self, "_map", None) is not None:
            _DEFERRED.append(("map", self._map))
            self._map = None
        if getattr(self, "_fh", None):
            _DEFERRED.append(("file", self._fh))
            self._fh = None
        if len(_DEFERRED) > 12:  # a caller that opens and closes many genomes and never writes a VCF: bounded
            release_deferred()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass


_DEFERRED = []  # mappings and descriptors of closed FastaFile objects, not yet given back


def release_deferred(background=True):
    """Give back what closed FastaFile objects held (write_vcf_table calls this behind its last write; a long-lived
    caller may call it any time).  `background`: on a daemon thread, beside whatever the caller does next."""
    todo = _DEFERRED[:]
    del _DEFERRED[:len(todo)]
    if not todo:
        return

    def work():
        for item in todo:
            try:
                if item[0] == "native":
                    item[1].svx_fasta_close(item[2])
                else:
                    item[1].close()
            except Exception:  # noqa: BLE001 — nothing left to report to
                pass
    if background:
        import threading
        threading.Thread(target=work, daemon=True).start()
    else:
        work()


def write_fasta(path, names, seqs, line=60):
    """Write FASTA + .fai; `seqs` are ASCII byte strings / numpy uint8 arrays."""
    with open(path, "wb") as fh, open(path + ".fai", "w") as fai:
        for name, seq in zip(names, seqs):
            a = np.frombuffer(seq, dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq
            hdr = (">%s\n" % name).encode()
            fh.write(hdr)
            off = fh.tell()
            n = len(a)
            full = n // line
            if full:
                body = np.empty((full, line + 1), dtype=np.uint8)
                body[:, :line] = a[:full * line].reshape(full, line)
                body[:, line] = 10
                fh.write(body.tobytes())
            if n % line:
                fh.write(a[full * line:].tobytes() + b"\n")
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (name, n, off, line, line + 1))


def bgzip_fasta(src, dst, level=6, member_size=0xFF00, threads=1, gzi_end=False):
    """bgzip `src` (a FASTA with its .fai) into `dst` with `dst`.fai (the same: its offsets count uncompressed bytes) and
    `dst`.gzi.  level: zlib 0-9, or 100 + n for libdeflate at level n (bamio's writers' convention; what bgzip writes
    when htslib has libdeflate).  member_size: uncompressed bytes per member (bgzip: 0xFF00).  gzi_end: the .gzi also
    lists the end of the data."""
    from concurrent.futures import ThreadPoolExecutor
    from svim_asm_amd import bamio
    data = open(src, "rb").read()
    mv = memoryview(data)
    starts = list(range(0, len(data), member_size))
    if threads > 1 and len(starts) > 64:
        with ThreadPoolExecutor(min(int(threads), 16)) as ex:
            parts = list(ex.map(lambda p: bamio._bgzf_member(mv[p:p + member_size], level), starts))
    else:
        parts = [bamio._bgzf_member(mv[p:p + member_size], level) for p in starts]
    entries, coff = [], 0
    for k, part in enumerate(parts):
        if k:
            entries.append((coff, starts[k]))
        coff += len(part)
    if gzi_end:  # (the end of the data: where the EOF marker starts)
        entries.append((coff, len(data)))
    with open(dst, "wb") as fh:
        fh.write(b"".join(parts))
        fh.write(bamio._BGZF_EOF)
    with open(dst + ".gzi", "wb") as fh:
        fh.write(struct.pack("<Q", len(entries)))
        for c, u in entries:
            fh.write(struct.pack("<QQ", c, u))
    with open(src + ".fai", "rb") as a, open(dst + ".fai", "wb") as b:
        b.write(a.read())
    return dst


def write_bgzf_fasta(path, names, seqs, line=60, level=6, member_size=0xFF00, threads=1, gzi_end=False):
    """write_fasta, then bgzip: `path` (compressed) with `path`.fai and `path`.gzi."""
    import tempfile
    fd, tmp = tempfile.mkstemp(suffix=".fa", dir=os.path.dirname(os.path.abspath(path)))
    os.close(fd)
    try:
        write_fasta(tmp, names, seqs, line=line)
        bgzip_fasta(tmp, path, level=level, member_size=member_size, threads=threads, gzi_end=gzi_end)
    finally:
        for p in (tmp, tmp + ".fai"):
            if os.path.exists(p):
                os.remove(p)
    return path
