"""The VCF as bgzip and tabix write it (`--bgzip_output`): `variants.vcf.gz` (BGZF: blocks of 65 280 bytes, one gzip
member each, the EOF member behind) and its index `variants.vcf.gz.tbi`, or `.csi` when a record ends beyond 2^29.

The members are compressed on the device (svx_bgzf_deflate_dev, svx_deflate.hip) or with zlib on host threads
(svx_bgzf_compress with no context); the index is built on the host (svx_tabix_build) while the device works."""
import ctypes as C
import logging
import os

import numpy as np

from svim_asm_amd import _lib

BLOCK = 65280
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# Whether the command compresses on its device: SVX_VCF_BGZF_DEVICE=1 / =0 decide, else this default, chosen from
# tools/vcf_bgzf_probe.py's measurements
DEVICE_DEFAULT = True
HOST_THREADS = 16


def device_path_wanted():
    v = os.environ.get("SVX_VCF_BGZF_DEVICE")
    if v in ("0", "1"):
        return v == "1"
    return DEVICE_DEFAULT


def _addr(data):
    """(address, length, keep-alive) of bytes-like data or of an (address, length) pair."""
    if isinstance(data, tuple):
        return data[0], data[1], None
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    return buf.ctypes.data, len(data), buf


def compress(data, ctx=None, n_threads=HOST_THREADS):
    """BGZF of `data` (bytes-like, or (address, length)): on `ctx`'s device, or with zlib on host threads when ctx is
    None.  Returns (bytes, member sizes as uint32)."""
    lib = _lib.load()
    ptr, n, keep = _addr(data)
    out, out_len, ml, n_m = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    rc = lib.svx_bgzf_compress(ctx.h if ctx is not None else None, ptr, n, int(n_threads), C.byref(out), C.byref(out_len),
                               C.byref(ml), C.byref(n_m))
    del keep
    if rc != _lib.SVX_OK:
        msg = (lib.svx_last_error(ctx.h) or b"").decode() if ctx is not None else ""
        raise _lib.SvxError(rc, "svx_bgzf_compress " + msg)
    try:
        blob = C.string_at(out, out_len.value)
        sizes = np.frombuffer(C.string_at(ml, 4 * n_m.value), dtype=np.uint32).copy() if n_m.value else np.zeros(0, np.uint32)
    finally:
        lib.svx_bgzf_free(out)
        lib.svx_bgzf_free(ml)
    return blob, sizes


class Unordered(Exception):
    """The records cannot be indexed (svx_tabix_build's kind 0); the message names the first offending record."""


def build_index(data, member_sizes):
    """(index bytes, uncompressed, and 'tbi' or 'csi') for text `data` compressed into members of `member_sizes`."""
    lib = _lib.load()
    ptr, n, keep = _addr(data)
    sizes = np.ascontiguousarray(member_sizes, dtype=np.uint32)
    out, out_len, kind = C.c_void_p(), C.c_uint64(), C.c_int()
    err = C.create_string_buffer(512)
    rc = lib.svx_tabix_build(ptr, n, sizes.ctypes.data if len(sizes) else None, len(sizes), C.byref(out), C.byref(out_len),
                             C.byref(kind), err, len(err))
    del keep
    if rc != _lib.SVX_OK:
        raise _lib.SvxError(rc, "svx_tabix_build: " + err.value.decode("utf-8", "replace"))
    if kind.value == 0:
        raise Unordered(err.value.decode("utf-8", "replace"))
    try:
        return C.string_at(out, out_len.value), ("tbi" if kind.value == 1 else "csi")
    finally:
        lib.svx_vcf_free(out)


def _write(path, blob):
    with open(path, "wb") as fh:
        fh.write(blob)


def write(path, data, ctx=None):
    """`path` (…/variants.vcf.gz) and its index from the text `data` (bytes-like or (address, length)).  ctx: the
    device context to compress on when the device path is wanted (None: host).  Returns the index path or None when
    the records could not be indexed.  On any failure neither file is left behind."""
    index_paths = [path + ".tbi", path + ".csi"]
    use_dev = ctx is not None and device_path_wanted()
    try:
        blob = None
        if use_dev:
            try:
                blob, sizes = compress(data, ctx=ctx)
            except _lib.SvxError as e:
                if e.status != _lib.SVX_E_NOMEM:
                    raise
                logging.warning("variants.vcf.gz: the device has no memory for the compression (%s); compressing on the "
                                "host instead", e)
        if blob is None:
            blob, sizes = compress(data, ctx=None)
        try:
            index, kind = build_index(data, sizes)
        except Unordered as u:
            index, kind = None, None
            logging.warning("%s is not indexed: %s", os.path.basename(path), u)
        _write(path, blob)
        for p in index_paths:
            if os.path.exists(p) and (index is None or not p.endswith("." + kind)):
                os.remove(p)
        if index is None:
            return None
        ipath = path + "." + kind
        _write(ipath, compress(index, ctx=None, n_threads=1)[0])
        return ipath
    except BaseException:
        for p in [path] + index_paths:
            if os.path.exists(p):
                os.remove(p)
        raise
