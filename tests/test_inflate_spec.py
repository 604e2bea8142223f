"""The seeded corpus of tests/deflate_writer.py — streams written from RFC 1951 alone, in the encodings zlib's and libdeflate's
compressors never use and in the malformed shapes a decoder must refuse on structure alone — against zlib's inflate (which
pins the writer to an independent decoder) and against the build's host decoder, svx_inflate_raw and svx_inflate_raw_pair
(svim_asm_amd/csrc/svx_inflate.h).  No GPU: the device forms run the same corpus in tests/test_gpu_inflate_spec.py."""
import ctypes as C
import random
import zlib

import pytest

from svim_asm_amd import _lib
from tests import deflate_writer as dw

DIGEST_SEED_0 = "ead31f1ac1e614b7502218e6674096f1e1b2ef3a20e4b00f82dc18c7d5191e01"


@pytest.fixture(scope="module")
def corpus():
    return dw.spec_corpus(0)


def zlib_inflate(payload):
    """zlib's verdict: the bytes up to the final block (anything behind it ignored), or None."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error:
        return None
    return out if d.eof else None


def host_inflate(payload, cap, stops=()):
    lib = _lib.load()
    out = (C.c_uint8 * max(cap, 1))()
    st = (C.c_uint64 * max(len(stops), 1))(*stops)
    n = C.c_uint64(0)
    rc = lib.svx_inflate_raw(payload, len(payload), out, cap, st, len(stops), C.byref(n))
    return rc, bytes(out[: n.value])


def host_inflate_pair(pa, cap_a, pb, cap_b):
    lib = _lib.load()
    oa, ob = (C.c_uint8 * max(cap_a, 1))(), (C.c_uint8 * max(cap_b, 1))()
    na, nb, ra, rb = C.c_uint64(0), C.c_uint64(0), C.c_int(7), C.c_int(7)
    end = 2 ** 64 - 1
    assert lib.svx_inflate_raw_pair(pa, len(pa), oa, cap_a, end, C.byref(na), C.byref(ra),
                                    pb, len(pb), ob, cap_b, end, C.byref(nb), C.byref(rb)) == 0
    return (ra.value, bytes(oa[: na.value])), (rb.value, bytes(ob[: nb.value]))


def test_corpus_is_deterministic_and_covers_every_category(corpus):
    assert dw.corpus_digest(corpus) == DIGEST_SEED_0
    assert dw.corpus_digest(dw.spec_corpus(1)) != DIGEST_SEED_0
    assert 250 <= len(corpus) <= 400
    names = {m.name for m in corpus}
    for cat in ("eob_shortest_1", "only_eob", "dist_single_1bit_0", "dist_none", "len258_as_284_fixed", "len258_as_284_dynamic",
                "rle_zero16", "rle_cross", "rep16_after_18", "hclen6", "hclen19", "dist_far_fixed", "empty_blocks_mid",
                "trailing_bytes_1", "stored_len_65531", "never_resync_60000", "codes_15bit_0", "overlap_d1_fixed",
                "overlap_d65_dynamic", "edge_64_eob_end", "edge_65_eob_start", "random",
                "isize_short", "isize_long", "crc_wrong", "isize_over_65536",
                "oversubscribed_ll", "oversubscribed_d", "oversubscribed_cl", "incomplete_ll", "incomplete_d",
                "incomplete_d_single_2bit", "incomplete_ll_15bit", "incomplete_cl", "no_eob", "hclen4_no_eob", "hlit_287",
                "hlit_288", "hdist_31", "hdist_32", "rep16_first", "rep_past_end", "rep_past_end_by_one", "fixed_ll_286",
                "fixed_ll_287", "fixed_d_30", "fixed_d_31", "dist_before_start_0", "dist_before_start_300", "stored_nlen",
                "type3", "dist_missing_code_used", "cut_at_symbol", "cut_in_header", "cut_in_stored"):
        assert cat in names, cat
    for m in corpus:
        assert len(m.payload) <= 65536
        assert (m.expect is None) == (m.status in (dw.BAD, dw.TRUNC))
        assert m.isize <= 65536 or m.status == dw.SIZE
        if m.status == dw.OK:
            assert (m.isize, m.crc) == (len(m.expect), dw.crc32(m.expect))


def test_zlib_decodes_every_valid_member_and_refuses_every_malformed_one(corpus):
    for k, m in enumerate(corpus):
        got = zlib_inflate(m.payload)
        if m.expect is None:
            assert got is None, (k, m.name)
        else:
            assert got == m.expect, (k, m.name)


def test_host_decoder_agrees_with_zlib(corpus):
    """svx_inflate_raw: every valid member whole and in resumed prefix steps, every malformed one refused (with the room
    its consistent ISIZE gives it)."""
    pr = random.Random(3)
    for k, m in enumerate(corpus):
        if m.expect is None:
            assert host_inflate(m.payload, min(m.isize, 65536))[0] != 0, (k, m.name)
            continue
        n = len(m.expect)
        assert host_inflate(m.payload, n) == (0, m.expect), (k, m.name)
        stops = sorted(pr.randrange(0, n + 1) for _ in range(pr.randrange(1, 5)))
        assert host_inflate(m.payload, n, stops) == (0, m.expect), (k, m.name, stops)
        if n:
            assert host_inflate(m.payload, n - 1)[0] != 0, (k, m.name)


def test_host_pair_decoder_agrees_with_zlib(corpus):
    """svx_inflate_raw_pair: two members side by side, each what it is alone."""
    pr = random.Random(4)
    for _ in range(300):
        a, b = pr.choice(corpus), pr.choice(corpus)
        cap_a, cap_b = min(a.isize, 65536), min(b.isize, 65536)
        if a.expect is not None:
            cap_a = len(a.expect)
        if b.expect is not None:
            cap_b = len(b.expect)
        got_a, got_b = host_inflate_pair(a.payload, cap_a, b.payload, cap_b)
        for got, m in ((got_a, a), (got_b, b)):
            if m.expect is None:
                assert got[0] != 0, m.name
            else:
                assert got == (0, m.expect), m.name
