// svx_bgzf.cpp — the BGZF member layer (svx_bgzf.h): the member header, the host inflate with CRC32 and ISIZE checked, and
// the raw-DEFLATE C-ABI of include/svx_bam.h (svx_inflate_raw, svx_inflate_raw_pair).  Host code only.
#include "svx_bgzf.h"

#include <dlfcn.h>
#include <stdlib.h>

#include <algorithm>

#include "svx.h"
#include "svx_bam.h"

namespace {

// ------------------------------------------------------------------ optional libdeflate
struct LibDeflate {
    void* handle = nullptr;
    uint32_t (*crc32)(uint32_t, const void*, size_t) = nullptr;
};

const LibDeflate* libdeflate() {
    static const LibDeflate lib = [] {
        LibDeflate d;
        if (svx_bgzf::use_zlib()) return d;  // the zlib path, its CRC32 included (tests)
        void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return d;
        d.crc32 = reinterpret_cast<uint32_t (*)(uint32_t, const void*, size_t)>(dlsym(h, "libdeflate_crc32"));
        if (d.crc32) d.handle = h;
        else dlclose(h);
        return d;
    }();
    return lib.handle ? &lib : nullptr;
}

}  // namespace

namespace svx_bgzf {

// (one parser for both front ends: what svx_bam.cpp had as parse_block and svx_fasta_bgzf.cpp as its own parse_member)
int parse_member(const uint8_t* map, uint64_t fsize, uint64_t coff, Member* m) {
    if (coff == fsize) return 1;
    if (coff + 18 > fsize) return -1;
    const uint8_t* p = map + coff;
    if (p[0] != 0x1F || p[1] != 0x8B || p[2] != 8 || !(p[3] & 4)) return -1;
    const uint32_t xlen = le16(p + 10);
    // the subfield walk stays inside the file; that the 8 bytes of CRC32 and ISIZE do too follows from
    // coff + bsize <= fsize with bsize >= xlen + 20 below
    if (coff + 12 + xlen > fsize) return -1;
    uint32_t q = 12, end = 12 + xlen, bsize = 0;
    while (q + 4 <= end) {
        const uint32_t slen = le16(p + q + 2);
        if (p[q] == 66 && p[q + 1] == 67 && slen == 2 && q + 6 <= end) bsize = (uint32_t)le16(p + q + 4) + 1;
        q += 4 + slen;
    }
    if (!bsize || bsize < xlen + 20 || coff + bsize > fsize) return -1;
    m->bsize = bsize;
    m->payload_off = 12 + xlen;
    m->payload_len = bsize - xlen - 20;
    m->crc = le32(p + bsize - 8);
    m->isize = le32(p + bsize - 4);
    if (m->isize > 65536) return -1;
    return 0;
}

bool use_zlib() {
    static const bool z = [] { const char* v = getenv("SVX_BAM_ZLIB"); return v && v[0] == '1'; }();
    return z;
}

uint32_t member_crc(const uint8_t* p, size_t n) {
    const LibDeflate* L = libdeflate();
    if (L) return L->crc32(0, p, n);
    return (uint32_t)::crc32(::crc32(0L, Z_NULL, 0), p, (uInt)n);
}

bool Inflater::begin(const uint8_t* in, size_t in_len) {
    ++n_blocks;
    if (!zlib) {
        if (!own) own.reset(new svx_inflate::Stream());
        own->begin(in, in_len);
        return true;
    }
    if (!z_ready) {
        if (inflateInit2(&zs, -15) != Z_OK) return false;
        z_ready = true;
    } else if (inflateReset(&zs) != Z_OK) {
        return false;
    }
    zs.next_in = const_cast<Bytef*>(in);
    zs.avail_in = (uInt)in_len;
    return true;
}

bool Inflater::extend(uint8_t* out, size_t have, size_t want, size_t member_len, uint32_t crc, uint32_t* valid) {
    const bool whole = want == member_len;
    if (!zlib) {
        if (!own->run(out, member_len, want, whole)) return false;
        *valid = (uint32_t)own->produced();
        if (whole) return own->produced() == member_len && member_crc(out, member_len) == crc;
        return true;
    }
    *valid = (uint32_t)want;
    if (want <= have && !whole) return true;
    zs.next_out = out + have;
    zs.avail_out = (uInt)(want - have);
    const int rc = inflate(&zs, whole ? Z_FINISH : Z_SYNC_FLUSH);
    if (zs.avail_out != 0 || (rc != Z_OK && rc != Z_STREAM_END && rc != Z_BUF_ERROR)) return false;
    if (whole) {
        if (rc != Z_STREAM_END) return false;
        return member_crc(out, member_len) == crc;
    }
    return true;
}

bool Inflater::run_two(Inflater inf[2], const uint8_t* const in[2], const size_t in_len[2], uint8_t* const out[2],
                       const size_t isize[2], const size_t want[2], const uint32_t crc[2], size_t n, bool ok[2]) {
    ok[0] = ok[1] = false;
    if (n == 2 && !inf[0].zlib) {
        for (int k = 0; k < 2; ++k) (void)inf[k].begin(in[k], in_len[k]);
        svx_inflate::Stream::run_pair(*inf[0].own, out[0], isize[0], want[0], want[0] == isize[0], &ok[0],
                                      *inf[1].own, out[1], isize[1], want[1], want[1] == isize[1], &ok[1]);
        for (int k = 0; k < 2; ++k)
            if (ok[k] && want[k] == isize[k])
                ok[k] = inf[k].own->produced() == isize[k] && member_crc(out[k], isize[k]) == crc[k];
        return ok[0] && ok[1];
    }
    bool all = true;
    for (size_t k = 0; k < n; ++k) {
        uint32_t valid = 0;
        ok[k] = inf[k].begin(in[k], in_len[k]) && inf[k].extend(out[k], 0, want[k], isize[k], crc[k], &valid);
        all = all && ok[k];
    }
    return all;
}

}  // namespace svx_bgzf

extern "C" int svx_inflate_raw(const uint8_t* in, size_t in_len, uint8_t* out, size_t cap, const uint64_t* stops,
                               uint32_t n_stops, uint64_t* n_out) {
    if ((!in && in_len) || (!out && cap) || (!stops && n_stops) || !n_out) return SVX_E_INVALID;
    *n_out = 0;
    std::unique_ptr<svx_inflate::Stream> st(new svx_inflate::Stream());
    st->begin(in, in_len);
    for (uint32_t i = 0; i < n_stops; ++i) {
        const bool ok = st->run(out, cap, (size_t)std::min<uint64_t>(stops[i], cap), false);
        *n_out = st->produced();
        if (!ok) return SVX_E_INVALID;
    }
    const bool ok = st->run(out, cap, 0, true);
    *n_out = st->produced();
    return ok ? SVX_OK : SVX_E_INVALID;
}

extern "C" int svx_inflate_raw_pair(const uint8_t* in_a, size_t in_len_a, uint8_t* out_a, size_t cap_a, uint64_t stop_a,
                                    uint64_t* n_out_a, int* rc_a, const uint8_t* in_b, size_t in_len_b, uint8_t* out_b,
                                    size_t cap_b, uint64_t stop_b, uint64_t* n_out_b, int* rc_b) {
    if ((!in_a && in_len_a) || (!out_a && cap_a) || (!in_b && in_len_b) || (!out_b && cap_b) || !n_out_a || !n_out_b ||
        !rc_a || !rc_b)
        return SVX_E_INVALID;
    std::unique_ptr<svx_inflate::Stream> a(new svx_inflate::Stream()), b(new svx_inflate::Stream());
    a->begin(in_a, in_len_a);
    b->begin(in_b, in_len_b);
    bool ok_a = false, ok_b = false;
    const bool end_a = stop_a == ~0ull, end_b = stop_b == ~0ull;
    svx_inflate::Stream::run_pair(*a, out_a, cap_a, end_a ? 0 : (size_t)std::min<uint64_t>(stop_a, cap_a), end_a, &ok_a,
                                  *b, out_b, cap_b, end_b ? 0 : (size_t)std::min<uint64_t>(stop_b, cap_b), end_b, &ok_b);
    *n_out_a = a->produced();
    *n_out_b = b->produced();
    *rc_a = ok_a ? SVX_OK : SVX_E_INVALID;
    *rc_b = ok_b ? SVX_OK : SVX_E_INVALID;
    return SVX_OK;
}
