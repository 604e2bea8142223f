// svx_bgzf.h — the BGZF member layer under the BAM reader (svx_bam.cpp) and the bgzip-FASTA handle (svx_fasta_bgzf.cpp):
// what a member is (SAM specification §4.1), how one is inflated and checked on the host, and how a set of members is
// laid out for the device inflate of svx_inflate.hip (svx_inflate_dev.h).  Internal; host code only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <zlib.h>

#include <memory>
#include <vector>

#include "svx_inflate.h"
#include "svx_inflate_dev.h"

namespace svx_bgzf {

inline uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

// ------------------------------------------------------------------ member header
struct Member {
    uint32_t bsize = 0, isize = 0, payload_off = 0, payload_len = 0, crc = 0;
};

// The member whose header starts at file offset coff: 0 ok, 1 clean end of file (coff == fsize), -1 malformed (gzip
// magic, CM 8, FLG.FEXTRA, a BC subfield of length 2 among the extra subfields, ISIZE at most 65 536).
int parse_member(const uint8_t* map, uint64_t fsize, uint64_t coff, Member* m);

// ------------------------------------------------------------------ host inflate
// SVX_BAM_ZLIB=1: the BAM reader inflates with zlib, the differential oracle of the build's own decoder (svx_inflate.h).
bool use_zlib();
// CRC32 of a member's bytes: libdeflate's routine when the runtime has the library (dlopen, optional; carry-less multiply:
// 64 KiB in a few µs where zlib's table walk takes 40) and SVX_BAM_ZLIB is not 1, zlib's otherwise.
uint32_t member_crc(const uint8_t* p, size_t n);

struct Inflater {
    z_stream zs;
    bool z_ready = false;
    const bool zlib;  // the decoder: zlib, or the build's own
    std::unique_ptr<svx_inflate::Stream> own;
    uint64_t n_blocks = 0;

    explicit Inflater(bool with_zlib) : zlib(with_zlib) { memset(&zs, 0, sizeof(zs)); }
    Inflater(const Inflater&) = delete;
    Inflater& operator=(const Inflater&) = delete;
    ~Inflater() {
        if (z_ready) inflateEnd(&zs);
    }
    // Streaming use: begin() a member, then extend() the inflated prefix as far as somebody needs it.
    // A slice of a contig-sized SEQ field sits somewhere inside a 64 KiB member: inflating only up to its last
    // byte halves the work on average.  The CRC covers whole members, so it is checked when (and only when)
    // the prefix reaches the member's end.
    bool begin(const uint8_t* in, size_t in_len);
    // `out` holds `have` bytes of the member already (zlib: exactly; own decoder: at least — it may have run past the
    // last request by up to one match, *valid is what is there now)
    bool extend(uint8_t* out, size_t have, size_t want, size_t member_len, uint32_t crc, uint32_t* valid);
    // raw deflate stream `in` → exactly out_len bytes, CRC32 checked
    bool run(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_len, uint32_t crc) {
        uint32_t valid = 0;
        return begin(in, in_len) && extend(out, 0, out_len, out_len, crc, &valid);
    }
    // One or two members at once, each inflated into out[k] (room for isize[k] bytes) up to want[k] of its isize[k] bytes
    // (want == isize: to the end, CRC32 checked); with the build's own decoder two members are decoded side by side
    // (svx_inflate::Stream::run_pair).  ok[k]: member k came out right; returns whether all n did.
    static bool run_two(Inflater inf[2], const uint8_t* const in[2], const size_t in_len[2], uint8_t* const out[2],
                        const size_t isize[2], const size_t want[2], const uint32_t crc[2], size_t n, bool ok[2]);
};

// ------------------------------------------------------------------ device member tables
// What the kernels ask of the buffers (svx_inflate.hip reads the payloads in words and copies matches 8 bytes at a time):
// every payload padded to 4 bytes, every member's output to 16 with 8 bytes of slack behind its ISIZE bytes.
inline uint64_t padded_payload(uint32_t payload_len) { return ((uint64_t)payload_len + 3) & ~3ull; }
inline uint64_t padded_output(uint32_t isize) { return ((uint64_t)isize + 8 + 15) & ~15ull; }

// The members of one device inflate, in the order they were added: where each payload lies in the file, where it goes in
// the input buffer and where its bytes come out (from `out_base` on), with the three header fields the kernels check.
struct MemberTables {
    std::vector<const uint8_t*> src;
    std::vector<uint64_t> in_off, out_off;
    std::vector<uint32_t> in_len, isize, crc;
    uint64_t in_bytes = 0;  // the input buffer so far
    uint64_t out_end;       // where the next member's output starts

    explicit MemberTables(uint64_t out_base = 0) : out_end(out_base) {}
    uint32_t size() const { return (uint32_t)in_off.size(); }
    void add(const uint8_t* map, uint64_t coff, const Member& m) {
        src.push_back(map + coff + m.payload_off);
        in_off.push_back(in_bytes);
        out_off.push_back(out_end);
        in_len.push_back(m.payload_len);
        isize.push_back(m.isize);
        crc.push_back(m.crc);
        in_bytes += padded_payload(m.payload_len);
        out_end += padded_output(m.isize);
    }
    // as the device sees them: in_off | out_off (u64) | in_len | isize | crc (u32)
    uint64_t bytes() const { return (uint64_t)size() * 28; }
    void write(uint8_t* dst) const {
        const size_t n = size();
        const void* const cols[5] = {in_off.data(), out_off.data(), in_len.data(), isize.data(), crc.data()};
        for (int c = 0; c < 5; ++c) {
            const size_t bytes = n * (c < 2 ? 8 : 4);
            if (bytes) memcpy(dst, cols[c], bytes);
            dst += bytes;
        }
    }
    // members [m0, m1) through `fn`; d_tables: a copy of write()'s bytes on the device (8-byte aligned), d_status and
    // d_ntok: one word per member of the tables, d_tok: token lists for tok_members members at a time.  hipError_t as int.
    int launch(svx_inflate_launch_fn fn, void* stream, const uint8_t* d_in, const uint8_t* d_tables, uint32_t m0, uint32_t m1,
               uint8_t* d_out, uint32_t* d_status, uint32_t* d_ntok, void* d_tok, uint32_t tok_members) const {
        const size_t n = size();
        const uint64_t* const t_in_off = reinterpret_cast<const uint64_t*>(d_tables);
        const uint64_t* const t_out_off = t_in_off + n;
        const uint32_t* const t_in_len = reinterpret_cast<const uint32_t*>(t_out_off + n);
        return fn(stream, d_in, t_in_off + m0, t_in_len + m0, t_in_len + n + m0, t_in_len + 2 * n + m0, m1 - m0, d_out,
                  t_out_off + m0, d_status + m0, d_ntok + m0, d_tok, tok_members);
    }
};

}  // namespace svx_bgzf
