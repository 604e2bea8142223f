// svx_sam_internal.h — what the text front ends of the alignment ingest share: svx_sam.cpp (SAM lines) and svx_paf.cpp
// (PAF rows).  Both fill the columns of a `svx_sam` and hand their gathered CIGAR text to the same two parsers, so the
// record order, the pool in HBM and every message about a CIGAR exist once, in svx_sam.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "svx_sam.h"

namespace svx_samx {

inline int thread_count(int asked) {
    if (asked > 0) return std::min(asked, 64);
    const unsigned hw = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(hw ? hw : 1u, 64u));
}

// fn(i) for i in [0, n) on up to `threads` threads; items are handed out one at a time (records differ 10^5-fold in size)
template <typename F>
void parallel_for(int threads, uint64_t n, F fn) {
    if (n == 0) return;
    const int t = (int)std::min<uint64_t>((uint64_t)std::max(1, threads), n);
    if (t == 1) {
        for (uint64_t i = 0; i < n; ++i) fn(i);
        return;
    }
    std::atomic<uint64_t> next(0);
    std::vector<std::thread> pool;
    for (int k = 0; k < t; ++k)
        pool.emplace_back([&] {
            for (uint64_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
        });
    for (auto& th : pool) th.join();
}

inline bool parse_uint(const char* s, size_t n, uint64_t max, uint64_t* out) {
    if (n == 0 || n > 19) return false;
    uint64_t v = 0;
    for (size_t i = 0; i < n; ++i) {
        if ((uint32_t)(uint8_t)s[i] - '0' >= 10u) return false;
        v = v * 10 + (uint64_t)(s[i] - '0');
    }
    if (v > max) return false;
    *out = v;
    return true;
}

// THE ORDER of svx_sam.h: (tid, pos, reverse-strand flag, place in the file), tid -1 last
inline bool record_before(int32_t tid_a, int32_t pos_a, uint16_t flag_a, uint64_t idx_a, int32_t tid_b, int32_t pos_b, uint16_t flag_b,
                          uint64_t idx_b) {
    const uint32_t ta = (uint32_t)tid_a, tb = (uint32_t)tid_b;  // (-1 as the largest)
    if (ta != tb) return ta < tb;
    if (pos_a != pos_b) return pos_a < pos_b;
    const int ra = (flag_a >> 4) & 1, rb = (flag_b >> 4) & 1;
    if (ra != rb) return ra < rb;
    return idx_a < idx_b;
}

struct Rec {
    uint64_t line_off, file_idx;  // file_idx: (piece << 40 | place in the piece) until the pieces are joined
    uint64_t name_off, cig_off, seq_off, seq_len, aux_off, aux_end;
    uint32_t name_len, cig_len, line_local;  // line_local: place of the line in its piece, later its 1-based number
    int32_t tid, pos;
    uint16_t flag;
    uint8_t mapq;
};

}  // namespace svx_samx

struct svx_sam {
    int fd = -1;
    const char* map = nullptr;
    size_t size = 0;
    size_t body = 0;          // offset of the first line that is no header line
    uint64_t header_lines = 0;
    std::string text;
    std::vector<std::string> ref_name;
    std::vector<int32_t> ref_length;
    std::unordered_map<std::string, int32_t> tid_of;
    int n_threads = 1;
    int pin_device = -1;
    int device_parse = 1;
    int parsed_on_device = 0;
    std::string err;
    // the loaded columns
    uint64_t n = 0;
    std::vector<svx_samx::Rec> recs;  // in the presented order
    std::vector<int32_t> tid, pos, l_seq, ref_len;
    std::vector<uint16_t> flag;
    std::vector<uint8_t> mapq;
    std::vector<uint64_t> cigar_off, name_off, aux_off, voffset;
    std::vector<int64_t> sa_off;
    std::vector<uint32_t> sa_len;
    std::string names;
    std::vector<uint8_t> aux;
    uint32_t* cigar = nullptr;
    bool cigar_pinned = false;
    uint64_t n_ops = 0;
    // device side
    uint32_t* d_cigar = nullptr;
    char* d_tmp = nullptr;
    uint8_t* h_text = nullptr;  // page-locked copy of the gathered text
    bool h_text_pinned = false;
    hipEvent_t ready = nullptr;
    bool d_valid = false;
};

namespace svx_samx {

// What a load does behind its own lines and fields, for a handle whose fixed columns (n, tid .. voffset, names, aux; l_seq
// is what the CIGAR's query length must equal where both are there) are filled in the presented order:
//   begin_load      the device of the handle made current, the last load's pool given back
//   alloc_text      s->h_text for n_text bytes of CIGAR text (page-locked when the device is to read it); false: no memory
//   finish_cigars   the text rec_off[r] .. rec_off[r + 1] of every record -> s->cigar, cigar_off, ref_len, the copy in HBM;
//                   line_of[r]: the 1-based line a message about record r names; seq_what: what l_seq is called there
void begin_load(svx_sam* s);
bool alloc_text(svx_sam* s, uint64_t n_text);
int finish_cigars(svx_sam* s, const std::vector<uint64_t>& rec_off, const std::vector<uint32_t>& line_of, const char* seq_what);
// the 256-entry mapping of a BAM round trip (=ACMGRSVTWYHKDBN, lower case -> upper, anything else -> N)
const uint8_t* bam_alphabet();

}  // namespace svx_samx
