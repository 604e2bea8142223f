// svx_textaln.h — what the text front ends of the alignment ingest share: svx_sam.cpp (SAM lines) and svx_paf.cpp (PAF
// rows).  A front end says "here are my rows, in order, with their CIGAR text" and gets columns, a pool and a copy in HBM:
//   MappedText   the memory-mapped file
//   scan_lines   the mapping cut at line ends, the pieces parsed on the handle's threads, the rows joined in file order
//   Columns      what a load produces and owns: the columns of svx_bam.h, the CIGAR pool, its copy in HBM, the error text
// The record order, the two CIGAR parsers and every message about a CIGAR exist once, in svx_textaln.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "svx_bam.h"

namespace svx_textaln {

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

struct MappedText {
    int fd = -1;
    const char* map = nullptr;
    size_t size = 0;
    // What open() found; the front end words the refusal.  GZIP: the file is open and mapped, its first bytes are gzip's.
    enum Found { OK, CANNOT_OPEN, NOT_REGULAR, CANNOT_MAP, GZIP };
    Found open(const char* path);
    void close();
    MappedText() = default;
    MappedText(const MappedText&) = delete;
    ~MappedText() { close(); }
};

// What the scanner fills in of every row; a front end's row type derives from it.
struct Line {
    uint64_t line_off;  // byte offset of the line in the file
    uint64_t file_idx;  // place among all rows of the file
    uint32_t line;      // 1-based line number (place of the line in its piece until the pieces are joined)
};

template <typename R>
struct Piece {
    std::vector<R> rows;
    uint64_t n_lines = 0;   // line ends seen in the piece
    int64_t bad_line = -1;  // place (0-based, in the piece) of the first malformed line
    std::string bad_what;
};

// The lines of m[a, b): a '\r' in front of the line end dropped, empty lines counted and skipped,
// parse(start, end, &row, &what) for every other one.
template <typename R, typename Parse>
void scan_piece(const char* m, uint64_t a, uint64_t b, Parse& parse, Piece<R>* out) {
    while (a < b) {
        const char* nl = (const char*)memchr(m + a, '\n', b - a);
        uint64_t e = nl ? (uint64_t)(nl - m) : b;
        const uint64_t next = e + 1;
        if (e > a && m[e - 1] == '\r') --e;
        if (e > a) {
            R r;
            std::string what;
            if (!parse(a, e, &r, &what)) {
                if (out->bad_line < 0) { out->bad_line = (int64_t)out->n_lines; out->bad_what = what; }
            } else {
                r.line_off = a;
                r.line = (uint32_t)out->n_lines;
                out->rows.push_back(r);
            }
        }
        ++out->n_lines;
        a = next;
    }
}

// Every row of t[body, size) in file order into *rows, `lines_before` lines in front of `body`.  false: *err is
// "line N: what" for the first malformed line in file order.
template <typename R, typename Parse>
bool scan_lines(const MappedText& t, uint64_t body, uint64_t lines_before, int n_threads, Parse parse, std::vector<R>* rows, std::string* err) {
    rows->clear();
    const uint64_t bytes = t.size - body;
    const uint64_t n_pieces = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_threads * 4, bytes >> 16));
    std::vector<uint64_t> cut(n_pieces + 1, t.size);
    cut[0] = body;
    for (uint64_t k = 1; k < n_pieces; ++k) {
        const uint64_t at = std::max(cut[k - 1], body + bytes / n_pieces * k);
        const char* nl = at < t.size ? (const char*)memchr(t.map + at, '\n', t.size - at) : nullptr;
        cut[k] = nl ? (uint64_t)(nl - t.map) + 1 : t.size;
    }
    std::vector<Piece<R>> pieces(n_pieces);
    parallel_for(n_threads, n_pieces, [&](uint64_t k) { scan_piece(t.map, cut[k], cut[k + 1], parse, &pieces[k]); });
    uint64_t n_all = 0, first_line = lines_before;
    for (const Piece<R>& p : pieces) {
        if (p.bad_line >= 0) {
            *err = "line " + std::to_string(first_line + (uint64_t)p.bad_line + 1) + ": " + p.bad_what;
            return false;
        }
        first_line += p.n_lines;
        n_all += p.rows.size();
    }
    rows->reserve(n_all);
    for (const Piece<R>& p : pieces) {
        for (const R& r : p.rows) {
            rows->push_back(r);
            rows->back().file_idx = rows->size() - 1;
            rows->back().line = (uint32_t)std::min<uint64_t>(lines_before + r.line + 1, 0xFFFFFFFFu);
        }
        lines_before += p.n_lines;
    }
    return true;
}

// What a load produces and owns.  A front end fills the fixed columns in the presented order (after resize: tid .. voffset,
// names, aux; l_seq is what the CIGAR's query length must equal where both are there), gathers the CIGAR text of the records
// back to back in h_text and calls finish_cigars.  A failure leaves its message in `err`, the handle's one error text.
struct Columns {
    int n_threads = 1;
    int pin_device = -1;
    int device_parse = 1;
    int parsed_on_device = 0;
    std::string err;
    uint64_t n = 0;
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

    Columns() = default;
    Columns(const Columns&) = delete;
    ~Columns();  // the pool, its copy in HBM, the event

    int fail(int rc, const std::string& what) { err = what; return rc; }
    void begin_load();               // the handle's device made current, the last load's pool given back, n = 0
    void resize(uint64_t n_records);  // n and every column sized for it, the offsets zero, names and aux empty
    bool alloc_text(uint64_t n_text);  // h_text for n_text bytes (page-locked when the device is to read it); false: no memory
    // the text rec_off[r] .. rec_off[r + 1] of every record -> cigar, cigar_off, ref_len, the copy in HBM;
    // line_of[r]: the 1-based line a message about record r names; seq_what: what l_seq is called there
    int finish_cigars(const std::vector<uint64_t>& rec_off, const std::vector<uint32_t>& line_of, const char* seq_what);
    void release_pool();
    int get_columns(svx_bam_columns* out) const;
    int device_pool(const uint32_t** d_cigar_out, uint64_t* n_ops_out, void** ready_out) const;
    int device_pool_wait(double* waited_us);
};

// the 256-entry mapping of a BAM round trip (=ACMGRSVTWYHKDBN, lower case -> upper, anything else -> N)
const uint8_t* bam_alphabet();

}  // namespace svx_textaln
