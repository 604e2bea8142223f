// svx_sam.cpp — native SAM ingest (include/svx_sam.h): minimap2's text output, records in any order and without an
// index, into the columns of svx_bam.h.  Replaces `samtools sort` + `samtools index` + pysam.AlignmentFile in front of
// `bam.fetch(contig=...)` (svim-asm:63-72, SVIM_COLLECT.py:65-71) for text input.
//   * the file is memory-mapped; the handle's threads cut it at line ends (memchr) and take the first eleven fields of
//     every line; SEQ / QUAL are hopped over, bases are read from the mapping when svx_sam_seq_slices asks for them
//   * the records are ordered in memory — (tid, pos, reverse flag, place in the file), unplaced last — and every column,
//     pool and offset is laid out in that order
//   * the CIGAR strings of the kept records are gathered back to back and turned into BAM words either by the kernels
//     of svx_cigartext.hip on the pinned device (the pool is then born in HBM and a page-locked copy comes back) or by
//     svx_cigar_text_parse below on the threads (and the pool is uploaded), svx_sam_set_device_parse
// This file also builds alone with a host compiler (tests/native/sam_sanitize.cpp): the kernels are reached through
// pointers that svx_cigartext.hip registers.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "svx_cigartext_dev.h"
#include "svx_sam.h"
#include "svx_sam_internal.h"

namespace {

using namespace svx_samx;

svx_cigar_text_launch_fn g_launch = nullptr;  // svx_cigartext.hip registers its launches when the library loads
svx_cigar_text_ws_fn g_ws_need = nullptr;

inline bool is_digit(uint32_t c) { return c - '0' < 10u; }

// M I D N S H P = X -> 0..8; 15: a letter that is no operator; 14: no letter at all
inline uint32_t op_code(uint32_t c) {
    switch (c) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
        default: break;
    }
    return ((c | 32u) - 'a' < 26u) ? 15u : 14u;
}

// One record's text t[a, b): status; *n_ops and *ref_len of a good record; words written when out != nullptr.
uint32_t parse_one(const uint8_t* t, uint64_t a, uint64_t b, uint32_t* out, uint64_t* n_ops, uint32_t* ref_len) {
    *n_ops = 0;
    *ref_len = 0;
    if (a == b) return SVX_CIGAR_EMPTY_NUMBER;
    if (b - a == 1 && t[a] == '*') return SVX_CIGAR_OK;
    uint64_t n = 0;
    uint32_t v = 0, nd = 0, rl = 0;
    for (uint64_t p = a; p < b; ++p) {
        const uint32_t c = t[p];
        if (is_digit(c)) {
            v = v >= (1u << 28) ? v : v * 10 + (c - '0');  // (stays at or above 2^28 once there)
            ++nd;
            continue;
        }
        if (c == '*') return SVX_CIGAR_BAD_CHAR;
        const uint32_t code = op_code(c);
        if (code == 14) return SVX_CIGAR_BAD_CHAR;
        if (code == 15) return SVX_CIGAR_BAD_OP;
        if (nd == 0) return SVX_CIGAR_EMPTY_NUMBER;
        if (v >= (1u << 28)) return SVX_CIGAR_NUMBER_TOO_BIG;
        if (out) out[n] = (v << 4) | code;
        if ((0x18Du >> code) & 1u) rl += v;
        ++n;
        v = 0;
        nd = 0;
    }
    if (nd) return SVX_CIGAR_TRAILING_DIGITS;
    *n_ops = n;
    *ref_len = rl;
    return SVX_CIGAR_OK;
}

const char* cigar_status_text(uint32_t st) {
    switch (st) {
        case SVX_CIGAR_BAD_CHAR: return "a character that cannot stand in a CIGAR";
        case SVX_CIGAR_BAD_OP: return "an operator outside MIDNSHP=X";
        case SVX_CIGAR_EMPTY_NUMBER: return "an operator without a length";
        case SVX_CIGAR_NUMBER_TOO_BIG: return "a length of 2^28 or more";
        case SVX_CIGAR_TRAILING_DIGITS: return "digits without an operator at its end";
        default: return "malformed";
    }
}

// the 16 letters of BAM's 4-bit codes; everything else reads back as N, lower case as upper
struct SeqMap {
    uint8_t m[256];
    SeqMap() {
        memset(m, 'N', sizeof m);
        for (const char* p = "=ACMGRSVTWYHKDBN"; *p; ++p) {
            m[(uint8_t)*p] = (uint8_t)*p;
            if (*p >= 'A' && *p <= 'Z') m[(uint8_t)(*p + 32)] = (uint8_t)*p;
        }
    }
};
const SeqMap kSeqMap;

struct Piece {
    std::vector<Rec> recs;
    uint64_t n_lines = 0;      // line ends seen in the piece
    int64_t bad_line = -1;     // place (0-based, in the piece) of the first malformed line
    std::string bad_what;
};

bool parse_int(const char* s, size_t n, int64_t lo, int64_t hi, int64_t* out) {
    bool neg = false;
    if (n && (s[0] == '-' || s[0] == '+')) { neg = s[0] == '-'; ++s; --n; }
    uint64_t v;
    if (!parse_uint(s, n, (uint64_t)1 << 40, &v)) return false;
    const int64_t x = neg ? -(int64_t)v : (int64_t)v;
    if (x < lo || x > hi) return false;
    *out = x;
    return true;
}

template <typename T>
void put(std::vector<uint8_t>* out, T v) {
    uint8_t b[sizeof(T)];
    memcpy(b, &v, sizeof(T));
    out->insert(out->end(), b, b + sizeof(T));
}

bool put_typed(std::vector<uint8_t>* out, char type, const char* s, size_t n) {
    if (type == 'f') {
        if (n == 0 || n > 63) return false;
        char buf[64];
        memcpy(buf, s, n);
        buf[n] = 0;
        char* end = nullptr;
        const float f = strtof(buf, &end);
        if (end != buf + n) return false;
        put<float>(out, f);
        return true;
    }
    int64_t x;
    switch (type) {
        case 'c': if (!parse_int(s, n, -128, 127, &x)) return false; put<int8_t>(out, (int8_t)x); return true;
        case 'C': if (!parse_int(s, n, 0, 255, &x)) return false; put<uint8_t>(out, (uint8_t)x); return true;
        case 's': if (!parse_int(s, n, -32768, 32767, &x)) return false; put<int16_t>(out, (int16_t)x); return true;
        case 'S': if (!parse_int(s, n, 0, 65535, &x)) return false; put<uint16_t>(out, (uint16_t)x); return true;
        case 'i': if (!parse_int(s, n, INT32_MIN, INT32_MAX, &x)) return false; put<int32_t>(out, (int32_t)x); return true;
        case 'I': if (!parse_int(s, n, 0, UINT32_MAX, &x)) return false; put<uint32_t>(out, (uint32_t)x); return true;
        default: return false;
    }
}

// The optional fields s[0, n) (tab-separated TAG:TYPE:VALUE) as BAM binary aux appended to *out; *sa_off / *sa_len: the
// SA:Z string inside *out (offset from the vector's start), -1 without one.
bool encode_aux(const char* s, size_t n, std::vector<uint8_t>* out, int64_t* sa_off, uint32_t* sa_len) {
    *sa_off = -1;
    *sa_len = 0;
    size_t at = 0;
    while (at < n) {
        const char* tab = (const char*)memchr(s + at, '\t', n - at);
        const size_t end = tab ? (size_t)(tab - s) : n;
        const char* f = s + at;
        const size_t l = end - at;
        at = end + 1;
        if (l == 0) continue;  // (a trailing tab)
        if (l < 5 || f[2] != ':' || f[4] != ':') return false;
        const char type = f[3];
        const char* v = f + 5;
        const size_t vl = l - 5;
        out->push_back((uint8_t)f[0]);
        out->push_back((uint8_t)f[1]);
        switch (type) {
            case 'A':
                if (vl != 1) return false;
                out->push_back('A');
                out->push_back((uint8_t)v[0]);
                break;
            case 'i': {
                int64_t x;
                if (!parse_int(v, vl, INT32_MIN, UINT32_MAX, &x)) return false;
                // htslib's choice (sam_parse1): the smallest type that holds the value, unsigned for a value >= 0
                const char t = x < 0 ? (x >= -128 ? 'c' : x >= -32768 ? 's' : 'i') : (x <= 255 ? 'C' : x <= 65535 ? 'S' : 'I');
                out->push_back((uint8_t)t);
                if (!put_typed(out, t, v, vl)) return false;
                break;
            }
            case 'f':
                out->push_back('f');
                if (!put_typed(out, 'f', v, vl)) return false;
                break;
            case 'Z':
            case 'H':
                if (memchr(v, 0, vl)) return false;
                out->push_back((uint8_t)type);
                if (type == 'Z' && f[0] == 'S' && f[1] == 'A') { *sa_off = (int64_t)out->size(); *sa_len = (uint32_t)vl; }
                out->insert(out->end(), v, v + vl);
                out->push_back(0);
                break;
            case 'B': {
                if (vl < 1 || !strchr("cCsSiIf", v[0]) || v[0] == 0) return false;
                out->push_back('B');
                out->push_back((uint8_t)v[0]);
                const size_t count_at = out->size();
                put<int32_t>(out, 0);
                int32_t count = 0;
                size_t q = 1;
                while (q < vl) {
                    if (v[q] != ',') return false;
                    ++q;
                    const char* c = (const char*)memchr(v + q, ',', vl - q);
                    const size_t e = c ? (size_t)(c - v) : vl;
                    if (!put_typed(out, v[0], v + q, e - q)) return false;
                    ++count;
                    q = e;
                }
                memcpy(out->data() + count_at, &count, 4);
                break;
            }
            default: return false;
        }
    }
    return true;
}

std::mutex g_stream_mu;
hipStream_t g_stream[64] = {};  // one per device for all handles, never destroyed (a stream's creation costs milliseconds)

hipStream_t device_stream(int device) {
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(g_stream_mu);
    if (!g_stream[device]) {
        if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&g_stream[device], hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            g_stream[device] = nullptr;
        }
    }
    return g_stream[device];
}

}  // namespace

namespace {

int fail(svx_sam* s, int rc, const std::string& what) {
    s->err = what;
    return rc;
}

void release_pool(svx_sam* s) {
    if (s->d_valid && s->ready) (void)hipEventSynchronize(s->ready);
    s->d_valid = false;
    if (s->cigar) {
        if (s->cigar_pinned) (void)hipHostFree(s->cigar);
        else free(s->cigar);
    }
    s->cigar = nullptr;
    s->cigar_pinned = false;
    if (s->d_cigar) (void)hipFree(s->d_cigar);
    s->d_cigar = nullptr;
    if (s->d_tmp) (void)hipFree(s->d_tmp);
    s->d_tmp = nullptr;
    if (s->h_text) {
        if (s->h_text_pinned) (void)hipHostFree(s->h_text);
        else free(s->h_text);
    }
    s->h_text = nullptr;
    (void)hipGetLastError();
    s->n_ops = 0;
}

// One line [a, e) (no line end, no '\r'): false with *what set when it is malformed.
bool parse_line(const svx_sam* s, uint64_t a, uint64_t e, Rec* r, std::string* what) {
    const char* m = s->map;
    uint64_t f[12];  // starts of fields 0..10, f[11]: one behind the tab that ends field 10 (or e + 1)
    f[0] = a;
    uint64_t at = a;
    for (int k = 1; k <= 11; ++k) {
        const char* tab = at < e ? (const char*)memchr(m + at, '\t', e - at) : nullptr;
        if (!tab) {
            if (k == 11) { f[11] = e + 1; break; }
            *what = "fewer than 11 fields";
            return false;
        }
        at = (uint64_t)(tab - m) + 1;
        f[k] = at;
    }
    auto len = [&](int k) { return f[k + 1] - 1 - f[k]; };
    uint64_t v;
    r->line_off = a;
    r->name_off = f[0];
    r->name_len = (uint32_t)std::min<uint64_t>(len(0), 0xFFFFFFFFu);
    if (!parse_uint(m + f[1], len(1), 65535, &v)) { *what = "FLAG is not a number in 0..65535"; return false; }
    r->flag = (uint16_t)v;
    if (len(2) == 1 && m[f[2]] == '*') {
        r->tid = -1;
    } else {
        auto it = s->tid_of.find(std::string(m + f[2], len(2)));
        if (it == s->tid_of.end()) { *what = "RNAME '" + std::string(m + f[2], std::min<uint64_t>(len(2), 80)) + "' is not in the @SQ lines"; return false; }
        r->tid = it->second;
    }
    if (!parse_uint(m + f[3], len(3), 0x7FFFFFFFu, &v)) { *what = "POS is not a number in 0..2^31-1"; return false; }
    r->pos = (int32_t)v - 1;
    if (!parse_uint(m + f[4], len(4), 255, &v)) { *what = "MAPQ is not a number in 0..255"; return false; }
    r->mapq = (uint8_t)v;
    if (len(5) > 0xFFFFFFFFull) { *what = "CIGAR longer than 4 GiB"; return false; }
    r->cig_off = f[5];
    r->cig_len = (uint32_t)len(5);
    r->seq_off = f[9];
    r->seq_len = (len(9) == 1 && m[f[9]] == '*') ? 0 : len(9);
    if (r->seq_len > 0x7FFFFFFFull) { *what = "SEQ longer than 2^31-1 bases"; return false; }
    r->aux_off = std::min(f[11], e);
    r->aux_end = e;
    return true;
}

void scan_piece(const svx_sam* s, uint64_t a, uint64_t b, uint64_t piece, Piece* out) {
    const char* m = s->map;
    while (a < b) {
        const char* nl = (const char*)memchr(m + a, '\n', b - a);
        uint64_t e = nl ? (uint64_t)(nl - m) : b;
        const uint64_t next = e + 1;
        if (e > a && m[e - 1] == '\r') --e;
        if (e > a) {
            Rec r;
            std::string what;
            if (!parse_line(s, a, e, &r, &what)) {
                if (out->bad_line < 0) { out->bad_line = (int64_t)out->n_lines; out->bad_what = what; }
            } else {
                r.line_local = (uint32_t)out->n_lines;
                r.file_idx = (piece << 40) | out->recs.size();
                out->recs.push_back(r);
            }
        }
        ++out->n_lines;
        a = next;
    }
}

}  // namespace

extern "C" void svx_sam_register_device_parser(svx_cigar_text_launch_fn launch, svx_cigar_text_ws_fn ws) {
    g_launch = launch;
    g_ws_need = ws;
}

extern "C" int svx_cigar_text_parse(const uint8_t* text, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, uint32_t* words,
                                    uint64_t cap, uint64_t* cigar_off, int32_t* ref_len, uint32_t* status, int n_threads) {
    if (!rec_off || !cigar_off || (n_bytes && !text) || (n_rec && (!ref_len || !status)) || (cap && !words)) return SVX_E_INVALID;
    if (cap < n_bytes / 2) return SVX_E_INVALID;
    if (rec_off[0] != 0 || rec_off[n_rec] != n_bytes) return SVX_E_INVALID;
    for (uint32_t r = 0; r < n_rec; ++r)
        if (rec_off[r] > rec_off[r + 1]) return SVX_E_INVALID;
    const int t = thread_count(n_threads);
    std::vector<uint64_t> n_ops(n_rec);
    parallel_for(t, n_rec, [&](uint64_t r) {
        uint32_t rl;
        status[r] = parse_one(text, rec_off[r], rec_off[r + 1], nullptr, &n_ops[r], &rl);
        ref_len[r] = (int32_t)rl;
    });
    cigar_off[0] = 0;
    for (uint32_t r = 0; r < n_rec; ++r) cigar_off[r + 1] = cigar_off[r] + n_ops[r];
    if (cigar_off[n_rec] > cap) return SVX_E_CAPACITY;
    parallel_for(t, n_rec, [&](uint64_t r) {
        if (status[r] != SVX_CIGAR_OK || n_ops[r] == 0) return;
        uint64_t n;
        uint32_t rl;
        (void)parse_one(text, rec_off[r], rec_off[r + 1], words + cigar_off[r], &n, &rl);
    });
    return SVX_OK;
}

extern "C" int svx_sam_open(const char* path, int n_threads, svx_sam** out, char* err, size_t err_cap) {
    auto refuse = [&](int rc, const std::string& m) {
        if (err && err_cap) snprintf(err, err_cap, "%s", m.c_str());
        if (out) *out = nullptr;
        return rc;
    };
    if (!path || !out) return refuse(SVX_E_INVALID, "svx_sam_open: null argument");
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return refuse(SVX_E_INVALID, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
        close(fd);
        return refuse(SVX_E_INVALID, std::string(path) + " is not a regular file");
    }
    svx_sam* s = new svx_sam();
    s->fd = fd;
    s->size = (size_t)st.st_size;
    s->n_threads = thread_count(n_threads);
    if (s->size) {
        void* p = mmap(nullptr, s->size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) {
            close(fd);
            delete s;
            return refuse(SVX_E_NOMEM, std::string("cannot map ") + path);
        }
        s->map = (const char*)p;
    }
    auto bail = [&](const std::string& m) {
        svx_sam_close(s);
        return refuse(SVX_E_INVALID, m);
    };
    if (s->size >= 2 && (uint8_t)s->map[0] == 0x1f && (uint8_t)s->map[1] == 0x8b)
        return bail(std::string(path) + " is gzip- or bgzip-compressed: alignments are read from an uncompressed SAM or from a BAM");
    // header: every leading line that starts with '@'
    size_t at = 0;
    while (at < s->size && s->map[at] == '@') {
        const char* nl = (const char*)memchr(s->map + at, '\n', s->size - at);
        const size_t next = nl ? (size_t)(nl - s->map) + 1 : s->size;
        size_t e = nl ? next - 1 : s->size;
        if (e > at && s->map[e - 1] == '\r') --e;
        if (e - at >= 3 && memcmp(s->map + at, "@SQ", 3) == 0 && (e - at == 3 || s->map[at + 3] == '\t')) {
            std::string name;
            int64_t length = -1;
            size_t q = at + 3;
            while (q < e) {
                ++q;  // the tab
                const char* tab = (const char*)memchr(s->map + q, '\t', e - q);
                const size_t fe = tab ? (size_t)(tab - s->map) : e;
                if (fe - q >= 3 && s->map[q + 2] == ':') {
                    if (s->map[q] == 'S' && s->map[q + 1] == 'N') name.assign(s->map + q + 3, fe - q - 3);
                    else if (s->map[q] == 'L' && s->map[q + 1] == 'N' && !parse_int(s->map + q + 3, fe - q - 3, 0, INT32_MAX, &length)) length = -1;
                }
                q = fe;
            }
            if (name.empty() || length < 0) return bail(std::string(path) + ": @SQ line " + std::to_string(s->header_lines + 1) + " lacks SN or a valid LN");
            if (s->tid_of.count(name)) return bail(std::string(path) + ": @SQ name '" + name + "' appears twice");
            s->tid_of[name] = (int32_t)s->ref_name.size();
            s->ref_name.push_back(name);
            s->ref_length.push_back((int32_t)length);
        }
        s->text.append(s->map + at, e - at);
        s->text.push_back('\n');
        ++s->header_lines;
        at = next;
    }
    s->body = at;
    if (s->ref_name.empty())
        return bail(std::string(path) + " is not a SAM file with a reference dictionary: it has no @SQ header lines (minimap2 -a writes them; "
                                        "BAM input is recognised by its gzip magic)");
    *out = s;
    return SVX_OK;
}

extern "C" void svx_sam_close(svx_sam* s) {
    if (!s) return;
    if (s->pin_device >= 0 && (s->cigar_pinned || s->d_cigar || s->d_tmp || s->h_text_pinned)) {
        if (hipSetDevice(s->pin_device) != hipSuccess) (void)hipGetLastError();
    }
    release_pool(s);
    if (s->ready) { (void)hipEventDestroy(s->ready); (void)hipGetLastError(); }
    if (s->map) munmap((void*)s->map, s->size);
    if (s->fd >= 0) close(s->fd);
    delete s;
}

extern "C" const char* svx_sam_last_error(const svx_sam* s) { return s ? s->err.c_str() : "null handle"; }

extern "C" int svx_sam_header(const svx_sam* s, const char** text, uint64_t* l_text, int32_t* n_ref) {
    if (!s) return SVX_E_INVALID;
    if (text) *text = s->text.data();
    if (l_text) *l_text = s->text.size();
    if (n_ref) *n_ref = (int32_t)s->ref_name.size();
    return SVX_OK;
}

extern "C" int svx_sam_reference(const svx_sam* s, int32_t tid, const char** name, int32_t* length) {
    if (!s || tid < 0 || (size_t)tid >= s->ref_name.size()) return SVX_E_INVALID;
    if (name) *name = s->ref_name[(size_t)tid].c_str();
    if (length) *length = s->ref_length[(size_t)tid];
    return SVX_OK;
}

extern "C" int svx_sam_set_pinned_device(svx_sam* s, int device) {
    if (!s) return SVX_E_INVALID;
    s->pin_device = device < 0 ? -1 : device;
    return SVX_OK;
}

extern "C" int svx_sam_set_device_parse(svx_sam* s, int on) {
    if (!s) return SVX_E_INVALID;
    s->device_parse = on ? 1 : 0;
    return SVX_OK;
}

extern "C" int svx_sam_parsed_on_device(const svx_sam* s) { return s ? s->parsed_on_device : 0; }

namespace {

// The device's turn: text and offsets up, the kernels, offsets / ref_len / status back, then the words into a page-locked
// pool of exactly their size.  false: nothing of it is left behind and the threads take over.
bool parse_on_device(svx_sam* s, uint64_t n_text, const std::vector<uint64_t>& rec_off, std::vector<uint32_t>* status) {
    if (!g_launch || !g_ws_need || s->pin_device < 0 || !s->h_text_pinned) return false;
    hipStream_t st = device_stream(s->pin_device);
    if (!st || hipSetDevice(s->pin_device) != hipSuccess) { (void)hipGetLastError(); return false; }
    const uint64_t n = s->n;
    const uint64_t cap = n_text / 2 + 1;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_text = 0, o_rec = up(n_text + 1), o_coff = o_rec + up((n + 1) * 8), o_rl = o_coff + up((n + 1) * 8),
                 o_st = o_rl + up((n + 1) * 4), o_ws = o_st + up((n + 1) * 4), total = o_ws + g_ws_need(n_text, (uint32_t)n) + 256;
    bool ok = hipMalloc((void**)&s->d_tmp, total) == hipSuccess && hipMalloc((void**)&s->d_cigar, cap * 4) == hipSuccess;
    if (ok && !s->ready) ok = hipEventCreateWithFlags(&s->ready, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMemcpyAsync(s->d_tmp + o_text, s->h_text, n_text, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(s->d_tmp + o_rec, rec_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && g_launch(st, (const uint8_t*)(s->d_tmp + o_text), n_text, (const uint64_t*)(s->d_tmp + o_rec), (uint32_t)n, s->d_cigar, cap,
                        (uint64_t*)(s->d_tmp + o_coff), (int32_t*)(s->d_tmp + o_rl), (uint32_t*)(s->d_tmp + o_st), s->d_tmp + o_ws) == 0;
    ok = ok && hipEventRecord(s->ready, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(s->cigar_off.data(), s->d_tmp + o_coff, (n + 1) * 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipMemcpyAsync(s->ref_len.data(), s->d_tmp + o_rl, n * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipMemcpyAsync(status->data(), s->d_tmp + o_st, n * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
    if (ok) {
        s->n_ops = s->cigar_off[n];
        ok = s->n_ops <= cap;
        if (ok && s->n_ops) {
            ok = hipHostMalloc((void**)&s->cigar, s->n_ops * 4, hipHostMallocDefault) == hipSuccess;
            s->cigar_pinned = ok;
            ok = ok && hipMemcpyAsync(s->cigar, s->d_cigar, s->n_ops * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipStreamSynchronize(st) == hipSuccess;
        }
    }
    if (!ok) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
        uint8_t* keep = s->h_text;  // (the gathered text is still needed)
        const bool keep_pinned = s->h_text_pinned;
        s->h_text = nullptr;
        release_pool(s);
        s->h_text = keep;
        s->h_text_pinned = keep_pinned;
        return false;
    }
    s->d_valid = s->n_ops != 0;
    return true;
}

}  // namespace

extern "C" int svx_sam_load(svx_sam* s, const int32_t* tids, int32_t n_tids) {
    if (!s || (n_tids > 0 && !tids) || n_tids < 0) return SVX_E_INVALID;
    begin_load(s);
    const size_t n_ref = s->ref_name.size();
    std::vector<uint8_t> want;
    if (tids) {
        want.assign(n_ref, 0);
        for (int32_t k = 0; k < n_tids; ++k) {
            if (tids[k] < 0 || (size_t)tids[k] >= n_ref) return fail(s, SVX_E_INVALID, "svx_sam_load: contig id out of range");
            want[(size_t)tids[k]] = 1;
        }
    }
    // 1. lines and fields: pieces of the mapping cut at line ends
    const uint64_t body_bytes = s->size - s->body;
    const uint64_t n_pieces = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)s->n_threads * 4, body_bytes >> 16));
    std::vector<uint64_t> cut(n_pieces + 1, s->size);
    cut[0] = s->body;
    for (uint64_t k = 1; k < n_pieces; ++k) {
        uint64_t at = std::max(cut[k - 1], s->body + body_bytes / n_pieces * k);
        const char* nl = at < s->size ? (const char*)memchr(s->map + at, '\n', s->size - at) : nullptr;
        cut[k] = nl ? (uint64_t)(nl - s->map) + 1 : s->size;
    }
    std::vector<Piece> pieces(n_pieces);
    parallel_for(s->n_threads, n_pieces, [&](uint64_t k) { scan_piece(s, cut[k], cut[k + 1], k, &pieces[k]); });
    uint64_t lines_before = s->header_lines, n_all = 0;
    std::vector<uint64_t> first_line(n_pieces), first_rec(n_pieces);
    for (uint64_t k = 0; k < n_pieces; ++k) {
        if (pieces[k].bad_line >= 0)
            return fail(s, SVX_E_INVALID, "line " + std::to_string(lines_before + (uint64_t)pieces[k].bad_line + 1) + ": " + pieces[k].bad_what);
        first_line[k] = lines_before;
        first_rec[k] = n_all;
        lines_before += pieces[k].n_lines;
        n_all += pieces[k].recs.size();
    }
    // 2. the kept records in the presented order
    std::vector<Rec>& recs = s->recs;
    recs.clear();
    recs.reserve(n_all);
    for (uint64_t k = 0; k < n_pieces; ++k)
        for (const Rec& r0 : pieces[k].recs) {
            if (tids && (r0.tid < 0 || !want[(size_t)r0.tid])) continue;
            Rec r = r0;
            r.file_idx = first_rec[k] + (r0.file_idx & ((1ull << 40) - 1));
            r.line_local = (uint32_t)std::min<uint64_t>(first_line[k] + r0.line_local + 1, 0xFFFFFFFFu);  // from here on: the 1-based line
            recs.push_back(r);
        }
    pieces.clear();
    std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) {
        return record_before(a.tid, a.pos, a.flag, a.file_idx, b.tid, b.pos, b.flag, b.file_idx);
    });
    const uint64_t n = s->n = recs.size();
    if (n >= 0xFFFFFFFFull) return fail(s, SVX_E_TOO_LARGE, "more than 2^32 - 2 records");
    // 3. fixed columns, names, aux
    s->tid.resize(n); s->pos.resize(n); s->l_seq.resize(n); s->ref_len.assign(n, 0); s->flag.resize(n); s->mapq.resize(n);
    s->voffset.resize(n); s->sa_off.resize(n); s->sa_len.resize(n);
    s->cigar_off.assign(n + 1, 0); s->name_off.assign(n + 1, 0); s->aux_off.assign(n + 1, 0);
    s->names.clear();
    s->aux.clear();
    std::vector<uint64_t> rec_off(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        const Rec& r = recs[i];
        s->tid[i] = r.tid; s->pos[i] = r.pos; s->l_seq[i] = (int32_t)r.seq_len; s->flag[i] = r.flag; s->mapq[i] = r.mapq;
        s->voffset[i] = r.line_off;
        s->names.append(s->map + r.name_off, r.name_len);
        s->name_off[i + 1] = s->names.size();
        int64_t so;
        uint32_t sl;
        if (!encode_aux(s->map + r.aux_off, r.aux_end - r.aux_off, &s->aux, &so, &sl))
            return fail(s, SVX_E_INVALID, "line " + std::to_string(r.line_local) + ": an optional field is not TAG:TYPE:VALUE of a type the SAM format defines");
        s->sa_off[i] = so;
        s->sa_len[i] = sl;
        s->aux_off[i + 1] = s->aux.size();
        rec_off[i + 1] = rec_off[i] + r.cig_len;
    }
    // 4. the CIGAR strings back to back, then their words
    if (!alloc_text(s, rec_off[n])) return fail(s, SVX_E_NOMEM, "no memory for the CIGAR text");
    parallel_for(s->n_threads, n, [&](uint64_t i) { memcpy(s->h_text + rec_off[i], s->map + recs[i].cig_off, recs[i].cig_len); });
    std::vector<uint32_t> line_of(n);
    for (uint64_t i = 0; i < n; ++i) line_of[i] = recs[i].line_local;
    return finish_cigars(s, rec_off, line_of, "the length of SEQ");
}

namespace svx_samx {

const uint8_t* bam_alphabet() { return kSeqMap.m; }

void begin_load(svx_sam* s) {
    if (s->pin_device >= 0 && hipSetDevice(s->pin_device) != hipSuccess) (void)hipGetLastError();
    release_pool(s);
    s->n = 0;
    s->parsed_on_device = 0;
}

// (page-locked when the device is to read the text)
bool alloc_text(svx_sam* s, uint64_t n_text) {
    const bool want_device = s->pin_device >= 0 && s->device_parse && g_launch && n_text > 0;
    if (want_device && hipHostMalloc((void**)&s->h_text, n_text + 1, hipHostMallocDefault) == hipSuccess) {
        s->h_text_pinned = true;
    } else {
        (void)hipGetLastError();
        s->h_text = (uint8_t*)malloc(n_text + 1);
        s->h_text_pinned = false;
    }
    return s->h_text != nullptr;
}

int finish_cigars(svx_sam* s, const std::vector<uint64_t>& rec_off, const std::vector<uint32_t>& line_of, const char* seq_what) {
    const uint64_t n = s->n;
    const uint64_t n_text = rec_off[n];
    const bool want_device = s->h_text_pinned;
    std::vector<uint32_t> status(n, 0);
    if (want_device && parse_on_device(s, n_text, rec_off, &status)) {
        s->parsed_on_device = 1;
    } else {
        std::vector<uint64_t> n_ops(n);
        parallel_for(s->n_threads, n, [&](uint64_t r) {
            uint32_t rl;
            status[r] = parse_one(s->h_text, rec_off[r], rec_off[r + 1], nullptr, &n_ops[r], &rl);
            s->ref_len[r] = (int32_t)rl;
        });
        for (uint64_t r = 0; r < n; ++r) s->cigar_off[r + 1] = s->cigar_off[r] + n_ops[r];
        s->n_ops = s->cigar_off[n];
        if (s->n_ops) {
            if (s->pin_device >= 0 && hipSetDevice(s->pin_device) == hipSuccess &&
                hipHostMalloc((void**)&s->cigar, s->n_ops * 4, hipHostMallocDefault) == hipSuccess) {
                s->cigar_pinned = true;
            } else {
                (void)hipGetLastError();
                s->cigar = (uint32_t*)malloc(s->n_ops * 4);
                if (!s->cigar) return fail(s, SVX_E_NOMEM, "no memory for the CIGAR pool");
            }
        }
        parallel_for(s->n_threads, n, [&](uint64_t r) {
            if (status[r] != SVX_CIGAR_OK || n_ops[r] == 0) return;
            uint64_t k;
            uint32_t rl;
            (void)parse_one(s->h_text, rec_off[r], rec_off[r + 1], s->cigar + s->cigar_off[r], &k, &rl);
        });
    }
    for (uint64_t r = 0; r < n; ++r)
        if (status[r] != SVX_CIGAR_OK) {
            const uint32_t st = status[r];
            const uint32_t line = line_of[r];
            release_pool(s);
            s->n = 0;
            return fail(s, SVX_E_INVALID, "line " + std::to_string(line) + ": the CIGAR has " + cigar_status_text(st));
        }
    // query-consuming length against SEQ where both are present
    std::atomic<int64_t> bad(-1);
    parallel_for(s->n_threads, n, [&](uint64_t r) {
        if (s->l_seq[r] == 0 || s->cigar_off[r + 1] == s->cigar_off[r]) return;
        uint64_t q = 0;
        for (uint64_t k = s->cigar_off[r]; k < s->cigar_off[r + 1]; ++k)
            if ((0x193u >> (s->cigar[k] & 15)) & 1u) q += s->cigar[k] >> 4;  // M I S = X
        if (q != (uint64_t)s->l_seq[r]) {
            int64_t none = -1;
            bad.compare_exchange_strong(none, (int64_t)r);
        }
    });
    if (bad.load() >= 0) {
        const uint32_t line = line_of[(size_t)bad.load()];
        release_pool(s);
        s->n = 0;
        return fail(s, SVX_E_INVALID, "line " + std::to_string(line) + ": the CIGAR's query length differs from " + seq_what);
    }
    // the threads' pool goes up to where svx_collect_batch wants it
    if (!s->parsed_on_device && s->cigar_pinned && s->n_ops) {
        hipStream_t st = device_stream(s->pin_device);
        bool ok = st != nullptr && hipMalloc((void**)&s->d_cigar, s->n_ops * 4) == hipSuccess;
        if (ok && !s->ready) ok = hipEventCreateWithFlags(&s->ready, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipMemcpyAsync(s->d_cigar, s->cigar, s->n_ops * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipEventRecord(s->ready, st) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (st) (void)hipStreamSynchronize(st);
            if (s->d_cigar) (void)hipFree(s->d_cigar);
            (void)hipGetLastError();
            s->d_cigar = nullptr;
        }
        s->d_valid = ok;
    }
    if (s->h_text && !s->h_text_pinned) { free(s->h_text); s->h_text = nullptr; }  // (a page-locked one waits for close: freeing it waits for the device)
    return SVX_OK;
}

}  // namespace svx_samx

extern "C" int svx_sam_get_columns(const svx_sam* s, svx_bam_columns* c) {
    if (!s || !c) return SVX_E_INVALID;
    memset(c, 0, sizeof *c);
    c->n_records = s->n;
    c->tid = s->tid.data(); c->pos = s->pos.data(); c->l_seq = s->l_seq.data(); c->ref_len = s->ref_len.data();
    c->flag = s->flag.data(); c->mapq = s->mapq.data(); c->cigar_off = s->cigar_off.data(); c->cigar = s->cigar;
    c->name_off = s->name_off.data(); c->names = s->names.data(); c->aux_off = s->aux_off.data(); c->aux = s->aux.data();
    c->sa_off = s->sa_off.data(); c->sa_len = s->sa_len.data(); c->voffset = s->voffset.data();
    c->cigar_pinned = s->cigar_pinned ? 1 : 0;
    c->n_threads = s->n_threads;
    return SVX_OK;
}

extern "C" int svx_sam_seq_slices(svx_sam* s, const uint32_t* rec, const uint32_t* begin, const uint32_t* end, uint32_t n,
                                  const uint64_t* out_off, uint8_t* out) {
    if (!s) return SVX_E_INVALID;
    if (n == 0) return SVX_OK;
    if (!rec || !begin || !end || !out_off || !out) return fail(s, SVX_E_INVALID, "svx_sam_seq_slices: null argument");
    std::atomic<bool> failed(false);
    const uint64_t n_jobs = (n + 255) / 256;
    parallel_for(s->n_threads, n_jobs, [&](uint64_t j) {
        for (uint64_t i = j * 256; i < std::min<uint64_t>((j + 1) * 256, n); ++i) {
            if (rec[i] >= s->n) { failed.store(true); return; }
            const Rec& r = s->recs[rec[i]];
            const uint64_t a = std::min<uint64_t>(begin[i], r.seq_len), b = std::max(a, std::min<uint64_t>(end[i], r.seq_len));
            if (out_off[i + 1] < out_off[i] || out_off[i + 1] - out_off[i] < b - a) { failed.store(true); return; }
            const uint8_t* src = (const uint8_t*)s->map + r.seq_off + a;
            uint8_t* dst = out + out_off[i];
            for (uint64_t k = 0; k < b - a; ++k) dst[k] = kSeqMap.m[src[k]];
        }
    });
    if (failed.load()) return fail(s, SVX_E_INVALID, "svx_sam_seq_slices: bad slice bounds");
    return SVX_OK;
}

extern "C" int svx_sam_device_pool(svx_sam* s, const uint32_t** d_cigar, uint64_t* n_ops, void** ready) {
    if (!s) return SVX_E_INVALID;
    if (d_cigar) *d_cigar = s->d_valid ? s->d_cigar : nullptr;
    if (n_ops) *n_ops = s->d_valid ? s->n_ops : 0;
    if (ready) *ready = s->d_valid ? (void*)s->ready : nullptr;
    return SVX_OK;
}

extern "C" int svx_sam_device_pool_wait(svx_sam* s, double* waited_us) {
    if (!s) return SVX_E_INVALID;
    if (waited_us) *waited_us = 0;
    if (!s->d_valid) return SVX_OK;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipEventSynchronize(s->ready) != hipSuccess) {
        (void)hipGetLastError();
        return fail(s, SVX_E_HIP, "svx_sam_device_pool_wait: the CIGAR pool's copy in HBM failed");
    }
    if (waited_us) *waited_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return SVX_OK;
}
