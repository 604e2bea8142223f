// svx_sam.cpp — native SAM ingest (include/svx_sam.h): minimap2's text output, records in any order and without an
// index, into the columns of svx_bam.h.  Replaces `samtools sort` + `samtools index` + pysam.AlignmentFile in front of
// `bam.fetch(contig=...)` (svim-asm:63-72, SVIM_COLLECT.py:65-71) for text input.  A front end of svx_textaln.h:
//   * the file is memory-mapped (MappedText); scan_lines cuts it at line ends on the handle's threads and parse_line
//     takes the first eleven fields of every line; SEQ / QUAL are hopped over, bases are read from the mapping when
//     svx_sam_seq_slices asks for them
//   * the records are ordered in memory — (tid, pos, reverse flag, place in the file), unplaced last — and every column,
//     pool and offset is laid out in that order
//   * the CIGAR strings of the kept records are gathered back to back and handed to Columns::finish_cigars: device
//     kernels or threads, pool in HBM, messages — nothing of it is restated here
// This file also builds alone with a host compiler, beside svx_textaln.cpp (tests/native/sam_sanitize.cpp).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <unordered_map>
#include <vector>

#include "svx_sam.h"
#include "svx_textaln.h"

using namespace svx_textaln;

namespace {

struct Rec : Line {
    uint64_t name_off, cig_off, seq_off, seq_len, aux_off, aux_end;
    uint32_t name_len, cig_len;
    int32_t tid, pos;
    uint16_t flag;
    uint8_t mapq;
};

}  // namespace

struct svx_sam {
    MappedText file;
    size_t body = 0;  // offset of the first line that is no header line
    uint64_t header_lines = 0;
    std::string text;
    std::vector<std::string> ref_name;
    std::vector<int32_t> ref_length;
    std::unordered_map<std::string, int32_t> tid_of;
    std::vector<Rec> recs;  // the loaded records in the presented order
    Columns c;
};

namespace {

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

// One line [a, e) (no line end, no '\r'): false with *what set when it is malformed.
bool parse_line(const svx_sam* s, uint64_t a, uint64_t e, Rec* r, std::string* what) {
    const char* m = s->file.map;
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

}  // namespace
extern "C" int svx_sam_open(const char* path, int n_threads, svx_sam** out, char* err, size_t err_cap) {
    svx_sam* s = nullptr;
    auto refuse = [&](int rc, const std::string& m) {
        delete s;
        if (err && err_cap) snprintf(err, err_cap, "%s", m.c_str());
        if (out) *out = nullptr;
        return rc;
    };
    if (!path || !out) return refuse(SVX_E_INVALID, "svx_sam_open: null argument");
    s = new svx_sam();
    s->c.n_threads = thread_count(n_threads);
    auto bail = [&](const std::string& m) { return refuse(SVX_E_INVALID, m); };
    switch (s->file.open(path)) {
        case MappedText::CANNOT_OPEN: return bail(std::string("cannot open ") + path);
        case MappedText::NOT_REGULAR: return bail(std::string(path) + " is not a regular file");
        case MappedText::CANNOT_MAP: return refuse(SVX_E_NOMEM, std::string("cannot map ") + path);
        case MappedText::GZIP:
            return bail(std::string(path) + " is gzip- or bgzip-compressed: alignments are read from an uncompressed SAM or from a BAM");
        case MappedText::OK: break;
    }
    // header: every leading line that starts with '@'
    const char* map = s->file.map;
    const size_t size = s->file.size;
    size_t at = 0;
    while (at < size && map[at] == '@') {
        const char* nl = (const char*)memchr(map + at, '\n', size - at);
        const size_t next = nl ? (size_t)(nl - map) + 1 : size;
        size_t e = nl ? next - 1 : size;
        if (e > at && map[e - 1] == '\r') --e;
        if (e - at >= 3 && memcmp(map + at, "@SQ", 3) == 0 && (e - at == 3 || map[at + 3] == '\t')) {
            std::string name;
            int64_t length = -1;
            size_t q = at + 3;
            while (q < e) {
                ++q;  // the tab
                const char* tab = (const char*)memchr(map + q, '\t', e - q);
                const size_t fe = tab ? (size_t)(tab - map) : e;
                if (fe - q >= 3 && map[q + 2] == ':') {
                    if (map[q] == 'S' && map[q + 1] == 'N') name.assign(map + q + 3, fe - q - 3);
                    else if (map[q] == 'L' && map[q + 1] == 'N' && !parse_int(map + q + 3, fe - q - 3, 0, INT32_MAX, &length)) length = -1;
                }
                q = fe;
            }
            if (name.empty() || length < 0) return bail(std::string(path) + ": @SQ line " + std::to_string(s->header_lines + 1) + " lacks SN or a valid LN");
            if (s->tid_of.count(name)) return bail(std::string(path) + ": @SQ name '" + name + "' appears twice");
            s->tid_of[name] = (int32_t)s->ref_name.size();
            s->ref_name.push_back(name);
            s->ref_length.push_back((int32_t)length);
        }
        s->text.append(map + at, e - at);
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

extern "C" void svx_sam_close(svx_sam* s) { delete s; }

extern "C" const char* svx_sam_last_error(const svx_sam* s) { return s ? s->c.err.c_str() : "null handle"; }

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
    s->c.pin_device = device < 0 ? -1 : device;
    return SVX_OK;
}

extern "C" int svx_sam_set_device_parse(svx_sam* s, int on) {
    if (!s) return SVX_E_INVALID;
    s->c.device_parse = on ? 1 : 0;
    return SVX_OK;
}

extern "C" int svx_sam_parsed_on_device(const svx_sam* s) { return s ? s->c.parsed_on_device : 0; }

extern "C" int svx_sam_load(svx_sam* s, const int32_t* tids, int32_t n_tids) {
    if (!s || (n_tids > 0 && !tids) || n_tids < 0) return SVX_E_INVALID;
    Columns& c = s->c;
    c.begin_load();
    const size_t n_ref = s->ref_name.size();
    std::vector<uint8_t> want;
    if (tids) {
        want.assign(n_ref, 0);
        for (int32_t k = 0; k < n_tids; ++k) {
            if (tids[k] < 0 || (size_t)tids[k] >= n_ref) return c.fail(SVX_E_INVALID, "svx_sam_load: contig id out of range");
            want[(size_t)tids[k]] = 1;
        }
    }
    // 1. lines and fields, then the kept records in the presented order
    const char* map = s->file.map;
    std::vector<Rec>& recs = s->recs;
    auto parse = [s](uint64_t a, uint64_t e, Rec* r, std::string* what) { return parse_line(s, a, e, r, what); };
    if (!scan_lines(s->file, s->body, s->header_lines, c.n_threads, parse, &recs, &c.err)) return SVX_E_INVALID;
    if (tids)
        recs.erase(std::remove_if(recs.begin(), recs.end(), [&](const Rec& r) { return r.tid < 0 || !want[(size_t)r.tid]; }), recs.end());
    std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) {
        return record_before(a.tid, a.pos, a.flag, a.file_idx, b.tid, b.pos, b.flag, b.file_idx);
    });
    const uint64_t n = c.n = recs.size();
    if (n >= 0xFFFFFFFFull) return c.fail(SVX_E_TOO_LARGE, "more than 2^32 - 2 records");
    // 2. fixed columns, names, aux
    c.resize(n);
    std::vector<uint64_t> rec_off(n + 1, 0);
    std::vector<uint32_t> line_of(n);
    for (uint64_t i = 0; i < n; ++i) {
        const Rec& r = recs[i];
        c.tid[i] = r.tid; c.pos[i] = r.pos; c.l_seq[i] = (int32_t)r.seq_len; c.flag[i] = r.flag; c.mapq[i] = r.mapq;
        c.voffset[i] = r.line_off;
        line_of[i] = r.line;
        c.names.append(map + r.name_off, r.name_len);
        c.name_off[i + 1] = c.names.size();
        int64_t so;
        uint32_t sl;
        if (!encode_aux(map + r.aux_off, r.aux_end - r.aux_off, &c.aux, &so, &sl))
            return c.fail(SVX_E_INVALID, "line " + std::to_string(r.line) + ": an optional field is not TAG:TYPE:VALUE of a type the SAM format defines");
        c.sa_off[i] = so;
        c.sa_len[i] = sl;
        c.aux_off[i + 1] = c.aux.size();
        rec_off[i + 1] = rec_off[i] + r.cig_len;
    }
    // 3. the CIGAR strings back to back, then their words
    if (!c.alloc_text(rec_off[n])) return c.fail(SVX_E_NOMEM, "no memory for the CIGAR text");
    parallel_for(c.n_threads, n, [&](uint64_t i) { memcpy(c.h_text + rec_off[i], map + recs[i].cig_off, recs[i].cig_len); });
    return c.finish_cigars(rec_off, line_of, "the length of SEQ");
}

extern "C" int svx_sam_get_columns(const svx_sam* s, svx_bam_columns* out) { return s ? s->c.get_columns(out) : SVX_E_INVALID; }

extern "C" int svx_sam_seq_slices(svx_sam* s, const uint32_t* rec, const uint32_t* begin, const uint32_t* end, uint32_t n,
                                  const uint64_t* out_off, uint8_t* out) {
    if (!s) return SVX_E_INVALID;
    if (n == 0) return SVX_OK;
    if (!rec || !begin || !end || !out_off || !out) return s->c.fail(SVX_E_INVALID, "svx_sam_seq_slices: null argument");
    const uint8_t* alphabet = bam_alphabet();
    std::atomic<bool> failed(false);
    const uint64_t n_jobs = (n + 255) / 256;
    parallel_for(s->c.n_threads, n_jobs, [&](uint64_t j) {
        for (uint64_t i = j * 256; i < std::min<uint64_t>((j + 1) * 256, n); ++i) {
            if (rec[i] >= s->c.n) { failed.store(true); return; }
            const Rec& r = s->recs[rec[i]];
            const uint64_t a = std::min<uint64_t>(begin[i], r.seq_len), b = std::max(a, std::min<uint64_t>(end[i], r.seq_len));
            if (out_off[i + 1] < out_off[i] || out_off[i + 1] - out_off[i] < b - a) { failed.store(true); return; }
            const uint8_t* src = (const uint8_t*)s->file.map + r.seq_off + a;
            uint8_t* dst = out + out_off[i];
            for (uint64_t k = 0; k < b - a; ++k) dst[k] = alphabet[src[k]];
        }
    });
    if (failed.load()) return s->c.fail(SVX_E_INVALID, "svx_sam_seq_slices: bad slice bounds");
    return SVX_OK;
}

extern "C" int svx_sam_device_pool(svx_sam* s, const uint32_t** d_cigar, uint64_t* n_ops, void** ready) {
    return s ? s->c.device_pool(d_cigar, n_ops, ready) : SVX_E_INVALID;
}

extern "C" int svx_sam_device_pool_wait(svx_sam* s, double* waited_us) { return s ? s->c.device_pool_wait(waited_us) : SVX_E_INVALID; }
