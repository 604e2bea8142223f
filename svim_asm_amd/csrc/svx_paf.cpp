// svx_paf.cpp — native PAF ingest (include/svx_paf.h): minimap2's `-c` output read into the columns of svx_bam.h, the
// bases served from the query assembly.  A front end of svx_textaln.h, as svx_sam.cpp is:
//   * the file is memory-mapped (MappedText); scan_lines cuts it at line ends on the handle's threads and parse_row takes
//     the twelve columns and the tp / cg / NM tags of every row
//   * flags (primary / supplementary by file order) and SA strings come from ALL rows of a query name, then the kept rows
//     are ordered by svx_sam.h's comparison and every column is laid out in that order
//   * per kept row the text `<clip5>S` + cg + `<clip3>S` is gathered back to back and handed to Columns::finish_cigars:
//     device kernels or threads, pool in HBM, messages — nothing of it is restated here
//   * svx_paf_seq_slices turns (record, begin, end) into oriented windows of the query FASTA (svx_fasta_fetch_oriented)
// The handle holds its Columns by value: get_columns / device_pool and the error text are theirs.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "svx_paf.h"
#include "svx_textaln.h"

namespace {

using namespace svx_textaln;

struct Row : Line {
    uint64_t name_off, cg_off;
    uint32_t name_len, cg_len;
    int64_t nm;                       // -1: no NM:i tag
    int32_t qlen, qstart, qend, tid, tstart, tend;
    int32_t q_ref;                    // the query's place in the assembly's .fai (svx_paf_set_query)
    uint16_t flag;
    uint8_t mapq, rev, secondary, has_cg;
};

}  // namespace

struct svx_paf {
    MappedText file;
    std::string text;  // the @SQ lines of the dictionary
    std::vector<std::string> ref_name;
    std::vector<int32_t> ref_length;
    std::unordered_map<std::string, int32_t> tid_of;
    Columns c;              // the columns, the CIGAR pool and its copy in HBM, the error text
    std::vector<Row> rows;  // the loaded rows in the presented order
    // the assembly
    const svx_fasta* query = nullptr;
    std::unordered_map<std::string, std::pair<int32_t, int64_t>> query_of;  // name -> (place in the .fai, length)
    bool query_bound = false;  // the loaded rows carry q_ref
};

namespace {

int fail(svx_paf* p, int rc, const std::string& what) { return p->c.fail(rc, what); }

// clip5 / clip3 of the row's record (BAM orientation)
inline uint32_t clip5(const Row& r) { return (uint32_t)(r.rev ? r.qlen - r.qend : r.qstart); }
inline uint32_t clip3(const Row& r) { return (uint32_t)(r.rev ? r.qstart : r.qlen - r.qend); }

inline bool is_digit_byte(char c) { return (uint32_t)(uint8_t)c - '0' < 10u; }

std::string clip_text(uint32_t n) { return n ? std::to_string(n) + "S" : std::string(); }

std::string short_cigar(const Row& r) {
    const uint32_t q = (uint32_t)(r.qend - r.qstart), t = (uint32_t)(r.tend - r.tstart), m = std::min(q, t);
    std::string s = clip_text(clip5(r));
    if (m) s += std::to_string(m) + "M";
    if (q > m) s += std::to_string(q - m) + "I";
    if (t > m) s += std::to_string(t - m) + "D";
    return s + clip_text(clip3(r));
}

// One row [a, e) (no line end, no '\r'): false with *what set when it is malformed.
bool parse_row(const svx_paf* p, uint64_t a, uint64_t e, Row* r, std::string* what) {
    const char* m = p->file.map;
    uint64_t f[13];  // starts of columns 0..11, f[12]: one behind the tab that ends column 11 (or e + 1)
    f[0] = a;
    uint64_t at = a;
    for (int k = 1; k <= 12; ++k) {
        const char* tab = at < e ? (const char*)memchr(m + at, '\t', e - at) : nullptr;
        if (!tab) {
            if (k == 12) { f[12] = e + 1; break; }
            *what = "fewer than 12 columns";
            return false;
        }
        at = (uint64_t)(tab - m) + 1;
        f[k] = at;
    }
    auto len = [&](int k) { return f[k + 1] - 1 - f[k]; };
    auto num = [&](int k, uint64_t max, uint64_t* v) { return parse_uint(m + f[k], len(k), max, v); };
    uint64_t qlen, qs, qe, tlen, ts, te, mq;
    r->name_off = f[0];
    r->name_len = (uint32_t)std::min<uint64_t>(len(0), 0xFFFFFFFFu);
    if (!num(1, 0x7FFFFFFFu, &qlen)) { *what = "the query length (column 2) is not a number in 0..2^31-1"; return false; }
    if (!num(2, qlen, &qs) || !num(3, qlen, &qe) || qs > qe) {
        *what = "the query span (columns 3 and 4) is not two numbers with start <= end <= query length";
        return false;
    }
    if (len(4) != 1 || (m[f[4]] != '+' && m[f[4]] != '-')) { *what = "the strand (column 5) is neither + nor -"; return false; }
    r->rev = m[f[4]] == '-';
    const std::string tname(m + f[5], len(5));
    auto it = p->tid_of.find(tname);
    if (it == p->tid_of.end()) { *what = "the target '" + tname.substr(0, 80) + "' is not in the reference's index"; return false; }
    r->tid = it->second;
    if (!num(6, 0x7FFFFFFFu, &tlen)) { *what = "the target length (column 7) is not a number in 0..2^31-1"; return false; }
    if (tlen != (uint64_t)p->ref_length[(size_t)r->tid]) {
        *what = "the target '" + tname.substr(0, 80) + "' has length " + std::to_string(tlen) + " here and " +
                std::to_string(p->ref_length[(size_t)r->tid]) + " in the reference's index";
        return false;
    }
    if (!num(7, tlen, &ts) || !num(8, tlen, &te) || ts > te) {
        *what = "the target span (columns 8 and 9) is not two numbers with start <= end <= target length";
        return false;
    }
    uint64_t ignored;
    if (!num(9, ~0ull >> 1, &ignored) || !num(10, ~0ull >> 1, &ignored)) { *what = "columns 10 and 11 are not numbers"; return false; }
    if (!num(11, 255, &mq)) { *what = "MAPQ (column 12) is not a number in 0..255"; return false; }
    r->qlen = (int32_t)qlen; r->qstart = (int32_t)qs; r->qend = (int32_t)qe;
    r->tstart = (int32_t)ts; r->tend = (int32_t)te;
    r->mapq = (uint8_t)mq;
    r->nm = -1;
    r->secondary = 0;
    r->has_cg = 0;
    r->cg_off = 0;
    r->cg_len = 0;
    r->q_ref = -1;
    r->flag = 0;
    // the tags this reader uses
    at = std::min(f[12], e);
    while (at < e) {
        const char* tab = (const char*)memchr(m + at, '\t', e - at);
        const uint64_t fe = tab ? (uint64_t)(tab - m) : e;
        const char* t = m + at;
        const uint64_t l = fe - at;
        if (l >= 5 && t[2] == ':' && t[4] == ':') {
            if (t[0] == 't' && t[1] == 'p' && t[3] == 'A') {
                r->secondary = l == 6 && t[5] == 'S';
            } else if (t[0] == 'c' && t[1] == 'g' && t[3] == 'Z') {
                if (l - 5 > 0xFFFFFFFFull) { *what = "cg:Z: longer than 4 GiB"; return false; }
                // (what the clips written around the value would hide from the parser: `80` + `10S` reads as one number)
                if (l == 5) { *what = "the CIGAR has an operator without a length"; return false; }
                if (is_digit_byte(t[l - 1])) { *what = "the CIGAR has digits without an operator at its end"; return false; }
                r->has_cg = 1;
                r->cg_off = at + 5;
                r->cg_len = (uint32_t)(l - 5);
            } else if (t[0] == 'N' && t[1] == 'M' && t[3] == 'i') {
                uint64_t v;
                if (!parse_uint(t + 5, l - 5, 0xFFFFFFFFull, &v)) { *what = "NM:i: is not a number in 0..2^32-1"; return false; }
                r->nm = (int64_t)v;
            }
        }
        at = fe + 1;
    }
    if (!r->secondary && !r->has_cg) {
        *what = "the row has no cg:Z: tag: a PAF carries its CIGAR only when minimap2 runs with -c";
        return false;
    }
    return true;
}

void put_nm(std::vector<uint8_t>* aux, int64_t nm) {
    aux->push_back('N');
    aux->push_back('M');
    const uint32_t v = (uint32_t)nm;
    if (v <= 255) { aux->push_back('C'); aux->push_back((uint8_t)v); }
    else if (v <= 65535) { aux->push_back('S'); aux->push_back((uint8_t)(v & 255)); aux->push_back((uint8_t)(v >> 8)); }
    else { aux->push_back('I'); for (int k = 0; k < 4; ++k) aux->push_back((uint8_t)(v >> (8 * k))); }
}

}  // namespace

extern "C" int svx_paf_open(const char* path, int32_t n_ref, const char* const* names, const int32_t* lengths, int n_threads,
                            svx_paf** out, char* err, size_t err_cap) {
    svx_paf* p = nullptr;
    auto refuse = [&](int rc, const std::string& m) {
        delete p;
        if (err && err_cap) snprintf(err, err_cap, "%s", m.c_str());
        if (out) *out = nullptr;
        return rc;
    };
    if (!path || !out || n_ref < 0 || (n_ref && (!names || !lengths))) return refuse(SVX_E_INVALID, "svx_paf_open: bad argument");
    p = new svx_paf();
    p->c.n_threads = thread_count(n_threads);
    auto bail = [&](const std::string& m) { return refuse(SVX_E_INVALID, m); };
    switch (p->file.open(path)) {
        case MappedText::CANNOT_OPEN: return bail(std::string("cannot open ") + path);
        case MappedText::NOT_REGULAR: return bail(std::string(path) + " is not a regular file");
        case MappedText::CANNOT_MAP: return refuse(SVX_E_NOMEM, std::string("cannot map ") + path);
        case MappedText::GZIP: return bail(std::string(path) + " is gzip-compressed: a PAF is read as uncompressed text");
        case MappedText::OK: break;
    }
    const char* map = p->file.map;
    const size_t size = p->file.size;
    size_t at = 0;
    while (at < size && (map[at] == '\n' || map[at] == '\r')) ++at;
    if (at >= size) return bail(std::string(path) + " is empty: no PAF rows");
    if (map[at] == '@')
        return bail(std::string(path) + " starts with a SAM header line: it is a SAM file, not a PAF (give it without a query FASTA)");
    for (int32_t k = 0; k < n_ref; ++k) {
        if (!names[k] || lengths[k] < 0) return bail("svx_paf_open: bad reference dictionary");
        const std::string name(names[k]);
        if (p->tid_of.count(name)) return bail("the reference's index names '" + name + "' twice");
        p->tid_of[name] = k;
        p->ref_name.push_back(name);
        p->ref_length.push_back(lengths[k]);
        p->text += "@SQ\tSN:" + name + "\tLN:" + std::to_string(lengths[k]) + "\n";
    }
    *out = p;
    return SVX_OK;
}

extern "C" void svx_paf_close(svx_paf* p) { delete p; }

extern "C" const char* svx_paf_last_error(const svx_paf* p) { return p ? p->c.err.c_str() : "null handle"; }

extern "C" int svx_paf_header(const svx_paf* p, const char** text, uint64_t* l_text, int32_t* n_ref) {
    if (!p) return SVX_E_INVALID;
    if (text) *text = p->text.data();
    if (l_text) *l_text = p->text.size();
    if (n_ref) *n_ref = (int32_t)p->ref_name.size();
    return SVX_OK;
}

extern "C" int svx_paf_reference(const svx_paf* p, int32_t tid, const char** name, int32_t* length) {
    if (!p || tid < 0 || (size_t)tid >= p->ref_name.size()) return SVX_E_INVALID;
    if (name) *name = p->ref_name[(size_t)tid].c_str();
    if (length) *length = p->ref_length[(size_t)tid];
    return SVX_OK;
}

extern "C" int svx_paf_set_pinned_device(svx_paf* p, int device) {
    if (!p) return SVX_E_INVALID;
    p->c.pin_device = device < 0 ? -1 : device;
    return SVX_OK;
}

extern "C" int svx_paf_set_device_parse(svx_paf* p, int on) {
    if (!p) return SVX_E_INVALID;
    p->c.device_parse = on ? 1 : 0;
    return SVX_OK;
}

extern "C" int svx_paf_parsed_on_device(const svx_paf* p) { return p ? p->c.parsed_on_device : 0; }

extern "C" int svx_paf_load(svx_paf* p, const int32_t* tids, int32_t n_tids) {
    if (!p || (n_tids > 0 && !tids) || n_tids < 0) return SVX_E_INVALID;
    Columns* c = &p->c;
    c->begin_load();
    p->rows.clear();
    p->query_bound = false;
    const size_t n_ref = p->ref_name.size();
    std::vector<uint8_t> want;
    if (tids) {
        want.assign(n_ref, 0);
        for (int32_t k = 0; k < n_tids; ++k) {
            if (tids[k] < 0 || (size_t)tids[k] >= n_ref) return fail(p, SVX_E_INVALID, "svx_paf_load: contig id out of range");
            want[(size_t)tids[k]] = 1;
        }
    }
    // 1. lines and columns
    const char* map = p->file.map;
    std::vector<Row> all;
    auto parse = [p](uint64_t a, uint64_t e, Row* r, std::string* what) { return parse_row(p, a, e, r, what); };
    if (!scan_lines(p->file, 0, 0, c->n_threads, parse, &all, &c->err)) return SVX_E_INVALID;
    if (all.size() >= 0xFFFFFFFFull) return fail(p, SVX_E_TOO_LARGE, "more than 2^32 - 2 rows");
    // 2. the rows of every query name in file order: one length, primary / supplementary, the partners of the SA strings
    std::unordered_map<std::string_view, std::vector<uint32_t>> by_name;  // (the rows of a name that are not secondary)
    std::unordered_map<std::string_view, int32_t> qlen_of;
    for (Row& r : all) {
        const std::string_view name(map + r.name_off, r.name_len);
        auto q = qlen_of.emplace(name, r.qlen);
        if (!q.second && q.first->second != r.qlen)
            return fail(p, SVX_E_INVALID, "line " + std::to_string(r.line) + ": the query '" + std::string(name.substr(0, 80)) + "' has length " +
                                              std::to_string(r.qlen) + " here and " + std::to_string(q.first->second) + " in an earlier row");
        r.flag = r.rev ? 0x10 : 0;
        if (r.secondary) {
            r.flag |= 0x100;
            continue;
        }
        std::vector<uint32_t>& group = by_name[name];
        if (!group.empty()) r.flag |= 0x800;
        group.push_back((uint32_t)r.file_idx);
    }
    // 3. the kept rows in the presented order
    std::vector<Row>& rows = p->rows;
    for (const Row& r : all)
        if (!tids || want[(size_t)r.tid]) rows.push_back(r);
    std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) {
        return record_before(a.tid, a.tstart, a.flag, a.file_idx, b.tid, b.tstart, b.flag, b.file_idx);
    });
    const uint64_t n = rows.size();
    // 4. fixed columns, names, aux (NM, SA)
    c->resize(n);
    std::vector<uint64_t> rec_off(n + 1, 0);
    std::vector<uint32_t> line_of(n);
    std::vector<std::string> head(n), tail(n);  // `<clip5>S` and `<clip3>S`
    for (uint64_t i = 0; i < n; ++i) {
        const Row& r = rows[i];
        c->tid[i] = r.tid; c->pos[i] = r.tstart; c->l_seq[i] = r.qlen; c->flag[i] = r.flag; c->mapq[i] = r.mapq;
        c->voffset[i] = r.line_off;
        line_of[i] = r.line;
        c->names.append(map + r.name_off, r.name_len);
        c->name_off[i + 1] = c->names.size();
        if (r.nm >= 0) put_nm(&c->aux, r.nm);
        c->sa_off[i] = -1;
        c->sa_len[i] = 0;
        if (!r.secondary) {
            const std::vector<uint32_t>& group = by_name[std::string_view(map + r.name_off, r.name_len)];
            if (group.size() > 1) {
                std::string sa;
                for (uint32_t k : group) {
                    if (k == r.file_idx) continue;
                    const Row& o = all[k];
                    sa += p->ref_name[(size_t)o.tid] + "," + std::to_string(o.tstart + 1) + "," + (o.rev ? "-" : "+") + "," + short_cigar(o) + "," +
                          std::to_string(o.mapq) + "," + std::to_string(o.nm < 0 ? 0 : o.nm) + ";";
                }
                c->aux.push_back('S'); c->aux.push_back('A'); c->aux.push_back('Z');
                c->sa_off[i] = (int64_t)c->aux.size();
                c->sa_len[i] = (uint32_t)sa.size();
                c->aux.insert(c->aux.end(), sa.begin(), sa.end());
                c->aux.push_back(0);
            }
        }
        c->aux_off[i + 1] = c->aux.size();
        if (r.has_cg) {
            head[i] = clip_text(clip5(r));
            tail[i] = clip_text(clip3(r));
            rec_off[i + 1] = rec_off[i] + head[i].size() + r.cg_len + tail[i].size();
        } else {
            rec_off[i + 1] = rec_off[i] + 1;  // `*`: a tp:A:S row without cg
        }
    }
    // 5. per record `<clip5>S` + cg + `<clip3>S` back to back, then the words
    if (!c->alloc_text(rec_off[n])) return fail(p, SVX_E_NOMEM, "no memory for the CIGAR text");
    parallel_for(p->c.n_threads, n, [&](uint64_t i) {
        const Row& r = rows[i];
        uint8_t* dst = c->h_text + rec_off[i];
        if (!r.has_cg) { *dst = '*'; return; }
        memcpy(dst, head[i].data(), head[i].size());
        memcpy(dst + head[i].size(), map + r.cg_off, r.cg_len);
        memcpy(dst + head[i].size() + r.cg_len, tail[i].data(), tail[i].size());
    });
    const int rc = c->finish_cigars(rec_off, line_of, "the row's query span (columns 4 - 3)");
    if (rc != SVX_OK) {
        p->rows.clear();
        return rc;
    }
    for (uint64_t i = 0; i < n; ++i)
        if (rows[i].has_cg && c->ref_len[i] != rows[i].tend - rows[i].tstart) {
            const uint32_t line = rows[i].line;
            c->begin_load();
            p->rows.clear();
            return fail(p, SVX_E_INVALID, "line " + std::to_string(line) + ": the CIGAR's reference length differs from the row's target span (columns 9 - 8)");
        }
    return SVX_OK;
}

extern "C" int svx_paf_get_columns(const svx_paf* p, svx_bam_columns* out) { return p ? p->c.get_columns(out) : SVX_E_INVALID; }

extern "C" int svx_paf_device_pool(svx_paf* p, const uint32_t** d_cigar, uint64_t* n_ops, void** ready) {
    return p ? p->c.device_pool(d_cigar, n_ops, ready) : SVX_E_INVALID;
}

extern "C" int svx_paf_device_pool_wait(svx_paf* p, double* waited_us) { return p ? p->c.device_pool_wait(waited_us) : SVX_E_INVALID; }

extern "C" int svx_paf_set_query(svx_paf* p, const svx_fasta* query, int32_t n_seq, const char* const* names, const int64_t* lengths) {
    if (!p || !query || n_seq < 0 || (n_seq && (!names || !lengths))) return SVX_E_INVALID;
    p->query = query;
    p->query_of.clear();
    p->query_bound = false;
    for (int32_t k = 0; k < n_seq; ++k) {
        if (!names[k]) return fail(p, SVX_E_INVALID, "svx_paf_set_query: null name");
        p->query_of.emplace(std::string(names[k]), std::make_pair(k, lengths[k]));  // (a name listed twice: the first, as the FASTA handle)
    }
    return SVX_OK;
}

extern "C" int svx_paf_seq_slices(svx_paf* p, const uint32_t* rec, const uint32_t* begin, const uint32_t* end, uint32_t n,
                                  const uint64_t* out_off, uint8_t* out) {
    if (!p) return SVX_E_INVALID;
    if (n == 0) return SVX_OK;
    if (!rec || !begin || !end || !out_off || !out) return fail(p, SVX_E_INVALID, "svx_paf_seq_slices: null argument");
    if (!p->query) return fail(p, SVX_E_INVALID, "svx_paf_seq_slices: no query assembly (svx_paf_set_query)");
    if (!p->query_bound) {
        for (Row& r : p->rows) {
            const std::string name(p->file.map + r.name_off, r.name_len);
            auto it = p->query_of.find(name);
            if (it == p->query_of.end())
                return fail(p, SVX_E_INVALID, "line " + std::to_string(r.line) + ": the query '" + name.substr(0, 80) + "' is not in the query FASTA's index");
            if (it->second.second != r.qlen)
                return fail(p, SVX_E_INVALID, "line " + std::to_string(r.line) + ": the query '" + name.substr(0, 80) + "' has length " + std::to_string(r.qlen) +
                                                  " here and " + std::to_string(it->second.second) + " in the query FASTA's index");
            r.q_ref = it->second.first;
        }
        p->query_bound = true;
    }
    std::vector<int32_t> ref(n);
    std::vector<int64_t> start(n), stop(n);
    std::vector<uint8_t> reverse(n);
    std::vector<uint64_t> packed(n + 1, 0);
    bool exact = true;
    for (uint32_t i = 0; i < n; ++i) {
        if (rec[i] >= p->rows.size()) return fail(p, SVX_E_INVALID, "svx_paf_seq_slices: bad slice bounds");
        const Row& r = p->rows[rec[i]];
        const int64_t a = std::min<int64_t>(begin[i], r.qlen), b = std::max<int64_t>(a, std::min<int64_t>(end[i], r.qlen));
        if (out_off[i + 1] < out_off[i] || out_off[i + 1] - out_off[i] < (uint64_t)(b - a))
            return fail(p, SVX_E_INVALID, "svx_paf_seq_slices: bad slice bounds");
        exact = exact && out_off[i + 1] - out_off[i] == (uint64_t)(b - a);
        ref[i] = r.q_ref;
        reverse[i] = r.rev;
        start[i] = r.rev ? r.qlen - b : a;
        stop[i] = r.rev ? r.qlen - a : b;
        packed[i + 1] = packed[i] + (uint64_t)(b - a);
    }
    int rc;
    if (exact) {
        rc = svx_fasta_fetch_oriented(p->query, ref.data(), start.data(), stop.data(), reverse.data(), n, 1, out_off, out, p->c.n_threads);
    } else {  // slots wider than their slices: fetched back to back, then put in place
        std::vector<uint8_t> tmp(packed[n] + 1);
        rc = svx_fasta_fetch_oriented(p->query, ref.data(), start.data(), stop.data(), reverse.data(), n, 1, packed.data(), tmp.data(), p->c.n_threads);
        for (uint32_t i = 0; rc == SVX_OK && i < n; ++i) memcpy(out + out_off[i], tmp.data() + packed[i], packed[i + 1] - packed[i]);
    }
    if (rc != SVX_OK) {
        const char* why = svx_fasta_last_error(p->query);
        return fail(p, rc, std::string("the query FASTA could not serve the bases") + (why && *why ? std::string(": ") + why : std::string(" (shorter than its index says?)")));
    }
    return SVX_OK;
}
