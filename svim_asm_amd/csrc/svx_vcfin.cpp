// svx_vcfin.cpp — the VCF reader (include/svx_vcfin.h; the classification of records is defined there): the third
// front end of svx_textaln.h's line scanner, beside svx_sam.cpp and svx_paf.cpp.
//   * plain text is memory-mapped (MappedText); a .gz is walked member by member (svx_bgzf::parse_member), the members
//     are inflated and CRC-checked on the handle's threads (svx_bgzf::Inflater) into one anonymous mapping, which the
//     MappedText then owns — a line may straddle members, the scanner sees joined text
//   * the header lines are walked serially (they name the sample columns); scan_lines cuts the rest at line ends on the
//     handle's threads and classify() takes every data line
//   * the DEL and INS rows are laid out as columns in file order; the inserted bytes are gathered upper-cased into a pool
// Host code only.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "svx.h"
#include "svx_bgzf.h"
#include "svx_textaln.h"
#include "svx_vcfin.h"

namespace {

using namespace svx_textaln;

struct Row : Line {
    uint64_t line_end, id_off, seq_off;  // seq_off: the inserted bytes in the text (INS; the alleles reader: the alternative bytes)
    int64_t start, end;                  // (the alleles reader: end = POS - 1)
    int32_t contig;
    uint32_t id_len, seq_len;
    uint64_t ref_off;                    // the alleles reader: the REF column in the text, as written
    uint32_t ref_text_len, ref_len;
    uint8_t cls, gt, phased;
};

struct Dict {
    std::unordered_map<std::string, int32_t> tid_of;
    std::vector<int64_t> length;
};

inline bool is_letter(char c) { return (uint32_t)((uint8_t)c | 32) - 'a' < 26u; }
inline char upper(char c) { return (uint32_t)(uint8_t)c - 'a' < 26u ? (char)(c - 32) : c; }

bool all_letters(const char* s, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (!is_letter(s[i])) return false;
    return true;
}

bool equals(const char* s, uint64_t n, const char* lit) { return n == strlen(lit) && memcmp(s, lit, n) == 0; }

// the value of `key=` among the ';'-separated fields of INFO: false when the key is not there
bool info_value(const char* s, uint64_t n, const char* key, const char** v, uint64_t* vn) {
    const size_t kn = strlen(key);
    uint64_t at = 0;
    while (at < n) {
        const char* semi = (const char*)memchr(s + at, ';', n - at);
        const uint64_t fe = semi ? (uint64_t)(semi - s) : n;
        if (fe - at > kn && memcmp(s + at, key, kn) == 0 && s[at + kn] == '=') {
            *v = s + at + kn + 1;
            *vn = fe - at - kn - 1;
            return true;
        }
        at = fe + 1;
    }
    return false;
}

// haplotype bits of the GT text [s, s + n): allele h == "1" sets bit h (the first two alleles), a single "1" sets both
uint8_t genotype_bits(const char* s, uint64_t n) {
    uint8_t bits = 0;
    int h = 0;
    uint64_t at = 0;
    while (at <= n && h < 2) {
        uint64_t e = at;
        while (e < n && s[e] != '/' && s[e] != '|') ++e;
        if (e - at == 1 && s[at] == '1') bits |= (uint8_t)(1 << h);
        ++h;
        if (e >= n) break;
        at = e + 1;
    }
    if (h == 1 && bits == 1) bits = 3;
    return bits;
}

// is the GT text [s, s + n) with the bits above phased?  its first separator is '|', it has one allele, or both alleles are 1
uint8_t genotype_phased(const char* s, uint64_t n, uint8_t bits) {
    for (uint64_t i = 0; i < n; ++i)
        if (s[i] == '/' || s[i] == '|') return s[i] == '|' || bits == 3;
    return 1;
}

struct Classifier {
    const char* m;
    const Dict* dict;
    int sample_col;  // column of the chosen sample (>= 9), -1: the file has no sample columns
    bool passonly;
    bool alleles;    // svx_vcfin_open_alleles: the classes and the rows of the second reader

    // One data line [a, e) (no line end, no '\r'): false with *what set when it is refused.
    bool operator()(uint64_t a, uint64_t e, Row* r, std::string* what) const {
        uint64_t f[9];  // starts of columns 0..7, f[8]: one behind the tab that ends column 7 (or e + 1)
        f[0] = a;
        uint64_t at = a;
        for (int k = 1; k <= 8; ++k) {
            const char* tab = at <= e ? (const char*)memchr(m + at, '\t', e - at) : nullptr;
            if (!tab) {
                if (k == 8) { f[8] = e + 1; break; }
                *what = "fewer than 8 columns";
                return false;
            }
            at = (uint64_t)(tab - m) + 1;
            f[k] = at;
        }
        auto len = [&](int k) { return f[k + 1] - 1 - f[k]; };
        r->line_end = e;
        r->id_off = f[2];
        r->id_len = (uint32_t)std::min<uint64_t>(len(2), 0xFFFFFFFFu);
        r->seq_off = 0; r->seq_len = 0; r->start = 0; r->end = 0; r->gt = 0;
        r->ref_off = 0; r->ref_text_len = 0; r->ref_len = 0; r->phased = 1;
        const std::string chrom(m + f[0], len(0));
        auto it = dict->tid_of.find(chrom);
        if (it == dict->tid_of.end()) { *what = "the contig '" + chrom.substr(0, 80) + "' is not in the genome's index"; return false; }
        r->contig = it->second;
        const int64_t clen = dict->length[(size_t)r->contig];
        uint64_t pos;
        if (!parse_uint(m + f[1], len(1), 1ull << 40, &pos) || pos < 1) { *what = "POS (column 2) is not a number >= 1"; return false; }
        if ((int64_t)pos > clen) {
            *what = "POS " + std::to_string(pos) + " is beyond the length of '" + chrom.substr(0, 80) + "' (" + std::to_string(clen) + ")";
            return false;
        }
        const char* ref = m + f[3];
        const char* alt = m + f[4];
        uint64_t nref = len(3), nalt = len(4);
        if (passonly && !equals(m + f[6], len(6), "PASS") && !equals(m + f[6], len(6), ".")) {
            r->cls = alleles ? SVX_VCFIN_A_FILTERED : SVX_VCFIN_FILTERED;
            return true;
        }
        if (memchr(alt, ',', nalt)) { r->cls = alleles ? SVX_VCFIN_A_MULTIALLELIC : SVX_VCFIN_MULTIALLELIC; return true; }
        if (equals(ref, nref, ".")) nref = 0;
        if (alleles) {
            if (equals(alt, nalt, ".")) nalt = 0;
            if (!all_letters(ref, nref) || !all_letters(alt, nalt)) { r->cls = SVX_VCFIN_A_SYMBOLIC_OR_OTHER; return true; }
            uint64_t p = 0, s = 0;
            const uint64_t lim = std::min(nref, nalt);
            while (p < lim && upper(ref[p]) == upper(alt[p])) ++p;
            while (s < lim - p && upper(ref[nref - 1 - s]) == upper(alt[nalt - 1 - s])) ++s;
            if (p == nref && p == nalt) { r->cls = SVX_VCFIN_A_NO_CHANGE; return true; }
            if (nref > 0xFFFFFFFFull || nalt > 0xFFFFFFFFull) { *what = "an allele longer than 4 GiB"; return false; }
            r->cls = SVX_VCFIN_A_ROW;
            r->end = (int64_t)pos - 1;
            r->start = (int64_t)(pos - 1 + p);
            r->ref_off = f[3];
            r->ref_text_len = (uint32_t)nref;
            r->ref_len = (uint32_t)(nref - p - s);
            r->seq_off = f[4] + p;
            r->seq_len = (uint32_t)(nalt - p - s);
            if ((int64_t)(pos - 1 + nref) > clen) {
                *what = "REF ends at " + std::to_string(pos - 1 + nref) + ", beyond the length of '" + chrom.substr(0, 80) + "' (" +
                        std::to_string(clen) + ")";
                return false;
            }
            return carried(f[8], e, r, what, SVX_VCFIN_A_NOT_CARRIED);
        }
        const bool symbolic_del = equals(alt, nalt, "<DEL>");
        if (equals(alt, nalt, ".")) nalt = 0;
        if (symbolic_del) {
            const char *v;
            uint64_t vn, end, svlen = 0;
            const char* info = m + f[7];
            const uint64_t ninfo = len(7);
            if (!info_value(info, ninfo, "END", &v, &vn) || !parse_uint(v, vn, 1ull << 40, &end)) {
                *what = "a <DEL> record without a numeric INFO END";
                return false;
            }
            int64_t start = (int64_t)pos;
            if (info_value(info, ninfo, "SVLEN", &v, &vn)) {
                if (vn && (v[0] == '-' || v[0] == '+')) { ++v; --vn; }
                if (!parse_uint(v, vn, 1ull << 40, &svlen)) { *what = "a <DEL> record whose INFO SVLEN is not a number"; return false; }
                start = (int64_t)end - (int64_t)svlen;
            }
            if (start < 0 || start >= (int64_t)end) { *what = "a <DEL> record with an empty interval"; return false; }
            if ((int64_t)end > clen) {
                *what = "END " + std::to_string(end) + " is beyond the length of '" + chrom.substr(0, 80) + "' (" + std::to_string(clen) + ")";
                return false;
            }
            r->cls = SVX_VCFIN_DEL;
            r->start = start;
            r->end = (int64_t)end;
        } else if (equals(alt, nalt, "<INS>")) {
            r->cls = SVX_VCFIN_UNRESOLVED;
            return true;
        } else if (!all_letters(ref, nref) || !all_letters(alt, nalt)) {
            r->cls = SVX_VCFIN_OTHER;
            return true;
        } else {
            uint64_t p = 0;
            const uint64_t lim = std::min(nref, nalt);
            while (p < lim && upper(ref[p]) == upper(alt[p])) ++p;
            if (p == nalt && nalt < nref) {
                r->cls = SVX_VCFIN_DEL;
                r->start = (int64_t)(pos - 1 + p);
                r->end = (int64_t)(pos - 1 + nref);
                if (r->end > clen) {
                    *what = "the deletion ends at " + std::to_string(r->end) + ", beyond the length of '" + chrom.substr(0, 80) + "' (" +
                            std::to_string(clen) + ")";
                    return false;
                }
            } else if (p == nref && nref < nalt) {
                if (nalt - p > 0xFFFFFFFFull) { *what = "an insertion longer than 4 GiB"; return false; }
                r->cls = SVX_VCFIN_INS;
                r->start = (int64_t)(pos - 1 + p);
                r->end = r->start + (int64_t)(nalt - p);
                r->seq_off = f[4] + p;
                r->seq_len = (uint32_t)(nalt - p);
                if (r->start > clen) {
                    *what = "the insertion lies at " + std::to_string(r->start) + ", beyond the length of '" + chrom.substr(0, 80) + "' (" +
                            std::to_string(clen) + ")";
                    return false;
                }
            } else {
                r->cls = SVX_VCFIN_COMPLEX;
                return true;
            }
        }
        return carried(f[8], e, r, what, SVX_VCFIN_NOT_CARRIED);
    }

    // A row's genotype from the sample column of the line that ends at e, `at` the start of FORMAT (column 8): gt, phased,
    // and the class `not_carried` where the GT carries no allele 1.
    bool carried(uint64_t at, uint64_t e, Row* r, std::string* what, uint8_t not_carried) const {
        if (sample_col < 0) return true;
        uint64_t fmt = 0, fmt_len = 0;
        for (int k = 8;; ++k) {
            if (at > e) { *what = "the line has no column for the sample"; return false; }
            const char* tab = (const char*)memchr(m + at, '\t', e - at);
            const uint64_t fe = tab ? (uint64_t)(tab - m) : e;
            if (k == 8) { fmt = at; fmt_len = fe - at; }
            if (k == sample_col) {
                // (a FORMAT that does not start with GT: no genotype, the record counts as carried)
                if (!(fmt_len >= 2 && m[fmt] == 'G' && m[fmt + 1] == 'T' && (fmt_len == 2 || m[fmt + 2] == ':'))) return true;
                const char* colon = (const char*)memchr(m + at, ':', fe - at);
                const uint64_t gn = colon ? (uint64_t)(colon - (m + at)) : fe - at;
                r->gt = genotype_bits(m + at, gn);
                r->phased = genotype_phased(m + at, gn, r->gt);
                if (!r->gt) r->cls = not_carried;
                return true;
            }
            at = fe + 1;
        }
    }
};

}  // namespace

struct svx_vcfin {
    MappedText file;  // the text: the mapped file, or the inflated members in an anonymous mapping
    uint64_t header_bytes = 0, n_lines = 0;
    uint64_t counts[SVX_VCFIN_N_CLASSES] = {};
    std::vector<uint8_t> type, gt, seqs;
    std::vector<int32_t> contig;
    std::vector<int64_t> start, end;
    std::vector<uint64_t> seq_off, line_off, id_off;
    std::vector<uint32_t> seq_len, line_len, line_no, id_len;
    // svx_vcfin_open_alleles: rows of svx_vcfin_alleles (start, contig, gt, seqs / seq_off / seq_len and the line columns above are shared)
    bool alleles = false;
    uint64_t acounts[SVX_VCFIN_A_N_CLASSES] = {};
    std::vector<int64_t> pos;
    std::vector<uint64_t> ref_off;
    std::vector<uint32_t> ref_len, ref_text_len;
    std::vector<uint8_t> phased;
};

namespace {

// The members of a BGZF file inflated into one anonymous mapping that `file` owns from then on.
int inflate_bgzf(svx_vcfin* v, const char* path, int n_threads, std::string* err) {
    const uint8_t* map = (const uint8_t*)v->file.map;
    const uint64_t fsize = v->file.size;
    std::vector<uint64_t> coff, ooff;
    std::vector<svx_bgzf::Member> mem;
    uint64_t at = 0, out = 0;
    for (;;) {
        svx_bgzf::Member m;
        const int rc = svx_bgzf::parse_member(map, fsize, at, &m);
        if (rc == 1) break;
        if (rc < 0) {
            *err = std::string(path) + (mem.empty() ? " is gzip-compressed but not BGZF: compress it with bgzip"
                                                    : " has a damaged BGZF member at byte " + std::to_string(at) +
                                                          " (or is not BGZF throughout: compress it with bgzip)");
            return SVX_E_INVALID;
        }
        coff.push_back(at);
        ooff.push_back(out);
        mem.push_back(m);
        at += m.bsize;
        out += m.isize;
    }
    char* text = nullptr;
    if (out) {
        void* p = mmap(nullptr, out, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) { *err = "no memory for the inflated text of " + std::string(path); return SVX_E_NOMEM; }
        text = (char*)p;
    }
    constexpr uint64_t kChunk = 32;  // members a thread takes at a time, with one decoder
    std::atomic<int64_t> bad(-1);
    parallel_for(n_threads, (mem.size() + kChunk - 1) / kChunk, [&](uint64_t c) {
        svx_bgzf::Inflater inf(svx_bgzf::use_zlib());
        for (uint64_t k = c * kChunk; k < std::min<uint64_t>(mem.size(), (c + 1) * kChunk); ++k) {
            if (!mem[k].isize) {  // (the empty member at the end of every bgzip file)
                continue;
            }
            if (!inf.run(map + coff[k] + mem[k].payload_off, mem[k].payload_len, (uint8_t*)text + ooff[k], mem[k].isize, mem[k].crc)) {
                int64_t none = -1;
                bad.compare_exchange_strong(none, (int64_t)k);
            }
        }
    });
    if (bad.load() >= 0) {
        if (text) munmap(text, out);
        *err = std::string(path) + ": a BGZF member near byte " + std::to_string(coff[(size_t)bad.load()]) +
               " does not inflate or fails its CRC32";
        return SVX_E_INVALID;
    }
    v->file.close();
    v->file.map = text;
    v->file.size = out;
    return SVX_OK;
}

}  // namespace

// svx_vcfin_open, or with `sites` svx_vcfin_open_sites: the sample columns are not looked at
static int open_vcf(const char* path, int32_t n_ref, const char* const* names, const int64_t* lengths, const char* sample, bool sites,
                    bool alleles, int passonly, int n_threads, svx_vcfin** out, char* err, size_t err_cap) {
    svx_vcfin* v = nullptr;
    auto refuse = [&](int rc, const std::string& msg) {
        delete v;
        if (err && err_cap) snprintf(err, err_cap, "%s", msg.c_str());
        if (out) *out = nullptr;
        return rc;
    };
    if (!path || !out || n_ref < 0 || (n_ref && (!names || !lengths))) return refuse(SVX_E_INVALID, "svx_vcfin_open: bad argument");
    v = new svx_vcfin();
    const int threads = thread_count(n_threads);
    auto bail = [&](const std::string& msg) { return refuse(SVX_E_INVALID, msg); };
    switch (v->file.open(path)) {
        case MappedText::CANNOT_OPEN: return bail(std::string("cannot open ") + path);
        case MappedText::NOT_REGULAR: return bail(std::string(path) + " is not a regular file");
        case MappedText::CANNOT_MAP: return refuse(SVX_E_NOMEM, std::string("cannot map ") + path);
        case MappedText::GZIP: {
            std::string msg;
            const int rc = inflate_bgzf(v, path, threads, &msg);
            if (rc != SVX_OK) return refuse(rc, msg);
            break;
        }
        case MappedText::OK: break;
    }
    Dict dict;
    for (int32_t t = 0; t < n_ref; ++t) {
        if (!names[t]) return bail("svx_vcfin_open: a null contig name");
        dict.tid_of.emplace(names[t], t);
        dict.length.push_back(lengths[t]);
    }
    // ---- the header: the lines in front of the first data line
    const char* map = v->file.map;
    const uint64_t size = v->file.size;
    uint64_t at = 0, n_before = 0, chrom_at = 0, chrom_end = 0, chrom_line = 0;
    bool last_is_chrom = false;
    while (at < size) {
        const char* nl = (const char*)memchr(map + at, '\n', size - at);
        uint64_t e = nl ? (uint64_t)(nl - map) : size;
        const uint64_t next = nl ? e + 1 : size;
        if (e > at && map[e - 1] == '\r') --e;
        if (e > at) {
            if (map[at] != '#') break;
            last_is_chrom = e - at >= 6 && memcmp(map + at, "#CHROM", 6) == 0;
            if (last_is_chrom) { chrom_at = at; chrom_end = e; chrom_line = n_before + 1; }
        }
        ++n_before;
        at = next;
    }
    if (!chrom_line) return bail(std::string(path) + ": line " + std::to_string(n_before + 1) + ": no #CHROM line in front of the records");
    if (!last_is_chrom)
        return bail(std::string(path) + ": line " + std::to_string(chrom_line) + ": the #CHROM line is not the last line of the header");
    v->header_bytes = at;
    // the sample columns the #CHROM line names
    int sample_col = -1;
    {
        std::vector<std::string> cols;
        uint64_t c = chrom_at;
        while (c <= chrom_end) {
            const char* tab = (const char*)memchr(map + c, '\t', chrom_end - c);
            const uint64_t fe = tab ? (uint64_t)(tab - map) : chrom_end;
            cols.emplace_back(map + c, fe - c);
            c = fe + 1;
        }
        if (cols.size() > 9 && !sites) sample_col = 9;
        if (sample && !sites) {
            sample_col = -1;
            for (size_t k = 9; k < cols.size(); ++k)
                if (cols[k] == sample) { sample_col = (int)k; break; }
            if (sample_col < 0)
                return bail(std::string(path) + ": line " + std::to_string(chrom_line) + ": the #CHROM line has no sample '" + sample + "'");
        }
    }
    // ---- the records
    std::vector<Row> rows;
    std::string msg;
    const Classifier classify{map, &dict, sample_col, passonly != 0, alleles};
    v->alleles = alleles;
    if (!scan_lines(v->file, at, n_before, threads, classify, &rows, &msg)) return bail(std::string(path) + ": " + msg);
    v->n_lines = rows.size();
    uint64_t n = 0, seq_bytes = 0;
    const uint8_t last_row_class = alleles ? SVX_VCFIN_A_ROW : SVX_VCFIN_INS;
    for (const Row& r : rows) {
        ++(alleles ? v->acounts : v->counts)[r.cls];
        if (r.cls <= last_row_class) { ++n; seq_bytes += r.seq_len; }
    }
    if (alleles) {
        v->pos.reserve(n); v->ref_off.reserve(n); v->ref_len.reserve(n); v->ref_text_len.reserve(n); v->phased.reserve(n);
    }
    v->type.reserve(n); v->gt.reserve(n); v->contig.reserve(n); v->start.reserve(n); v->end.reserve(n);
    v->seq_off.reserve(n); v->seq_len.reserve(n); v->line_off.reserve(n); v->line_len.reserve(n); v->line_no.reserve(n);
    v->id_off.reserve(n); v->id_len.reserve(n);
    v->seqs.resize(seq_bytes);
    uint64_t q = 0;
    for (const Row& r : rows) {
        if (r.cls > last_row_class) continue;
        if (alleles) {
            v->pos.push_back(r.end); v->ref_off.push_back(r.ref_off); v->ref_len.push_back(r.ref_len);
            v->ref_text_len.push_back(r.ref_text_len); v->phased.push_back(r.phased);
        }
        v->type.push_back(r.cls); v->gt.push_back(r.gt); v->contig.push_back(r.contig);
        v->start.push_back(r.start); v->end.push_back(r.end);
        v->seq_off.push_back(q); v->seq_len.push_back(r.seq_len);
        for (uint32_t k = 0; k < r.seq_len; ++k) v->seqs[q + k] = (uint8_t)upper(map[r.seq_off + k]);
        q += r.seq_len;
        v->line_off.push_back(r.line_off);
        v->line_len.push_back((uint32_t)std::min<uint64_t>(r.line_end - r.line_off, 0xFFFFFFFFu));
        v->line_no.push_back(r.line);
        v->id_off.push_back(r.id_off); v->id_len.push_back(r.id_len);
    }
    *out = v;
    return SVX_OK;
}

extern "C" int svx_vcfin_open(const char* path, int32_t n_ref, const char* const* names, const int64_t* lengths, const char* sample,
                              int passonly, int n_threads, svx_vcfin** out, char* err, size_t err_cap) {
    return open_vcf(path, n_ref, names, lengths, sample, false, false, passonly, n_threads, out, err, err_cap);
}

extern "C" int svx_vcfin_open_sites(const char* path, int32_t n_ref, const char* const* names, const int64_t* lengths, int passonly,
                                    int n_threads, svx_vcfin** out, char* err, size_t err_cap) {
    return open_vcf(path, n_ref, names, lengths, nullptr, true, false, passonly, n_threads, out, err, err_cap);
}

extern "C" int svx_vcfin_get_columns(const svx_vcfin* v, svx_vcfin_columns* out) {
    if (!v || !out || v->alleles) return SVX_E_INVALID;
    out->n = v->type.size();
    out->type = v->type.data(); out->contig = v->contig.data(); out->start = v->start.data(); out->end = v->end.data();
    out->gt = v->gt.data(); out->seq_off = v->seq_off.data(); out->seq_len = v->seq_len.data();
    out->seqs = v->seqs.data(); out->seq_bytes = v->seqs.size();
    out->line_off = v->line_off.data(); out->line_len = v->line_len.data(); out->line_no = v->line_no.data();
    out->id_off = v->id_off.data(); out->id_len = v->id_len.data();
    out->text = v->file.map; out->text_bytes = v->file.size; out->header_bytes = v->header_bytes; out->n_lines = v->n_lines;
    memcpy(out->counts, v->counts, sizeof(v->counts));
    return SVX_OK;
}

extern "C" int svx_vcfin_open_alleles(const char* path, int32_t n_ref, const char* const* names, const int64_t* lengths, const char* sample,
                                      int passonly, int n_threads, svx_vcfin** out, char* err, size_t err_cap) {
    return open_vcf(path, n_ref, names, lengths, sample, false, true, passonly, n_threads, out, err, err_cap);
}

extern "C" int svx_vcfin_get_alleles(const svx_vcfin* v, svx_vcfin_alleles* out) {
    if (!v || !out || !v->alleles) return SVX_E_INVALID;
    out->n = v->start.size();
    out->contig = v->contig.data(); out->start = v->start.data(); out->ref_len = v->ref_len.data();
    out->alt_off = v->seq_off.data(); out->alt_len = v->seq_len.data(); out->alts = v->seqs.data(); out->alt_bytes = v->seqs.size();
    out->pos = v->pos.data(); out->ref_off = v->ref_off.data(); out->ref_text_len = v->ref_text_len.data();
    out->gt = v->gt.data(); out->phased = v->phased.data();
    out->line_off = v->line_off.data(); out->line_len = v->line_len.data(); out->line_no = v->line_no.data();
    out->id_off = v->id_off.data(); out->id_len = v->id_len.data();
    out->text = v->file.map; out->text_bytes = v->file.size; out->header_bytes = v->header_bytes; out->n_lines = v->n_lines;
    memcpy(out->counts, v->acounts, sizeof(v->acounts));
    return SVX_OK;
}

extern "C" void svx_vcfin_close(svx_vcfin* v) { delete v; }
