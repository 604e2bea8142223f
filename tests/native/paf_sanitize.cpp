// paf_sanitize.cpp — the native PAF reader (svim_asm_amd/csrc/svx_paf.cpp behind include/svx_paf.h, with the CIGAR path of
// svx_sam.cpp and the oriented fetch of svx_text.cpp) under AddressSanitizer / UBSan / ThreadSanitizer on the CPU: every
// entry point on well-formed files, then on damaged copies (changed bytes, truncations, tabs and line ends moved, runs of
// random bytes, CIGAR letters changed).  A damaged file may be refused or read as whatever it now says; the reader must
// not touch memory it does not own.  Test infrastructure (tests/test_paf_sanitizers.py builds and runs it).
//   paf_sanitize <scratch-dir> <mutations-per-file> <reference.fai> <query.fa> <file.paf> [<query.fa> <file.paf>]...
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "svx_cigartext_dev.h"
#include "svx_paf.h"

static int no_launch(void*, const uint8_t*, uint64_t, const uint64_t*, uint32_t, uint32_t*, uint64_t, uint64_t*, int32_t*, uint32_t*, void*) { return 1; }
static size_t no_ws(uint64_t, uint32_t) { return 256; }
extern "C" void svx_sam_register_device_parser(svx_cigar_text_launch_fn, svx_cigar_text_ws_fn);

static uint64_t g_sum = 0;

struct Fai {
    std::vector<std::string> name;
    std::vector<int64_t> length, offset;
    std::vector<int32_t> line_bases, line_width;
    std::vector<const char*> ptr;
    std::vector<int32_t> length32;
};

static Fai read_fai(const std::string& path) {
    Fai f;
    FILE* fh = fopen(path.c_str(), "r");
    if (!fh) return f;
    char name[512];
    long long a, b;
    int c, d;
    while (fscanf(fh, "%511s %lld %lld %d %d", name, &a, &b, &c, &d) == 5) {
        f.name.push_back(name);
        f.length.push_back(a); f.offset.push_back(b); f.line_bases.push_back(c); f.line_width.push_back(d);
        f.length32.push_back((int32_t)a);
    }
    fclose(fh);
    for (const std::string& s : f.name) f.ptr.push_back(s.c_str());
    return f;
}

static int walk(const char* path, const Fai& ref, const svx_fasta* query, const Fai& qfai, int threads, bool per_contig) {
    char err[256] = {0};
    svx_paf* p = nullptr;
    if (svx_paf_open(path, (int32_t)ref.name.size(), ref.ptr.data(), ref.length32.data(), threads, &p, err, sizeof err) != 0 || !p) return 1;
    static unsigned turn = 0;
    if (++turn % 3 == 0) {  // no device here: every HIP call fails, the fall-backs run under the sanitizers
        static const bool registered = (svx_sam_register_device_parser(&no_launch, &no_ws), true);
        (void)registered;
        (void)svx_paf_set_pinned_device(p, 0);
        (void)svx_paf_set_device_parse(p, (int)((turn / 3) & 1));
    }
    if (turn % 5 != 0) (void)svx_paf_set_query(p, query, (int32_t)qfai.name.size(), qfai.ptr.data(), qfai.length.data());
    const char* text = nullptr;
    uint64_t l_text = 0;
    int32_t n_ref = 0;
    if (svx_paf_header(p, &text, &l_text, &n_ref) == 0)
        for (uint64_t i = 0; i < l_text; ++i) g_sum += (uint8_t)text[i];
    for (int32_t t = -1; t <= n_ref; ++t) {
        const char* name = nullptr;
        int32_t len = 0;
        if (svx_paf_reference(p, t, &name, &len) == 0 && name) g_sum += strlen(name) + (uint32_t)len;
    }
    int rc_all = 0;
    for (int pass = 0; pass < (per_contig ? 2 : 1); ++pass) {
        int rc;
        if (pass == 0) {
            rc = svx_paf_load(p, nullptr, 0);
        } else {
            std::vector<int32_t> tids;
            for (int32_t t = 0; t < n_ref; t += 2) tids.push_back(t);
            rc = svx_paf_load(p, tids.data(), (int32_t)tids.size());
        }
        if (rc != 0) { g_sum += strlen(svx_paf_last_error(p)); rc_all = 1; continue; }
        svx_bam_columns c;
        if (svx_paf_get_columns(p, &c) != 0) continue;
        for (uint64_t r = 0; r < c.n_records; ++r) {
            g_sum += (uint32_t)c.tid[r] + (uint32_t)c.pos[r] + (uint32_t)c.l_seq[r] + (uint32_t)c.ref_len[r] + c.flag[r] + c.mapq[r] + c.voffset[r];
            for (uint64_t k = c.cigar_off[r]; k < c.cigar_off[r + 1]; ++k) g_sum += c.cigar[k];
            for (uint64_t k = c.name_off[r]; k < c.name_off[r + 1]; ++k) g_sum += (uint8_t)c.names[k];
            for (uint64_t k = c.aux_off[r]; k < c.aux_off[r + 1]; ++k) g_sum += c.aux[k];
            if (c.sa_off[r] >= 0)
                for (uint32_t k = 0; k < c.sa_len[r]; ++k) g_sum += c.aux[(uint64_t)c.sa_off[r] + k];
        }
        const uint32_t n = (uint32_t)(c.n_records < 600 ? c.n_records : 600);
        std::vector<uint32_t> rec, begin, end;
        std::vector<uint64_t> off(1, 0);
        for (uint32_t r = 0; r < n; ++r) {
            const uint32_t l = c.l_seq[r] > 0 ? (uint32_t)c.l_seq[r] : 0u;
            const uint32_t cases[3][2] = {{0, l < 5000 ? l : 5000}, {l / 3, l / 3 + 77}, {l, l + 100}};
            for (auto& cs : cases) {
                rec.push_back(r); begin.push_back(cs[0]); end.push_back(cs[1]);
                const uint32_t b0 = cs[0] < l ? cs[0] : l, e0 = cs[1] < l ? cs[1] : l;
                off.push_back(off.back() + (e0 > b0 ? e0 - b0 : 0) + (r % 7 == 0 ? 3 : 0));  // (some slots wider than their slices)
            }
        }
        std::vector<uint8_t> out(off.back() + 1);
        if (!rec.empty()) {
            if (svx_paf_seq_slices(p, rec.data(), begin.data(), end.data(), (uint32_t)rec.size(), off.data(), out.data()) == 0) {
                for (uint32_t i = 0; i < rec.size(); ++i) {
                    const uint32_t l = (uint32_t)c.l_seq[rec[i]], b0 = begin[i] < l ? begin[i] : l, e0 = end[i] < l ? end[i] : l;
                    for (uint64_t k = 0; k < (e0 > b0 ? e0 - b0 : 0); ++k) g_sum += out[off[i] + k];
                }
            } else {
                g_sum += strlen(svx_paf_last_error(p));
            }
        }
        const uint32_t beyond = (uint32_t)c.n_records, zero = 0, one = 1;
        const uint64_t o2[2] = {0, 1};
        uint8_t b1[2];
        g_sum += (uint64_t)svx_paf_seq_slices(p, &beyond, &zero, &one, 1, o2, b1);
        const uint32_t* d = nullptr;
        uint64_t n_ops = 0;
        void* ev = nullptr;
        double us = 0;
        g_sum += (uint64_t)svx_paf_device_pool(p, &d, &n_ops, &ev) + (uint64_t)svx_paf_device_pool_wait(p, &us) + (uint64_t)svx_paf_parsed_on_device(p);
    }
    svx_paf_close(p);
    return rc_all;
}

static std::vector<uint8_t> slurp(const std::string& p) {
    std::vector<uint8_t> v;
    FILE* f = fopen(p.c_str(), "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize(n > 0 ? (size_t)n : 0);
    if (n > 0 && fread(v.data(), 1, v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}

static void spill(const std::string& p, const std::vector<uint8_t>& v) {
    FILE* f = fopen(p.c_str(), "wb");
    if (!f) return;
    if (!v.empty()) fwrite(v.data(), 1, v.size(), f);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 6 || (argc - 4) % 2 != 0) return 2;
    const std::string scratch = argv[1];
    const int n_mut = atoi(argv[2]);
    const Fai ref = read_fai(argv[3]);
    if (ref.name.empty()) return 2;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    int refused = 0, read = 0;
    for (int a = 4; a + 1 < argc; a += 2) {
        const std::string qpath = argv[a], path = argv[a + 1];
        const Fai qfai = read_fai(qpath + ".fai");
        svx_fasta* query = nullptr;
        char err[256];
        if (svx_fasta_open(qpath.c_str(), (int32_t)qfai.name.size(), qfai.length.data(), qfai.offset.data(), qfai.line_bases.data(),
                           qfai.line_width.data(), &query, err, sizeof err) != 0) { fprintf(stderr, "query FASTA: %s\n", err); return 1; }
        if (walk(path.c_str(), ref, query, qfai, 3, true) != 0) { fprintf(stderr, "well-formed file refused: %s\n", path.c_str()); return 1; }
        if (walk(path.c_str(), ref, query, qfai, 1, false) != 0) return 1;
        const std::vector<uint8_t> good = slurp(path);
        for (int m = 0; m < n_mut && !good.empty(); ++m) {
            std::vector<uint8_t> bad = good;
            const uint64_t kind = next() % 6;
            if (kind == 0) {                       // a few changed bytes anywhere
                for (int k = 0; k < 1 + (int)(next() % 4); ++k) bad[next() % bad.size()] ^= (uint8_t)(1u << (next() % 8));
            } else if (kind == 1) {                // truncated
                bad.resize(next() % bad.size());
            } else if (kind == 2) {                // a tab or a line end removed, or put where none was
                std::vector<size_t> seps;
                for (size_t k = 0; k < bad.size(); ++k) if (bad[k] == '\t' || bad[k] == '\n') seps.push_back(k);
                if (!seps.empty() && (next() & 1)) bad[seps[next() % seps.size()]] = 'x';
                else bad[next() % bad.size()] = (next() & 1) ? '\t' : '\n';
            } else if (kind == 3) {                // a run of random bytes
                const size_t at = next() % bad.size(), len = 1 + next() % 32;
                for (size_t k = at; k < at + len && k < bad.size(); ++k) bad[k] = (uint8_t)next();
            } else if (kind == 4) {                // a digit of some number column changed (spans, lengths, MAPQ)
                const size_t at = next() % bad.size();
                for (size_t k = at; k < bad.size() && k < at + 4000; ++k)
                    if (bad[k] >= '0' && bad[k] <= '9') { bad[k] = (uint8_t)('0' + next() % 10); break; }
            } else {                               // an operator of some CIGAR changed
                const size_t at = next() % bad.size();
                for (size_t k = at; k < bad.size() && k < at + 4000; ++k)
                    if (bad[k] == 'M') { bad[k] = (uint8_t)"Q*9\tID"[next() % 6]; break; }
            }
            const std::string p = scratch + "/mut.paf";
            spill(p, bad);
            (walk(p.c_str(), ref, query, qfai, 1 + (int)(next() % 4), (next() & 1) != 0) ? refused : read)++;
        }
        svx_fasta_close(query);
    }
    printf("paf_sanitize ok: %d damaged files refused, %d read, checksum %llu\n", refused, read, (unsigned long long)g_sum);
    return 0;
}
