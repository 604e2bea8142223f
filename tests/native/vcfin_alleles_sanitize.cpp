// vcfin_alleles_sanitize.cpp — the VCF reader's list of edits (svx_vcfin_open_alleles / svx_vcfin_get_alleles in
// svim_asm_amd/csrc/svx_vcfin.cpp behind include/svx_vcfin.h, compiled with svx_sam.cpp, the line scanner svx_textaln.cpp
// and the BGZF member layer svx_bgzf.cpp) under AddressSanitizer / UBSan / ThreadSanitizer on the CPU:
// the valid files, then the first file truncated at every byte, then seeded byte flips of every file (plain and BGZF).
// A damaged file may be refused or read as whatever it now says; the reader must not touch memory it does not own.
// Test infrastructure (tests/test_vcfin_alleles_sanitizers.py builds and runs it).
//   vcfin_alleles_sanitize <scratch-dir> <flips-per-file> <reference.fai> <small.vcf> [<file.vcf[.gz]>]...
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "svx_vcfin.h"

static uint64_t g_sum = 0;
static uint64_t g_read = 0, g_refused = 0;

struct Fai {
    std::vector<std::string> name;
    std::vector<int64_t> length;
    std::vector<const char*> ptr;
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
        f.length.push_back(a);
    }
    fclose(fh);
    for (const std::string& s : f.name) f.ptr.push_back(s.c_str());
    return f;
}

// every byte the columns point to is read once
static void walk(const char* path, const Fai& ref, const char* sample, int passonly, int threads) {
    char err[256] = {0};
    svx_vcfin* v = nullptr;
    if (svx_vcfin_open_alleles(path, (int32_t)ref.name.size(), ref.ptr.data(), ref.length.data(), sample, passonly, threads, &v, err, sizeof err) != 0 || !v) {
        ++g_refused;
        g_sum += strlen(err);
        return;
    }
    ++g_read;
    svx_vcfin_alleles c;
    svx_vcfin_columns other;
    if (svx_vcfin_get_columns(v, &other) == 0) { fprintf(stderr, "svx_vcfin_get_columns took a handle of the other kind\n"); exit(1); }
    if (svx_vcfin_get_alleles(v, &c) == 0) {
        for (uint64_t i = 0; i < c.n; ++i) {
            g_sum += (uint64_t)c.contig[i] + (uint64_t)c.start[i] + c.ref_len[i] + (uint64_t)c.pos[i] + c.gt[i] + c.phased[i] + c.line_no[i];
            for (uint32_t k = 0; k < c.alt_len[i]; ++k) g_sum += c.alts[c.alt_off[i] + k];
            for (uint32_t k = 0; k < c.ref_text_len[i]; ++k) g_sum += (uint8_t)c.text[c.ref_off[i] + k];
            for (uint32_t k = 0; k < c.line_len[i]; ++k) g_sum += (uint8_t)c.text[c.line_off[i] + k];
            for (uint32_t k = 0; k < c.id_len[i]; ++k) g_sum += (uint8_t)c.text[c.id_off[i] + k];
        }
        for (uint64_t k = 0; k < c.header_bytes; ++k) g_sum += (uint8_t)c.text[k];
        for (int k = 0; k < SVX_VCFIN_A_N_CLASSES; ++k) g_sum += c.counts[k];
        if (c.alt_bytes) g_sum += c.alts[c.alt_bytes - 1];
    }
    svx_vcfin_close(v);
}

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> out;
    FILE* fh = fopen(path, "rb");
    if (!fh) return out;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, fh)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(fh);
    return out;
}

static bool spill(const std::string& path, const uint8_t* p, size_t n) {
    FILE* fh = fopen(path.c_str(), "wb");
    if (!fh) return false;
    const bool ok = n == 0 || fwrite(p, 1, n, fh) == n;
    fclose(fh);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: vcfin_alleles_sanitize <scratch-dir> <flips-per-file> <reference.fai> <small.vcf> [<file>]...\n");
        return 2;
    }
    const std::string scratch = argv[1];
    const int flips = atoi(argv[2]);
    const Fai ref = read_fai(argv[3]);
    if (ref.name.empty()) { fprintf(stderr, "no contigs in %s\n", argv[3]); return 2; }
    // ---- the valid files, every way of opening them
    for (int f = 4; f < argc; ++f) {
        const uint64_t before = g_read;
        for (int threads : {1, 4}) {
            walk(argv[f], ref, nullptr, 0, threads);
            walk(argv[f], ref, nullptr, 1, threads);
            walk(argv[f], ref, "no-such-sample", 0, threads);
        }
        if (g_read - before < 4) { fprintf(stderr, "%s was refused\n", argv[f]); return 1; }
    }
    walk((scratch + "/missing.vcf").c_str(), ref, nullptr, 0, 1);
    // ---- the small file cut at every byte
    const std::vector<uint8_t> small = slurp(argv[4]);
    const std::string tmp = scratch + "/damaged.vcf";
    for (size_t n = 0; n < small.size(); ++n) {
        if (!spill(tmp, small.data(), n)) return 2;
        walk(tmp.c_str(), ref, nullptr, (int)(n & 1), 1 + (int)(n % 3));
    }
    // ---- seeded byte flips of every file
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    for (int f = 4; f < argc; ++f) {
        const std::vector<uint8_t> good = slurp(argv[f]);
        if (good.empty()) continue;
        for (int k = 0; k < flips; ++k) {
            std::vector<uint8_t> bad = good;
            const int n_flips = 1 + (int)(next() % 4);
            for (int j = 0; j < n_flips; ++j) {
                const size_t at = (size_t)(next() % bad.size());
                const uint64_t r = next();
                // a tab, a line end, a digit or any byte: what moves columns and lines
                bad[at] = (r & 3) == 0 ? '\t' : (r & 3) == 1 ? '\n' : (r & 3) == 2 ? (uint8_t)('0' + (r >> 8) % 10) : (uint8_t)(r >> 8);
            }
            if (!spill(tmp, bad.data(), bad.size())) return 2;
            walk(tmp.c_str(), ref, (k % 5 == 0) ? "S2" : nullptr, k & 1, 1 + k % 4);
        }
    }
    printf("vcfin_alleles_sanitize ok: %llu read, %llu refused, checksum %llu\n", (unsigned long long)g_read, (unsigned long long)g_refused,
           (unsigned long long)g_sum);
    return 0;
}
