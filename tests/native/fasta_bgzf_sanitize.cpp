// fasta_bgzf_sanitize.cpp — the bgzip-compressed FASTA handle (svim_asm_amd/csrc/svx_fasta_bgzf.cpp behind
// svx_fasta_open_bgzf, include/svx_text.h) under AddressSanitizer + UBSan or ThreadSanitizer on the CPU: random genomes
// (line widths 1..90, LF / CRLF, lower case and N runs) bgzipped at random member sizes, random windows fetched by
// several caller threads at once on one handle (the handle's own threads inside each call), the answers compared with
// the text; then damaged copies — flipped bytes, truncations, damaged .gzi columns — which may be refused at open or
// fail a fetch, and whose successful fetches must still be the text's bases.
// Test infrastructure (tests/test_fasta_bgzf_sanitizers.py builds and runs it); not part of the product.
//   fasta_bgzf_sanitize <scratch-dir> <genomes>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <random>
#include <string>
#include <thread>
#include <vector>

#include "svx_text.h"

namespace {

struct Genome {
    std::string text;  // the FASTA file
    std::vector<std::string> seq;
    std::vector<int64_t> length, offset;
    std::vector<int32_t> lb, lw;
};

Genome make_genome(std::mt19937_64& r) {
    Genome g;
    const int n = 1 + (int)(r() % 4);
    for (int k = 0; k < n; ++k) {
        const int64_t len = 1 + (int64_t)(r() % 40000);
        std::string s(len, 'A');
        for (auto& c : s) c = "ACGTNacgtn"[r() % 10];
        const int lb = 1 + (int)(r() % 90);
        const bool crlf = r() % 3 == 0;
        g.text += ">c" + std::to_string(k) + (crlf ? "\r\n" : "\n");
        g.offset.push_back((int64_t)g.text.size());
        for (int64_t p = 0; p < len; p += lb) g.text += s.substr(p, lb) + (crlf ? "\r\n" : "\n");
        g.length.push_back(len);
        g.lb.push_back(lb);
        g.lw.push_back(lb + (crlf ? 2 : 1));
        g.seq.push_back(s);
    }
    return g;
}

std::string member(const char* p, size_t n, int level) {
    std::vector<unsigned char> out(compressBound(n) + 64);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
    zs.next_in = (Bytef*)p;
    zs.avail_in = (uInt)n;
    zs.next_out = out.data();
    zs.avail_out = (uInt)out.size();
    deflate(&zs, Z_FINISH);
    const size_t clen = zs.total_out;
    deflateEnd(&zs);
    std::string m;
    const unsigned char hdr[18] = {0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 66, 67, 2, 0, 0, 0};
    m.assign((const char*)hdr, 18);
    const uint32_t bsize = (uint32_t)(clen + 25);
    m[16] = (char)(bsize & 0xFF);
    m[17] = (char)(bsize >> 8);
    m.append((const char*)out.data(), clen);
    const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)p, (uInt)n), isz = (uint32_t)n;
    for (int k = 0; k < 4; ++k) m.push_back((char)(crc >> (8 * k)));
    for (int k = 0; k < 4; ++k) m.push_back((char)(isz >> (8 * k)));
    return m;
}

struct Gz {
    std::string data;
    std::vector<uint64_t> coff, uoff;
};

Gz bgzip(const std::string& text, size_t msize, int level) {
    Gz z;
    for (size_t p = 0; p < text.size(); p += msize) {
        if (p) {
            z.coff.push_back(z.data.size());
            z.uoff.push_back(p);
        }
        z.data += member(text.data() + p, std::min(msize, text.size() - p), level);
    }
    z.data += member("", 0, level);  // end-of-file marker
    return z;
}

bool write_file(const std::string& path, const std::string& d) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(d.data(), 1, d.size(), f) == d.size();
    return fclose(f) == 0 && ok;
}

uint64_t g_ok = 0, g_refused = 0, g_failed = 0, g_wrong = 0;

// windows fetched by `callers` threads at once; true: every successful fetch equals the text
void fetch_round(svx_fasta* fa, const Genome& g, std::mt19937_64& r, int callers) {
    std::vector<std::thread> th;
    std::vector<uint64_t> seeds;
    for (int t = 0; t < callers; ++t) seeds.push_back(r());
    std::vector<int> okv(callers, 0), failv(callers, 0), wrongv(callers, 0);
    for (int t = 0; t < callers; ++t)
        th.emplace_back([&, t] {
            std::mt19937_64 q(seeds[t]);
            for (int call = 0; call < 4; ++call) {
                const uint32_t n = 1 + (uint32_t)(q() % (call == 0 ? 600 : 3));
                std::vector<int32_t> ref(n);
                std::vector<int64_t> st(n), en(n);
                std::vector<uint64_t> off(n + 1, 0);
                for (uint32_t i = 0; i < n; ++i) {
                    ref[i] = (int32_t)(q() % g.seq.size());
                    const int64_t L = g.length[ref[i]];
                    st[i] = (int64_t)(q() % (uint64_t)(L + 2));
                    en[i] = st[i] + (int64_t)(q() % 9000);
                    const int64_t e = std::min(en[i], L);
                    off[i + 1] = off[i] + (uint64_t)(e > st[i] ? e - st[i] : 0);
                }
                std::vector<uint8_t> out(off[n] + 1);
                const int upper = (int)(q() & 1);
                if (svx_fasta_fetch_batch(fa, ref.data(), st.data(), en.data(), n, upper, off.data(), out.data(), 1 + (int)(q() % 4)) != 0) {
                    ++failv[t];
                    (void)strlen(svx_fasta_last_error(fa));
                    continue;
                }
                ++okv[t];
                for (uint32_t i = 0; i < n; ++i)
                    for (uint64_t k = off[i]; k < off[i + 1]; ++k) {
                        char c = g.seq[ref[i]][(size_t)(st[i] + (int64_t)(k - off[i]))];
                        if (upper && c >= 'a' && c <= 'z') c = (char)(c - 32);
                        if ((char)out[k] != c) { ++wrongv[t]; break; }
                    }
            }
        });
    for (auto& x : th) x.join();
    for (int t = 0; t < callers; ++t) { g_ok += okv[t]; g_failed += failv[t]; g_wrong += wrongv[t]; }
    uint64_t stats[SVX_FASTA_STATS];
    (void)svx_fasta_stats(fa, stats);
}

void one(const std::string& path, const Gz& z, const Genome& g, std::mt19937_64& r) {
    if (!write_file(path, z.data)) return;
    char err[256];
    svx_fasta* fa = nullptr;
    if (svx_fasta_open_bgzf(path.c_str(), (int32_t)g.seq.size(), g.length.data(), g.offset.data(), g.lb.data(), g.lw.data(),
                            z.coff.data(), z.uoff.data(), z.coff.size(), &fa, err, sizeof err) != 0) {
        ++g_refused;
        return;
    }
    if (r() % 3 == 0) (void)svx_fasta_set_device(fa, 0, 1);  // (no device in this build: the host threads answer)
    fetch_round(fa, g, r, 1 + (int)(r() % 3));
    svx_fasta_close(fa);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int n = atoi(argv[2]);
    std::mt19937_64 r(12345);
    for (int i = 0; i < n; ++i) {
        const Genome g = make_genome(r);
        const Gz z = bgzip(g.text, 200 + r() % 9000, (int)(r() % 10));
        const std::string path = dir + "/g" + std::to_string(i % 4) + ".fa.gz";
        one(path, z, g, r);
        if (g_wrong) break;
        for (int k = 0; k < 3; ++k) {  // damaged copies
            Gz d = z;
            switch (r() % 4) {
                case 0: d.data[r() % d.data.size()] ^= (char)(1 << (r() % 8)); break;
                case 1: d.data.resize(r() % d.data.size()); break;
                case 2: if (!d.uoff.empty()) d.uoff[r() % d.uoff.size()] += 1 + r() % 3; break;
                default: if (!d.coff.empty()) d.coff[r() % d.coff.size()] ^= 1u << (r() % 12); break;
            }
            one(path, d, g, r);
        }
        if (g_wrong) break;
    }
    printf("fasta_bgzf_sanitize: %llu fetches ok, %llu failed, %llu opens refused, %llu wrong\n", (unsigned long long)g_ok,
           (unsigned long long)g_failed, (unsigned long long)g_refused, (unsigned long long)g_wrong);
    if (g_wrong) return 1;
    printf("fasta_bgzf_sanitize ok\n");
    return 0;
}
