// sam_sanitize.cpp — the native SAM reader and the host CIGAR-text parser (svim_asm_amd/csrc/svx_sam.cpp, the C-ABI of
// include/svx_sam.h) under AddressSanitizer / UBSan / ThreadSanitizer on the CPU: every entry point on well-formed files,
// then on damaged copies of them (changed bytes, truncations, tabs and line ends moved, runs of random bytes).  A damaged
// file may be refused with an error or read as whatever it now says; the reader must not touch memory it does not own.
// Test infrastructure (tests/test_sam_sanitizers.py builds and runs it); not part of the product.
//   sam_sanitize <scratch-dir> <mutations-per-file> <file.sam>...
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "svx_cigartext_dev.h"
#include "svx_sam.h"

// Stand-ins for the device launches (svx_cigartext.hip is not in this build): they fail like everything else that needs a
// device here, but with them registered a handle with a pinned device takes the device path's way in and its way back
// to the threads.
static int no_launch(void*, const uint8_t*, uint64_t, const uint64_t*, uint32_t, uint32_t*, uint64_t, uint64_t*, int32_t*, uint32_t*, void*) { return 1; }
static size_t no_ws(uint64_t, uint32_t) { return 256; }
extern "C" void svx_sam_register_device_parser(svx_cigar_text_launch_fn, svx_cigar_text_ws_fn);

static uint64_t g_sum = 0;  // keeps the reads of every column alive

static int walk(const char* path, int threads, bool per_contig) {
    char err[256] = {0};
    svx_sam* s = nullptr;
    if (svx_sam_open(path, threads, &s, err, sizeof err) != 0 || !s) return 1;  // refused: fine
    static unsigned turn = 0;
    if (++turn % 3 == 0) {  // no device here: every HIP call fails, the fall-backs run under the sanitizers
        static const bool registered = (svx_sam_register_device_parser(&no_launch, &no_ws), true);
        (void)registered;
        (void)svx_sam_set_pinned_device(s, 0);
        (void)svx_sam_set_device_parse(s, (int)((turn / 3) & 1));
    }
    const char* text = nullptr;
    uint64_t l_text = 0;
    int32_t n_ref = 0;
    if (svx_sam_header(s, &text, &l_text, &n_ref) == 0)
        for (uint64_t i = 0; i < l_text; ++i) g_sum += (uint8_t)text[i];
    for (int32_t t = -1; t <= n_ref; ++t) {
        const char* name = nullptr;
        int32_t len = 0;
        if (svx_sam_reference(s, t, &name, &len) == 0 && name) g_sum += strlen(name) + (uint32_t)len;
    }
    int rc_all = 0;
    for (int pass = 0; pass < (per_contig ? 2 : 1); ++pass) {
        int rc;
        if (pass == 0) {
            rc = svx_sam_load(s, nullptr, 0);
        } else {
            std::vector<int32_t> tids;
            for (int32_t t = 0; t < n_ref; t += 2) tids.push_back(t);
            rc = svx_sam_load(s, tids.data(), (int32_t)tids.size());
        }
        if (rc != 0) { g_sum += strlen(svx_sam_last_error(s)); rc_all = 1; continue; }
        svx_bam_columns c;
        if (svx_sam_get_columns(s, &c) != 0) continue;
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
                off.push_back(off.back() + (e0 > b0 ? e0 - b0 : 0));
            }
        }
        std::vector<uint8_t> out(off.back() + 1);
        if (!rec.empty() && svx_sam_seq_slices(s, rec.data(), begin.data(), end.data(), (uint32_t)rec.size(), off.data(), out.data()) == 0)
            for (uint8_t v : out) g_sum += v;
        const uint32_t beyond = (uint32_t)c.n_records;  // a record that does not exist: an error, not a read
        const uint32_t zero = 0, one = 1;
        const uint64_t o2[2] = {0, 1};
        uint8_t b1[2];
        g_sum += (uint64_t)svx_sam_seq_slices(s, &beyond, &zero, &one, 1, o2, b1);
        const uint32_t* d = nullptr;
        uint64_t n_ops = 0;
        void* ev = nullptr;
        double us = 0;
        g_sum += (uint64_t)svx_sam_device_pool(s, &d, &n_ops, &ev) + (uint64_t)svx_sam_device_pool_wait(s, &us) + (uint64_t)svx_sam_parsed_on_device(s);
    }
    svx_sam_close(s);
    return rc_all;
}

// the batch parser on its own: texts cut out of random bytes of the CIGAR alphabet, offsets with empty records
static void parser_fuzz(uint64_t* rng_state, int rounds) {
    uint64_t rng = *rng_state;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    static const char alphabet[] = "0123456789012345678901234567890123456789MIDNSHP=XMIDMIDMID*Qm \t-";
    for (int round = 0; round < rounds; ++round) {
        const uint64_t n_bytes = next() % 5000;
        std::vector<uint8_t> text(n_bytes + 1);
        for (uint64_t i = 0; i < n_bytes; ++i) text[i] = (next() % 200 == 0) ? (uint8_t)next() : (uint8_t)alphabet[next() % (sizeof alphabet - 1)];
        std::vector<uint64_t> off(1, 0);
        while (off.back() < n_bytes) {
            const uint64_t step = next() % 4 == 0 ? 0 : 1 + next() % 60;
            off.push_back(off.back() + step < n_bytes ? off.back() + step : n_bytes);
        }
        off.back() = n_bytes;
        const uint32_t n_rec = (uint32_t)off.size() - 1;
        const uint64_t cap = n_bytes / 2 + 1;
        std::vector<uint32_t> words(cap), status(n_rec + 1);
        std::vector<uint64_t> coff(n_rec + 1);
        std::vector<int32_t> ref_len(n_rec + 1);
        const int rc = svx_cigar_text_parse(text.data(), n_bytes, off.data(), n_rec, words.data(), cap, coff.data(), ref_len.data(), status.data(), 1 + (int)(next() % 4));
        if (rc == 0)
            for (uint64_t k = 0; k < coff[n_rec]; ++k) g_sum += words[k];
        for (uint32_t r = 0; r < n_rec; ++r) g_sum += status[r] + (uint32_t)ref_len[r];
        // arguments the entry refuses
        g_sum += (uint64_t)svx_cigar_text_parse(text.data(), n_bytes, off.data(), n_rec, words.data(), n_bytes / 2 > 0 ? n_bytes / 2 - 1 : 0, coff.data(), ref_len.data(), status.data(), 1);
        if (n_rec > 1 && off[1] > 0) {
            std::vector<uint64_t> bad = off;
            bad[1] = n_bytes + 5;
            g_sum += (uint64_t)svx_cigar_text_parse(text.data(), n_bytes, bad.data(), n_rec, words.data(), cap, coff.data(), ref_len.data(), status.data(), 2);
        }
    }
    *rng_state = rng;
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
    if (argc < 4) return 2;
    const std::string scratch = argv[1];
    const int n_mut = atoi(argv[2]);
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    parser_fuzz(&rng, 300);
    int refused = 0, read = 0;
    for (int a = 3; a < argc; ++a) {
        const std::string path = argv[a];
        if (walk(path.c_str(), 3, true) != 0) { fprintf(stderr, "well-formed file refused: %s\n", path.c_str()); return 1; }
        if (walk(path.c_str(), 1, false) != 0) return 1;
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
            } else if (kind == 4) {                // the header (first bytes: @SQ names and lengths)
                const size_t at = next() % (bad.size() < 200 ? bad.size() : 200);
                bad[at] = (uint8_t)next();
            } else {                               // a digit or operator of some CIGAR-like text changed
                const size_t at = next() % bad.size();
                for (size_t k = at; k < bad.size() && k < at + 4000; ++k)
                    if (bad[k] == 'M') { bad[k] = (uint8_t)"Q*9\t"[next() % 4]; break; }
            }
            const std::string p = scratch + "/mut.sam";
            spill(p, bad);
            (walk(p.c_str(), 1 + (int)(next() % 4), (next() & 1) != 0) ? refused : read)++;
        }
    }
    printf("sam_sanitize ok: %d damaged files refused, %d read, checksum %llu\n", refused, read, (unsigned long long)g_sum);
    return 0;
}
