// svx_fasta_bgzf.cpp — the bgzip-compressed form of the FASTA handle (svx_fasta_open_bgzf, include/svx_text.h), host C++.
//
// What htslib's faidx does with `ref.fa.gz` + `.fai` + `.gzi` (BGZF: SAM specification §4.1; the .gzi layout: a
// little-endian uint64 count, then (compressed, uncompressed) uint64 pairs, (0, 0) implicit).  The .fai offsets count
// uncompressed bytes; a window [start, end) of a sequence is the byte range fetch_one of svx_text.cpp reads, and the
// members under it are found by the uncompressed offsets of the member chain.
//
// Host path: the distinct members under a batch's windows are inflated once each (svx_bgzf.h's Inflater, two side by side)
// on up to 16 threads, CRC32 and ISIZE checked; then the windows are gathered from the inflated members.  Batches are cut
// into groups of at most kGroupMembers distinct members (in order of the windows' first member) so that a genome-wide call
// never holds more than that many inflated members at once.  A few recent members stay cached for the short fetches that
// follow each other (fetch() of the VCF's alleles).
//
// Device path (svx_fasta_set_device): the members not yet resident are staged through page-locked memory, inflated and
// checked by svx_inflate.hip's kernels into an arena that stays on the device for the handle's life, and the windows are
// gathered there by svx_fasta_gather.hip; the packed bytes come back to the caller's buffer.  Any failure to bring the
// device up sends the call to the host path (same bytes); a member the device finds damaged fails the call as on the host.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "svx.h"
#include "svx_bgzf.h"
#include "svx_fasta_bgzf.h"
#include "svx_text.h"

namespace {

using namespace svx_bgzf;  // Member, parse_member, Inflater, MemberTables

constexpr uint32_t kGroupMembers = 4096;   // inflated members a host call holds at once (256 MiB)
constexpr size_t kCacheMembers = 8;        // recent members kept between calls
constexpr uint64_t kArenaCap = 6ull << 30;  // device-resident inflated members of one handle

svx_inflate_launch_fn g_inflate = nullptr;   // svx_fasta_gather.hip registers the launches when the library loads
svx_fasta_gather_fn g_gather = nullptr;
svx_fasta_gather_oriented_fn g_gather_oriented = nullptr;
svx_inflate_arena_fn g_arena = nullptr;

bool host_only_env() {
    static const bool off = [] { const char* e = getenv("SVX_FASTA_DEVICE"); return e && e[0] == '0'; }();
    return off;
}

using Buf = std::shared_ptr<std::vector<uint8_t>>;

struct Fz {
    const uint8_t* map = nullptr;
    uint64_t fsize = 0, total = 0;
    std::vector<Member> mem;        // the chain, in file order
    std::vector<uint64_t> coff, uoff;  // where member i starts in the file / in the uncompressed text
    mutable std::mutex mu;          // everything below
    std::string err;
    std::vector<std::pair<uint32_t, Buf>> cache;  // most recent last
    uint64_t stat[SVX_FASTA_STATS] = {0, 0, 0, 0, 0, 0};
    // device
    int device = -1;
    uint32_t dev_min = 64;
    bool dev_broken = false;
    hipStream_t stream = nullptr;
    uint8_t* d_arena = nullptr;   // resident members
    uint64_t arena_cap = 0, arena_used = 0;
    std::vector<uint64_t> slot;   // arena offset of member i, ~0: not resident
    uint8_t* d_scratch = nullptr;  // a call's payloads, tables, token lists and packed output
    uint64_t scratch_cap = 0;
    uint8_t* h_stage = nullptr;    // page-locked staging
    uint64_t stage_cap = 0;

    // the member that holds uncompressed byte u (u < total): the last one starting at or before u (empty members
    // start where the next one does, so they are never it)
    uint32_t member_of(uint64_t u) const {
        return (uint32_t)(std::upper_bound(uoff.begin(), uoff.end(), u) - uoff.begin() - 1);
    }
    uint32_t next_nonempty(uint32_t m) const {
        uint32_t k = m + 1;
        while (k < mem.size() && mem[k].isize == 0) ++k;
        return k;
    }
    void set_err(const std::string& s) {
        std::lock_guard<std::mutex> g(mu);
        err = s;
    }
    void free_device() {
        if (device < 0 || (!stream && !d_arena && !d_scratch && !h_stage)) return;  // (nothing was brought up: no runtime call)
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (d_arena) (void)hipFree(d_arena);
        if (d_scratch) (void)hipFree(d_scratch);
        if (h_stage) (void)hipHostFree(h_stage);
        if (stream) (void)hipStreamDestroy(stream);
        (void)hipGetLastError();
        d_arena = d_scratch = h_stage = nullptr;
        stream = nullptr;
        arena_cap = arena_used = scratch_cap = stage_cap = 0;
        slot.assign(mem.size(), ~0ull);
    }
};

std::string member_msg(const char* what, uint64_t coff) {
    char buf[160];
    snprintf(buf, sizeof buf, "%s BGZF member at compressed offset %llu", what, (unsigned long long)coff);
    return buf;
}

// the uncompressed byte range of bases [s, e) of sequence r (as fetch_one of svx_text.cpp computes it)
inline void byte_range(const svx_fasta_geom* g, int32_t r, int64_t s, int64_t e, uint64_t* b0, uint64_t* b1) {
    const int64_t lb = g->line_bases[r], lw = g->line_width[r], off = g->offset[r];
    *b0 = (uint64_t)(off + (s / lb) * lw + s % lb);
    *b1 = (uint64_t)(off + ((e - 1) / lb) * lw + (e - 1) % lb + 1);
}

inline uint8_t ascii_upper(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }

// bases of [s, e) from raw bytes [b0, b1) into dst: line ends skipped, upper-cased when asked (fetch_one's loop)
void lines_to_bases(const svx_fasta_geom* g, int32_t r, int64_t s, int64_t e, bool upper, uint8_t* raw, size_t n, uint8_t* dst) {
    const int64_t lb = g->line_bases[r], lw = g->line_width[r];
    if (upper)
        for (size_t i = 0; i < n; ++i) raw[i] = ascii_upper(raw[i]);
    const uint8_t* src = raw;
    int64_t left = e - s;
    int64_t take = std::min<int64_t>(lb - s % lb, left);
    for (;;) {
        memcpy(dst, src, (size_t)take);
        dst += take;
        left -= take;
        if (left <= 0) break;
        src += take + (lw - lb);
        take = std::min<int64_t>(lb, left);
    }
}

int run_threads(int n_threads, const std::function<void()>& fn) {
    if (n_threads <= 1) {
        fn();
        return SVX_OK;
    }
    try {
        std::vector<std::thread> th;
        for (int t = 0; t < n_threads; ++t) th.emplace_back(fn);
        for (std::thread& t : th) t.join();
    } catch (...) {
        return SVX_E_NOMEM;
    }
    return SVX_OK;
}

// ------------------------------------------------------------------ open / close
int z_open(const uint8_t* map, uint64_t size, const uint64_t* gzi_coff, const uint64_t* gzi_uoff, uint64_t n_gzi, void** out,
           char* err, size_t err_cap) {
    auto fail = [&](const std::string& s) {
        if (err && err_cap) snprintf(err, err_cap, "%s", s.c_str());
        return SVX_E_INVALID;
    };
    std::unique_ptr<Fz> z(new (std::nothrow) Fz());
    if (!z) return SVX_E_NOMEM;
    z->map = map;
    z->fsize = size;
    // the .gzi behind the implicit (0, 0) (an explicit one in front is tolerated): compressed offsets strictly increasing,
    // uncompressed ones not decreasing — an empty member in the middle (bgzip files concatenated, each with its end-of-file
    // marker) starts where the next member does; the walk below checks every entry against the members' ISIZE
    uint64_t g0 = (n_gzi && gzi_coff[0] == 0 && gzi_uoff[0] == 0) ? 1 : 0;
    for (uint64_t i = g0; i < n_gzi; ++i) {
        const uint64_t pc = i > g0 ? gzi_coff[i - 1] : 0, pu = i > g0 ? gzi_uoff[i - 1] : 0;
        if (gzi_coff[i] <= pc || gzi_uoff[i] < pu) return fail("the .gzi index is not increasing (entry " + std::to_string(i) + ")");
        if (gzi_coff[i] > size) return fail("the .gzi index points past the end of the file (entry " + std::to_string(i) + ")");
    }
    // the member chain, every .gzi entry on one of its headers with the uncompressed offset the chain gives
    try {
        uint64_t coff = 0, u = 0, gi = g0;
        while (coff < size) {
            while (gi < n_gzi && gzi_coff[gi] < coff)
                return fail("the .gzi entry " + std::to_string(gi) + " does not point at a BGZF member header");
            if (gi < n_gzi && gzi_coff[gi] == coff) {
                if (gzi_uoff[gi] != u) return fail("the .gzi entry " + std::to_string(gi) + " disagrees with the members' sizes");
                ++gi;
            }
            Member m;
            if (parse_member(map, size, coff, &m) != 0)
                return fail(member_msg("truncated or malformed", coff) + " (not a complete BGZF file)");
            z->mem.push_back(m);
            z->coff.push_back(coff);
            z->uoff.push_back(u);
            coff += m.bsize;
            u += m.isize;
        }
        // what is left may only be the end entry (end of the data)
        for (; gi < n_gzi; ++gi)
            if (gzi_coff[gi] != size || gzi_uoff[gi] != u) return fail("the .gzi index points past the end of the data");
        z->total = u;
        z->slot.assign(z->mem.size(), ~0ull);
    } catch (...) {
        return SVX_E_NOMEM;
    }
    if (z->mem.empty()) return fail("empty BGZF file");
    *out = z.release();
    return SVX_OK;
}

void z_close(void* p) {
    Fz* z = static_cast<Fz*>(p);
    if (!z) return;
    z->free_device();
    delete z;
}

// ------------------------------------------------------------------ host path
struct Win {
    uint32_t i;       // window index
    uint32_t m0, m1;  // first and last member under it
    uint64_t b0, b1;
};

// a window's bases as they lie in the file -> reversed and complemented when asked, every byte through the direction's table
void orient(uint8_t* dst, size_t n, bool reversed, const uint8_t* tabs) {
    if (reversed) std::reverse(dst, dst + n);
    const uint8_t* t = tabs + (reversed ? 256 : 0);
    for (size_t i = 0; i < n; ++i) dst[i] = t[dst[i]];
}

int host_fetch(Fz* z, const svx_fasta_geom* g, const int32_t* ref, const int64_t* start, const int64_t* end,
               const uint8_t* reverse, const uint8_t* tabs, bool upper, const uint64_t* out_off, uint8_t* out, int n_threads, std::vector<Win>& wins) {
    std::sort(wins.begin(), wins.end(), [](const Win& a, const Win& b) { return a.m0 != b.m0 ? a.m0 < b.m0 : a.i < b.i; });
    {
        std::lock_guard<std::mutex> lk(z->mu);
        ++z->stat[5];
    }
    size_t w_lo = 0;
    while (w_lo < wins.size()) {
        // one group: windows in order of their first member until kGroupMembers distinct members are under them
        std::vector<uint32_t> ms;
        size_t w_hi = w_lo;
        uint32_t last = ~0u;
        while (w_hi < wins.size()) {
            const Win& w = wins[w_hi];
            const uint32_t from = last == ~0u ? w.m0 : std::max(w.m0, last + 1);
            const uint32_t add = w.m1 >= from ? w.m1 - from + 1 : 0;
            if (w_hi > w_lo && ms.size() + add > kGroupMembers) break;
            for (uint32_t m = from; add && m <= w.m1; ++m) ms.push_back(m);
            last = last == ~0u ? w.m1 : std::max(last, w.m1);
            ++w_hi;
        }
        // (ms: sorted and distinct by construction)  members from the cache, the rest inflated
        std::vector<Buf> bufs(ms.size());
        std::vector<uint32_t> todo;
        {
            std::lock_guard<std::mutex> lk(z->mu);
            for (size_t k = 0; k < ms.size(); ++k) {
                for (const auto& c : z->cache)
                    if (c.first == ms[k]) { bufs[k] = c.second; break; }
                if (bufs[k]) ++z->stat[3];
                else todo.push_back((uint32_t)k);
            }
        }
        std::atomic<size_t> next(0);
        std::atomic<int64_t> bad(-1);
        try {
            for (uint32_t k : todo) bufs[k] = std::make_shared<std::vector<uint8_t>>(z->mem[ms[k]].isize);
        } catch (...) {
            return SVX_E_NOMEM;
        }
        auto inflate_work = [&]() {  // two members at a time, each whole into its buffer; the first damaged one is named
            Inflater inf[2] = {Inflater(false), Inflater(false)};  // (the build's own decoder whatever SVX_BAM_ZLIB says)
            for (;;) {
                const size_t t = next.fetch_add(2);
                if (t >= todo.size() || bad.load() >= 0) break;
                const size_t n = std::min<size_t>(2, todo.size() - t);
                const uint8_t* in[2] = {nullptr, nullptr};
                uint8_t* dst[2] = {nullptr, nullptr};
                size_t in_len[2] = {0, 0}, isize[2] = {0, 0};
                uint32_t crc[2] = {0, 0};
                bool ok[2];
                for (size_t k = 0; k < n; ++k) {
                    const uint32_t m = ms[todo[t + k]];
                    in[k] = z->map + z->coff[m] + z->mem[m].payload_off;
                    in_len[k] = z->mem[m].payload_len;
                    dst[k] = bufs[todo[t + k]]->data();
                    isize[k] = z->mem[m].isize;
                    crc[k] = z->mem[m].crc;
                }
                if (!Inflater::run_two(inf, in, in_len, dst, isize, isize, crc, n, ok)) bad.store(ms[todo[t + (ok[0] ? 1 : 0)]]);
            }
        };
        int rc = run_threads(todo.size() >= 8 ? n_threads : 1, inflate_work);
        if (rc != SVX_OK) return rc;
        {
            std::lock_guard<std::mutex> lk(z->mu);
            z->stat[0] += todo.size();
        }
        if (bad.load() >= 0) {
            z->set_err(member_msg("damaged or malformed", z->coff[(size_t)bad.load()]) + " (CRC32, ISIZE or DEFLATE stream)");
            return SVX_E_INVALID;
        }
        // gather
        std::atomic<size_t> wnext(w_lo);
        auto gather_work = [&]() {
            std::vector<uint8_t> raw;
            for (;;) {
                const size_t w = wnext.fetch_add(64);
                if (w >= w_hi) break;
                for (size_t j = w; j < std::min(w_hi, w + 64); ++j) {
                    const Win& W = wins[j];
                    const size_t nb = (size_t)(W.b1 - W.b0);
                    raw.resize(nb);
                    uint64_t u = W.b0;
                    size_t k = (size_t)(std::lower_bound(ms.begin(), ms.end(), W.m0) - ms.begin());
                    for (uint32_t m = W.m0; m <= W.m1; ++m, ++k) {
                        const uint64_t hi = std::min<uint64_t>(W.b1, z->uoff[m] + z->mem[m].isize);
                        if (hi > u) {
                            memcpy(raw.data() + (u - W.b0), bufs[k]->data() + (u - z->uoff[m]), (size_t)(hi - u));
                            u = hi;
                        }
                    }
                    const int64_t e = std::min(end[W.i], g->length[ref[W.i]]);
                    lines_to_bases(g, ref[W.i], start[W.i], e, upper, raw.data(), nb, out + out_off[W.i]);
                    if (tabs) orient(out + out_off[W.i], (size_t)(e - start[W.i]), reverse && reverse[W.i], tabs);
                }
            }
        };
        rc = run_threads(w_hi - w_lo >= 256 ? n_threads : 1, gather_work);
        if (rc != SVX_OK) return rc;
        // the group's last members stay cached
        {
            std::lock_guard<std::mutex> lk(z->mu);
            for (size_t k = ms.size() > kCacheMembers ? ms.size() - kCacheMembers : 0; k < ms.size(); ++k) {
                auto it = std::find_if(z->cache.begin(), z->cache.end(), [&](const std::pair<uint32_t, Buf>& c) { return c.first == ms[k]; });
                if (it != z->cache.end()) z->cache.erase(it);
                z->cache.emplace_back(ms[k], bufs[k]);
            }
            if (z->cache.size() > kCacheMembers) z->cache.erase(z->cache.begin(), z->cache.end() - (long)kCacheMembers);
        }
        w_lo = w_hi;
    }
    return SVX_OK;
}

// ------------------------------------------------------------------ device path
// 1: done; 0: not taken (the caller runs the host path); < 0: a status to return
int device_fetch(Fz* z, const svx_fasta_geom* g, const int32_t* ref, const int64_t* start, const int64_t* end,
                 const uint8_t* reverse, const uint8_t* tabs, bool upper, const uint64_t* out_off, uint8_t* out, uint64_t out_lo, uint64_t out_bytes, int n_threads, const std::vector<Win>& wins) {
    std::lock_guard<std::mutex> lk(z->mu);  // one device call of a handle at a time (arena, scratch, stream)
    if (z->device < 0 || z->dev_broken || !g_inflate || !g_gather || !g_arena || (tabs && !g_gather_oriented) || host_only_env()) return 0;
    std::vector<uint32_t> ms;
    for (const Win& w : wins)
        for (uint32_t m = w.m0; m <= w.m1; ++m) ms.push_back(m);
    std::sort(ms.begin(), ms.end());
    ms.erase(std::unique(ms.begin(), ms.end()), ms.end());
    if (ms.size() < z->dev_min) return 0;
    auto broken = [&]() {  // the device could not be used: the host path from here on
        (void)hipGetLastError();
        z->free_device();
        z->dev_broken = true;
        return 0;
    };
    if (hipSetDevice(z->device) != hipSuccess) return broken();
    if (!z->stream && hipStreamCreateWithFlags(&z->stream, hipStreamNonBlocking) != hipSuccess) return broken();
    // the members not resident yet, and room for them in the arena
    std::vector<uint32_t> fresh;
    MemberTables mt(z->arena_used);  // (mt.out_off[k]: the arena slot member fresh[k] will have)
    for (uint32_t m : ms) {
        if (z->slot[m] != ~0ull) continue;
        fresh.push_back(m);
        mt.add(z->map, z->coff[m], z->mem[m]);
    }
    const uint64_t in_bytes = mt.in_bytes;
    z->stat[3] += ms.size() - fresh.size();
    if (mt.out_end > z->arena_cap) {
        if (mt.out_end > kArenaCap) return 0;  // (past the cap: this call on the host)
        uint64_t cap = std::max<uint64_t>(64ull << 20, 2 * z->arena_cap);
        while (cap < mt.out_end) cap *= 2;
        cap = std::min(cap, kArenaCap);
        void* p = nullptr;
        if (hipMalloc(&p, cap) != hipSuccess) return broken();
        if (z->arena_used && hipMemcpyAsync(p, z->d_arena, z->arena_used, hipMemcpyDeviceToDevice, z->stream) != hipSuccess) {
            (void)hipFree(p);
            return broken();
        }
        if (z->d_arena) {
            (void)hipStreamSynchronize(z->stream);
            (void)hipFree(z->d_arena);
        }
        z->d_arena = static_cast<uint8_t*>(p);
        z->arena_cap = cap;
    }
    // the chunks of the gather: up to SVX_FASTA_CHUNK_BASES bases of a window inside two members
    std::vector<svx_fasta_chunk> chunks;
    bool unplanned = false;  // (a member neither resident nor staged: never, by construction — checked all the same)
    auto slot_of = [&](uint32_t m) -> uint64_t {
        if (z->slot[m] != ~0ull) return z->slot[m];
        const size_t k = (size_t)(std::lower_bound(fresh.begin(), fresh.end(), m) - fresh.begin());
        if (k == fresh.size() || fresh[k] != m) {
            unplanned = true;
            return 0;
        }
        return mt.out_off[k];
    };
    for (const Win& w : wins) {
        const int32_t r = ref[w.i];
        const uint64_t lb = (uint64_t)g->line_bases[r], lw = (uint64_t)g->line_width[r], off = (uint64_t)g->offset[r];
        const uint64_t e = (uint64_t)std::min(end[w.i], g->length[r]);
        uint32_t shift = 0;
        uint64_t magic = 0;
        if (e < (1ull << 31) && lb < (1ull << 31)) {
            uint32_t c = 0;
            while ((1ull << c) < lb) ++c;
            shift = 31 + c;
            magic = ((1ull << shift) / lb) + 1;
        }
        // A reversed window is cut exactly like a forward one, in ascending SOURCE order, so that a chunk's bytes lie in
        // two members at most whichever way its lanes walk them; only its place in the output differs: source bases
        // [s, s + n) of a window that ends at e are output bases [e - s - n, e - s) of it (lane k: source s + n - 1 - k).
        const bool rev = tabs && reverse && reverse[w.i];
        uint64_t s = (uint64_t)start[w.i], o = out_off[w.i];
        while (s < e) {
            const uint64_t u0 = off + (s / lb) * lw + s % lb;
            const uint32_t ma = z->member_of(u0);
            // member b only where the window reaches it (a member behind the window may be neither resident nor staged)
            const uint32_t nb = z->next_nonempty(ma);
            const uint32_t mb = nb <= w.m1 ? nb : (uint32_t)z->mem.size();
            const uint64_t lim = mb < z->mem.size() ? z->uoff[mb] + z->mem[mb].isize : z->uoff[ma] + z->mem[ma].isize;
            const uint64_t rel = lim - off;  // bases in front of byte `lim`
            const uint64_t before = (rel / lw) * lb + std::min<uint64_t>(rel % lw, lb);
            const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(e, before) - s, SVX_FASTA_CHUNK_BASES);
            svx_fasta_chunk c;
            c.out = rev ? out_off[w.i] + (e - s - n) : o;
            c.reverse = rev ? 1u : 0u;
            c.pad = 0;
            c.off = off;
            c.s0 = s;
            c.src_a = slot_of(ma);
            c.u_a = z->uoff[ma];
            c.src_b = mb < z->mem.size() ? slot_of(mb) : c.src_a;
            c.u_b = mb < z->mem.size() ? z->uoff[mb] : ~0ull;
            c.magic = magic;
            c.shift = shift;
            c.n = (uint32_t)n;
            c.line_bases = (uint32_t)lb;
            c.line_width = (uint32_t)lw;
            chunks.push_back(c);
            s += n;
            o += n;
        }
    }
    if (unplanned) return 0;
    // scratch: payloads | the member tables (MemberTables::write) | status | n_tok (u32) | chunks | packed output | tokens
    const uint32_t nf = (uint32_t)fresh.size();
    auto up256 = [](uint64_t x) { return (x + 255) & ~255ull; };
    const uint32_t arena_members = std::min<uint32_t>(nf, std::max<uint32_t>(1u, g_arena()));
    const uint64_t o_in = 0, o_tab = up256(in_bytes + 8);
    const uint64_t o_status = o_tab + up256(mt.bytes()), o_ntok = o_status + up256((uint64_t)nf * 4);
    const uint64_t o_chunks = o_ntok + up256((uint64_t)nf * 4);
    const uint64_t o_tabs = o_chunks + up256(chunks.size() * sizeof(svx_fasta_chunk));  // (the oriented gather's two tables)
    const uint64_t o_packed = o_tabs + (tabs ? 512 : 0);
    const uint64_t o_tok = o_packed + up256(out_bytes + 8);
    const uint64_t need = o_tok + (nf ? up256((uint64_t)arena_members * SVX_INFLATE_TOK_STRIDE * 8) : 0);
    const uint64_t stage_need = tabs ? o_tabs + 512 : o_chunks + chunks.size() * sizeof(svx_fasta_chunk);  // everything that goes up
    if (z->scratch_cap < need) {
        if (z->d_scratch) {
            (void)hipStreamSynchronize(z->stream);
            (void)hipFree(z->d_scratch);
        }
        z->d_scratch = nullptr;
        z->scratch_cap = 0;
        void* p = nullptr;
        if (hipMalloc(&p, need + (need >> 3)) != hipSuccess) return broken();
        z->d_scratch = static_cast<uint8_t*>(p);
        z->scratch_cap = need + (need >> 3);
    }
    if (z->stage_cap < std::max(stage_need, out_bytes)) {
        (void)hipStreamSynchronize(z->stream);
        if (z->h_stage) (void)hipHostFree(z->h_stage);
        z->h_stage = nullptr;
        z->stage_cap = 0;
        const uint64_t want = std::max(stage_need, out_bytes);
        void* p = nullptr;
        if (hipHostMalloc(&p, want + (want >> 3), hipHostMallocDefault) != hipSuccess) return broken();
        z->h_stage = static_cast<uint8_t*>(p);
        z->stage_cap = want + (want >> 3);
    }
    // stage: the payloads (by the threads), the tables, the chunks
    uint8_t* h = z->h_stage;
    std::atomic<uint32_t> next(0);
    auto stage = [&]() {
        for (;;) {
            const uint32_t k0 = next.fetch_add(64);
            if (k0 >= nf) break;
            for (uint32_t k = k0; k < std::min(nf, k0 + 64); ++k) memcpy(h + o_in + mt.in_off[k], mt.src[k], mt.in_len[k]);
        }
    };
    int rc = run_threads(nf >= 256 ? n_threads : 1, stage);
    if (rc != SVX_OK) return rc;
    mt.write(h + o_tab);
    if (!chunks.empty()) memcpy(h + o_chunks, chunks.data(), chunks.size() * sizeof(svx_fasta_chunk));
    if (tabs) {
        memset(h + o_chunks + chunks.size() * sizeof(svx_fasta_chunk), 0, o_tabs - o_chunks - chunks.size() * sizeof(svx_fasta_chunk));
        memcpy(h + o_tabs, tabs, 512);
    }
    uint8_t* d = z->d_scratch;
    bool ok = hipMemcpyAsync(d, h, stage_need, hipMemcpyHostToDevice, z->stream) == hipSuccess;
    z->stat[2] += in_bytes;
    if (ok && nf)
        ok = mt.launch(g_inflate, z->stream, d + o_in, d + o_tab, 0, nf, z->d_arena, reinterpret_cast<uint32_t*>(d + o_status),
                       reinterpret_cast<uint32_t*>(d + o_ntok), d + o_tok, arena_members) == 0;
    if (tabs)
        ok = ok && g_gather_oriented(z->stream, z->d_arena, reinterpret_cast<const svx_fasta_chunk*>(d + o_chunks), (uint32_t)chunks.size(),
                                     d + o_tabs, d + o_packed) == 0;
    else
        ok = ok && g_gather(z->stream, z->d_arena, reinterpret_cast<const svx_fasta_chunk*>(d + o_chunks), (uint32_t)chunks.size(),
                            upper ? 1 : 0, d + o_packed) == 0;
    std::vector<uint32_t> status(nf);
    ok = ok && (nf == 0 || hipMemcpyAsync(status.data(), d + o_status, (size_t)nf * 4, hipMemcpyDeviceToHost, z->stream) == hipSuccess);
    ok = ok && (out_bytes == out_lo ||
                hipMemcpyAsync(h + out_lo, d + o_packed + out_lo, out_bytes - out_lo, hipMemcpyDeviceToHost, z->stream) == hipSuccess);
    ok = ok && hipStreamSynchronize(z->stream) == hipSuccess;
    if (!ok) return broken();  // (the host path takes the call; nothing of it was written yet)
    for (uint32_t k = 0; k < nf; ++k)
        if (status[k] != 0) {
            // nothing of this call becomes resident: the arena ends where it did
            z->err = member_msg("damaged or malformed", z->coff[fresh[k]]) + " (CRC32, ISIZE or DEFLATE stream; device)";
            return SVX_E_INVALID;
        }
    for (uint32_t k = 0; k < nf; ++k) z->slot[fresh[k]] = mt.out_off[k];
    z->arena_used = mt.out_end;
    z->stat[1] += nf;
    ++z->stat[4];
    if (out_bytes > out_lo) memcpy(out + out_lo, h + out_lo, out_bytes - out_lo);
    return 1;
}

int z_fetch(void* p, const svx_fasta_geom* g, const int32_t* ref, const int64_t* start, const int64_t* end, const uint8_t* reverse,
            const uint8_t* tabs, uint32_t n, int upper, const uint64_t* out_off, uint8_t* out, int n_threads) {
    Fz* z = static_cast<Fz*>(p);
    if (n_threads <= 0) n_threads = (int)std::min<unsigned>(16u, std::max<unsigned>(1u, std::thread::hardware_concurrency()));
    n_threads = std::min(n_threads, 16);
    std::vector<Win> wins;
    try {
        wins.reserve(n);
    } catch (...) {
        return SVX_E_NOMEM;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const int32_t r = ref[i];
        const int64_t e = std::min(end[i], g->length[r]);
        if (e <= start[i]) continue;
        if (g->line_bases[r] <= 0 || g->line_width[r] < g->line_bases[r] || g->offset[r] < 0) {
            z->set_err("bad .fai geometry");
            return SVX_E_INVALID;
        }
        Win w;
        w.i = i;
        byte_range(g, r, start[i], e, &w.b0, &w.b1);
        if (w.b1 > z->total || w.b1 <= w.b0) {
            z->set_err("reference windows shorter than the index says");
            return SVX_E_INVALID;
        }
        w.m0 = z->member_of(w.b0);
        w.m1 = z->member_of(w.b1 - 1);
        wins.push_back(w);
    }
    if (wins.empty()) return SVX_OK;
    const int d = device_fetch(z, g, ref, start, end, reverse, tabs, upper != 0, out_off, out, out_off[0], out_off[n], n_threads, wins);
    if (d < 0) return d;
    if (d == 1) return SVX_OK;
    return host_fetch(z, g, ref, start, end, reverse, tabs, upper != 0, out_off, out, n_threads, wins);
}

int z_set_device(void* p, int device, uint32_t min_members) {
    Fz* z = static_cast<Fz*>(p);
    std::lock_guard<std::mutex> lk(z->mu);
    if (device != z->device) {
        z->free_device();
        z->dev_broken = false;
    }
    z->device = device < 0 ? -1 : device;
    z->dev_min = min_members;
    return SVX_OK;
}

void z_stats(const void* p, uint64_t* out) {
    const Fz* z = static_cast<const Fz*>(p);
    std::lock_guard<std::mutex> lk(z->mu);
    for (int k = 0; k < SVX_FASTA_STATS; ++k) out[k] = z->stat[k];
}

const char* z_last_error(const void* p) {
    // a copy owned by the calling thread: another thread's failing fetch may replace the handle's message meanwhile
    thread_local std::string copy;
    const Fz* z = static_cast<const Fz*>(p);
    std::lock_guard<std::mutex> lk(z->mu);
    copy = z->err;
    return copy.c_str();
}

const svx_fasta_bgzf_ops kOps = {z_open, z_close, z_fetch, z_set_device, z_stats, z_last_error};
[[maybe_unused]] const int kRegistered = (svx_fasta_register_bgzf(&kOps), 0);

}  // namespace

extern "C" void svx_fasta_register_device(svx_inflate_launch_fn inflate, svx_fasta_gather_fn gather,
                                          svx_fasta_gather_oriented_fn gather_oriented, svx_inflate_arena_fn arena) {
    g_inflate = inflate;
    g_gather = gather;
    g_gather_oriented = gather_oriented;
    g_arena = arena;
}
