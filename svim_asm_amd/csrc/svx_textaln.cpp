// svx_textaln.cpp — the part of the alignment ingest that is the same for every text front end (svx_textaln.h): the
// mapped file, and the Columns a load fills.  The CIGAR strings a front end gathered back to back become BAM words either
// by the kernels of svx_cigartext.hip on the pinned device (the pool is then born in HBM and a page-locked copy comes
// back) or by svx_cigar_text_parse below on the threads (and the pool is uploaded), svx_sam_set_device_parse.
// This file also builds alone with a host compiler (tests/native/sam_sanitize.cpp): the kernels are reached through
// pointers that svx_cigartext.hip registers.
#include "svx_textaln.h"

#include <fcntl.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <mutex>

#include "svx_cigartext_dev.h"
#include "svx_sam.h"

namespace svx_textaln {

namespace {

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

// The device's turn: text and offsets up, the kernels, offsets / ref_len / status back, then the words into a page-locked
// pool of exactly their size.  false: nothing of it is left behind and the threads take over.
bool parse_on_device(Columns* s, uint64_t n_text, const std::vector<uint64_t>& rec_off, std::vector<uint32_t>* status) {
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
        s->release_pool();
        s->h_text = keep;
        s->h_text_pinned = keep_pinned;
        return false;
    }
    s->d_valid = s->n_ops != 0;
    return true;
}

}  // namespace

const uint8_t* bam_alphabet() { return kSeqMap.m; }

MappedText::Found MappedText::open(const char* path) {
    fd = ::open(path, O_RDONLY);
    if (fd < 0) return CANNOT_OPEN;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return NOT_REGULAR;
    size = (size_t)st.st_size;
    if (size) {
        void* p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) return CANNOT_MAP;
        map = (const char*)p;
    }
    return size >= 2 && (uint8_t)map[0] == 0x1f && (uint8_t)map[1] == 0x8b ? GZIP : OK;
}

void MappedText::close() {
    if (map) munmap((void*)map, size);
    if (fd >= 0) ::close(fd);
    map = nullptr;
    fd = -1;
}

Columns::~Columns() {
    if (pin_device >= 0 && (cigar_pinned || d_cigar || d_tmp || h_text_pinned)) {
        if (hipSetDevice(pin_device) != hipSuccess) (void)hipGetLastError();
    }
    release_pool();
    if (ready) { (void)hipEventDestroy(ready); (void)hipGetLastError(); }
}

void Columns::release_pool() {
    if (d_valid && ready) (void)hipEventSynchronize(ready);
    d_valid = false;
    if (cigar) {
        if (cigar_pinned) (void)hipHostFree(cigar);
        else free(cigar);
    }
    cigar = nullptr;
    cigar_pinned = false;
    if (d_cigar) (void)hipFree(d_cigar);
    d_cigar = nullptr;
    if (d_tmp) (void)hipFree(d_tmp);
    d_tmp = nullptr;
    if (h_text) {
        if (h_text_pinned) (void)hipHostFree(h_text);
        else free(h_text);
    }
    h_text = nullptr;
    (void)hipGetLastError();
    n_ops = 0;
}

void Columns::begin_load() {
    if (pin_device >= 0 && hipSetDevice(pin_device) != hipSuccess) (void)hipGetLastError();
    release_pool();
    n = 0;
    parsed_on_device = 0;
}

void Columns::resize(uint64_t n_records) {
    n = n_records;
    tid.resize(n); pos.resize(n); l_seq.resize(n); ref_len.assign(n, 0); flag.resize(n); mapq.resize(n);
    voffset.resize(n); sa_off.resize(n); sa_len.resize(n);
    cigar_off.assign(n + 1, 0); name_off.assign(n + 1, 0); aux_off.assign(n + 1, 0);
    names.clear();
    aux.clear();
}

bool Columns::alloc_text(uint64_t n_text) {
    const bool want_device = pin_device >= 0 && device_parse && g_launch && n_text > 0;
    if (want_device && hipHostMalloc((void**)&h_text, n_text + 1, hipHostMallocDefault) == hipSuccess) {
        h_text_pinned = true;
    } else {
        (void)hipGetLastError();
        h_text = (uint8_t*)malloc(n_text + 1);
        h_text_pinned = false;
    }
    return h_text != nullptr;
}

int Columns::finish_cigars(const std::vector<uint64_t>& rec_off, const std::vector<uint32_t>& line_of, const char* seq_what) {
    const uint64_t n_text = rec_off[n];
    const bool want_device = h_text_pinned;
    std::vector<uint32_t> status(n, 0);
    if (want_device && parse_on_device(this, n_text, rec_off, &status)) {
        parsed_on_device = 1;
    } else {
        std::vector<uint64_t> ops(n);
        parallel_for(n_threads, n, [&](uint64_t r) {
            uint32_t rl;
            status[r] = parse_one(h_text, rec_off[r], rec_off[r + 1], nullptr, &ops[r], &rl);
            ref_len[r] = (int32_t)rl;
        });
        for (uint64_t r = 0; r < n; ++r) cigar_off[r + 1] = cigar_off[r] + ops[r];
        n_ops = cigar_off[n];
        if (n_ops) {
            if (pin_device >= 0 && hipSetDevice(pin_device) == hipSuccess &&
                hipHostMalloc((void**)&cigar, n_ops * 4, hipHostMallocDefault) == hipSuccess) {
                cigar_pinned = true;
            } else {
                (void)hipGetLastError();
                cigar = (uint32_t*)malloc(n_ops * 4);
                if (!cigar) return fail(SVX_E_NOMEM, "no memory for the CIGAR pool");
            }
        }
        parallel_for(n_threads, n, [&](uint64_t r) {
            if (status[r] != SVX_CIGAR_OK || ops[r] == 0) return;
            uint64_t k;
            uint32_t rl;
            (void)parse_one(h_text, rec_off[r], rec_off[r + 1], cigar + cigar_off[r], &k, &rl);
        });
    }
    for (uint64_t r = 0; r < n; ++r)
        if (status[r] != SVX_CIGAR_OK) {
            const uint32_t st = status[r];
            const uint32_t line = line_of[r];
            release_pool();
            n = 0;
            return fail(SVX_E_INVALID, "line " + std::to_string(line) + ": the CIGAR has " + cigar_status_text(st));
        }
    // query-consuming length against SEQ where both are present
    std::atomic<int64_t> bad(-1);
    parallel_for(n_threads, n, [&](uint64_t r) {
        if (l_seq[r] == 0 || cigar_off[r + 1] == cigar_off[r]) return;
        uint64_t q = 0;
        for (uint64_t k = cigar_off[r]; k < cigar_off[r + 1]; ++k)
            if ((0x193u >> (cigar[k] & 15)) & 1u) q += cigar[k] >> 4;  // M I S = X
        if (q != (uint64_t)l_seq[r]) {
            int64_t none = -1;
            bad.compare_exchange_strong(none, (int64_t)r);
        }
    });
    if (bad.load() >= 0) {
        const uint32_t line = line_of[(size_t)bad.load()];
        release_pool();
        n = 0;
        return fail(SVX_E_INVALID, "line " + std::to_string(line) + ": the CIGAR's query length differs from " + seq_what);
    }
    // the threads' pool goes up to where svx_collect_batch wants it
    if (!parsed_on_device && cigar_pinned && n_ops) {
        hipStream_t st = device_stream(pin_device);
        bool ok = st != nullptr && hipMalloc((void**)&d_cigar, n_ops * 4) == hipSuccess;
        if (ok && !ready) ok = hipEventCreateWithFlags(&ready, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipMemcpyAsync(d_cigar, cigar, n_ops * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipEventRecord(ready, st) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (st) (void)hipStreamSynchronize(st);
            if (d_cigar) (void)hipFree(d_cigar);
            (void)hipGetLastError();
            d_cigar = nullptr;
        }
        d_valid = ok;
    }
    if (h_text && !h_text_pinned) { free(h_text); h_text = nullptr; }  // (a page-locked one waits for close: freeing it waits for the device)
    return SVX_OK;
}

int Columns::get_columns(svx_bam_columns* c) const {
    if (!c) return SVX_E_INVALID;
    memset(c, 0, sizeof *c);
    c->n_records = n;
    c->tid = tid.data(); c->pos = pos.data(); c->l_seq = l_seq.data(); c->ref_len = ref_len.data();
    c->flag = flag.data(); c->mapq = mapq.data(); c->cigar_off = cigar_off.data(); c->cigar = cigar;
    c->name_off = name_off.data(); c->names = names.data(); c->aux_off = aux_off.data(); c->aux = aux.data();
    c->sa_off = sa_off.data(); c->sa_len = sa_len.data(); c->voffset = voffset.data();
    c->cigar_pinned = cigar_pinned ? 1 : 0;
    c->n_threads = n_threads;
    return SVX_OK;
}

int Columns::device_pool(const uint32_t** d_cigar_out, uint64_t* n_ops_out, void** ready_out) const {
    if (d_cigar_out) *d_cigar_out = d_valid ? d_cigar : nullptr;
    if (n_ops_out) *n_ops_out = d_valid ? n_ops : 0;
    if (ready_out) *ready_out = d_valid ? (void*)ready : nullptr;
    return SVX_OK;
}

int Columns::device_pool_wait(double* waited_us) {
    if (waited_us) *waited_us = 0;
    if (!d_valid) return SVX_OK;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipEventSynchronize(ready) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SVX_E_HIP, "svx_sam_device_pool_wait: the CIGAR pool's copy in HBM failed");
    }
    if (waited_us) *waited_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return SVX_OK;
}

}  // namespace svx_textaln

using namespace svx_textaln;

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
