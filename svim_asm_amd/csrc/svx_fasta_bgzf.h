// svx_fasta_bgzf.h — what svx_text.cpp (the FASTA handle) and svx_fasta_bgzf.cpp (its bgzip-compressed form) agree on.
// svx_text.cpp also builds alone (tests/test_text_sanitizers.py): it reaches the compressed form only through the table
// svx_fasta_bgzf.cpp registers when the library loads.
#pragma once
#include <stddef.h>
#include <stdint.h>

// the .fai columns of a handle (uncompressed offsets)
struct svx_fasta_geom {
    int32_t n_refs;
    const int64_t* length;
    const int64_t* offset;
    const int32_t* line_bases;
    const int32_t* line_width;
};

struct svx_fasta_bgzf_ops {
    // the member chain of the mapped file, checked against the .gzi columns; *z: the state of the compressed form
    int (*open)(const uint8_t* map, uint64_t size, const uint64_t* gzi_coff, const uint64_t* gzi_uoff, uint64_t n_gzi,
                void** z, char* err, size_t err_cap);
    void (*close)(void* z);
    // svx_fasta_fetch_batch on the compressed form (arguments already checked against the geometry); with tabs != NULL
    // svx_fasta_fetch_oriented: tabs[0..256) maps the bytes of a window as it lies, tabs[256..512) those of a window with
    // reverse[i] != 0 (reverse == NULL: none), which is written back to front
    int (*fetch)(void* z, const svx_fasta_geom* g, const int32_t* ref, const int64_t* start, const int64_t* end,
                 const uint8_t* reverse, const uint8_t* tabs, uint32_t n, int upper, const uint64_t* out_off, uint8_t* out, int n_threads);
    int (*set_device)(void* z, int device, uint32_t min_members);
    void (*stats)(const void* z, uint64_t* out);  // SVX_FASTA_STATS words
    const char* (*last_error)(const void* z);
};
extern "C" void svx_fasta_register_bgzf(const svx_fasta_bgzf_ops* ops);

// The device gather of the compressed form (svx_fasta_gather.hip): one chunk = up to kFastaChunkBases output bases of one
// window whose bytes lie in at most two members (a and the next non-empty one, b) resident in the device arena.
#define SVX_FASTA_CHUNK_BASES 32768u
struct svx_fasta_chunk {
    uint64_t out;      // where its first base goes in the packed output
    uint64_t off;      // uncompressed offset of the sequence's first base (.fai column 3)
    uint64_t s0;       // index of its first base in the sequence
    uint64_t src_a;    // arena offsets of members a and b
    uint64_t src_b;
    uint64_t u_a;      // uncompressed offsets of members a and b (u_b: where a ends)
    uint64_t u_b;
    uint64_t magic;    // s / line_bases == (s * magic) >> shift for s < 2^31 (0: plain division)
    uint32_t n;        // bases
    uint32_t line_bases;
    uint32_t line_width;
    uint32_t shift;
    uint32_t reverse;  // the oriented gather only: lane k takes source base s0 + n - 1 - k
    uint32_t pad;
};
typedef int (*svx_fasta_gather_fn)(void* stream, const uint8_t* d_arena, const svx_fasta_chunk* d_chunks, uint32_t n_chunks,
                                   int upper, uint8_t* d_out);
// the oriented form: d_tabs[512], the two tables of svx_fasta_bgzf_ops::fetch
typedef int (*svx_fasta_gather_oriented_fn)(void* stream, const uint8_t* d_arena, const svx_fasta_chunk* d_chunks, uint32_t n_chunks,
                                            const uint8_t* d_tabs, uint8_t* d_out);
typedef uint32_t (*svx_inflate_arena_fn)(void);

#include "svx_inflate_dev.h"
// svx_fasta_gather.hip hands its launches (and the inflate of svx_inflate.hip) to svx_fasta_bgzf.cpp this way
extern "C" void svx_fasta_register_device(svx_inflate_launch_fn inflate, svx_fasta_gather_fn gather,
                                          svx_fasta_gather_oriented_fn gather_oriented, svx_inflate_arena_fn arena);
