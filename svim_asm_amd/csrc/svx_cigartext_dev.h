// svx_cigartext_dev.h — how svx_textaln.cpp reaches the device parser of svx_cigartext.hip: through pointers that the
// kernels' translation unit registers when the library loads (svx_textaln.cpp also builds alone, for the CPU sanitizer tests).
#pragma once
#include <stddef.h>
#include <stdint.h>

// the launches of svx_cigar_text_parse_dev on `stream`; d_ws: svx_cigar_text_ws_fn(n_bytes, n_rec) bytes.  hipError_t as int.
typedef int (*svx_cigar_text_launch_fn)(void* stream, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                                        uint32_t* d_words, uint64_t cap, uint64_t* d_cigar_off, int32_t* d_ref_len, uint32_t* d_status,
                                        void* d_ws);
typedef size_t (*svx_cigar_text_ws_fn)(uint64_t n_bytes, uint32_t n_rec);
