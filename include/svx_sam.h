/*
 * svx_sam.h — C-ABI of the native SAM ingest of libsvx.so: what minimap2 writes (`minimap2 -a ... > hap.sam`), read
 * as it is — uncompressed text, records in ANY order, no index — into the same columns as svx_bam.h.
 *
 * The reference opens its input with `pysam.AlignmentFile(path)` (svim-asm:63-90) and then requires a coordinate-sorted
 * file (`header["HD"]["SO"]`, svim-asm:64,86) with an index (`check_index()`, svim-asm:67-72) because `bam.fetch(contig)`
 * (SVIM_COLLECT.py:65) needs both: in practice a user runs `samtools sort` and `samtools index` on every haplotype first.
 * Nothing behind the reader needs a sorted FILE: COLLECT needs the records grouped by contig in coordinate order, one flat
 * pool of BAM CIGAR words, the SA strings and a few bases per insertion.  A genome-genome SAM has 10^3..10^4 records with
 * very long lines, so this reader orders the RECORDS in memory and fills svx_bam_columns (svx_bam.h) with them.
 *
 * ORDER (this reader's definition): records are presented sorted by (tid, pos, reverse-strand flag 0x10, position in the
 * file); records whose RNAME is `*` (tid -1) come last, among themselves in the same order.  This is meant to be the
 * comparison of `samtools sort`; that program is not available where this was written, so the statement above — and not
 * "what samtools does" — is what the tests pin.
 *
 * Lines: the file is memory-mapped and cut into pieces at line ends; the handle's threads find the line ends with memchr
 * and, per line, the first eleven tabs.  SEQ and QUAL (10^5..10^8 bytes) are skipped by memchr and never copied.  A `\r`
 * in front of the line end is dropped (htslib does the same); empty lines are skipped.  Fields:
 *   tid    RNAME looked up among the @SQ names (`*`: -1)        pos    POS - 1            flag, mapq   as written
 *   l_seq  bytes of SEQ (0 for `*`)                              names  QNAME
 *   aux    the optional fields re-encoded as BAM binary aux (SAM spec §4.2.4): `A`; `i` as the smallest of c/C/s/S/i/I
 *          that holds the value (htslib's choice: the unsigned type for a value >= 0); `f`; `Z`; `H`; `B`
 *   cigar  the CIGAR string as BAM words `len << 4 | op` — parsed on the pinned device (svx_cigar_text_parse_dev's kernels) or
 *          by the handle's threads (svx_cigar_text_parse), see svx_sam_set_device_parse; `*`: no words
 *   ref_len  Σ len over {M,D,N,=,X}                              voffset  BYTE OFFSET of the line in the file
 * blocks_inflated and blocks_spanned are 0.
 * Refused with SVX_E_INVALID and the 1-based line number in svx_sam_last_error: fewer than 11 fields; FLAG, POS or MAPQ not
 * a number in range; an RNAME that no @SQ line names; a CIGAR the parser rejects; a CIGAR whose query-consuming length
 * (M,I,S,=,X) differs from l_seq when both are present; an optional field that is not TAG:TYPE:VALUE of a known type.
 * svx_sam_open refuses a file without @SQ lines, and a gzip- or bgzip-compressed file (with a message that names the two
 * accepted forms: uncompressed SAM, or BAM through svx_bam_open).
 *
 * All functions return SVX_OK (0) or a negative svx_status (svx.h).  A handle is used by one thread at a time.  Pointers
 * handed out stay valid until the next svx_sam_load on the handle or svx_sam_close.
 */
#ifndef SVX_SAM_H_
#define SVX_SAM_H_

#include <stddef.h>
#include <stdint.h>

#include "svx.h"
#include "svx_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svx_sam svx_sam;

/* Open `path` (memory-mapped) and parse the header lines (every leading line that starts with `@`) and their @SQ SN/LN
 * fields.  n_threads <= 0: one per hardware thread, at most 64. */
int svx_sam_open(const char* path, int n_threads, svx_sam** out, char* err, size_t err_cap);
void svx_sam_close(svx_sam* sam);
const char* svx_sam_last_error(const svx_sam* sam);
int svx_sam_header(const svx_sam* sam, const char** text, uint64_t* l_text, int32_t* n_ref);
int svx_sam_reference(const svx_sam* sam, int32_t tid, const char** name, int32_t* length);

/* As svx_bam_set_pinned_device: the CIGAR pool of later loads is page-locked in the context of HIP device `device` and has
 * a copy in HBM (svx_sam_device_pool); device < 0 (default): pageable memory, no copy. */
int svx_sam_set_pinned_device(svx_sam* sam, int device);
/* Who turns the CIGAR text into words when a pinned device is set.  on != 0: the device (the gathered text goes up, the
 * kernels of svx_cigar_text_parse_dev write the pool where svx_collect_batch wants it, a page-locked host copy comes back
 * for svx_bam_columns.cigar); 0: the handle's threads (svx_cigar_text_parse), and the finished pool is uploaded.  Either way
 * the columns are the same; without a pinned device, or when the device cannot be used, the threads do it. */
int svx_sam_set_device_parse(svx_sam* sam, int on);
/* 1 when the last load's words were written by the device, 0 when by the threads. */
int svx_sam_parsed_on_device(const svx_sam* sam);

/* Index the records of contigs tids[0..n_tids) (NULL: every record, unplaced ones included) in the ORDER defined above. */
int svx_sam_load(svx_sam* sam, const int32_t* tids, int32_t n_tids);
int svx_sam_get_columns(const svx_sam* sam, svx_bam_columns* out);

/* Bases [begin[i], end[i]) of record rec[i] at out + out_off[i], as svx_bam_seq_slices: every byte goes through the mapping
 * of a BAM round trip (4-bit code and back: lower case -> upper, anything outside =ACMGRSVTWYHKDBN -> N). */
int svx_sam_seq_slices(svx_sam* sam, const uint32_t* rec, const uint32_t* begin, const uint32_t* end, uint32_t n,
                       const uint64_t* out_off, uint8_t* out);

/* As svx_bam_device_pool / svx_bam_device_pool_wait. */
int svx_sam_device_pool(svx_sam* sam, const uint32_t** d_cigar, uint64_t* n_ops, void** ready);
int svx_sam_device_pool_wait(svx_sam* sam, double* waited_us);

/*
 * CIGAR text -> words.  text[n_bytes]: the CIGAR strings of n_rec records back to back; rec_off[n_rec + 1], rec_off[0] = 0,
 * non-decreasing, rec_off[n_rec] = n_bytes.  Per record: status[r] (0, or the code of the error that comes FIRST in the
 * text; two at the same byte: the smaller code), ref_len[r], and its words at words[cigar_off[r] .. cigar_off[r + 1]).
 * A record with an error has no words and ref_len 0, its neighbours are not affected.  `*` alone: no words, no error.
 * A number may have leading zeros; its VALUE must be below 2^28.  cap (words `words` can hold) must be at least
 * n_bytes / 2 — an operation is two bytes at least.
 */
enum {
    SVX_CIGAR_OK = 0,
    SVX_CIGAR_BAD_CHAR = 1,         /* a byte that is no digit, no letter and no `=`; a `*` that is not the whole text   */
    SVX_CIGAR_BAD_OP = 2,           /* a letter outside MIDNSHPX (lower case included)                                    */
    SVX_CIGAR_EMPTY_NUMBER = 3,     /* an operator without digits in front of it; a text of no bytes                     */
    SVX_CIGAR_NUMBER_TOO_BIG = 4,   /* a length of 2^28 or more                                                          */
    SVX_CIGAR_TRAILING_DIGITS = 5   /* the text ends in a digit (reported at its last byte)                               */
};
/* On the host, by n_threads threads (<= 0: one per hardware thread, at most 64): the path without a device and the
 * device parser's oracle. */
int svx_cigar_text_parse(const uint8_t* text, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, uint32_t* words,
                         uint64_t cap, uint64_t* cigar_off, int32_t* ref_len, uint32_t* status, int n_threads);
/* On the device: every pointer is a device address, the launches are ordered on the context's stream (workspace from the
 * context); results are complete when the stream is (svx_ctx_sync, svx_dev_download). */
int svx_cigar_text_parse_dev(svx_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                             uint32_t* d_words, uint64_t cap, uint64_t* d_cigar_off, int32_t* d_ref_len, uint32_t* d_status);

#ifdef __cplusplus
}
#endif
#endif /* SVX_SAM_H_ */
