/*
 * svx_paf.h — C-ABI of the native PAF ingest of libsvx.so: what `minimap2 -c` writes (PAF with the `cg:Z:` CIGAR), read
 * into the same columns as svx_bam.h, with the bases taken from the assembly FASTA the alignment was made from.
 *
 * `minimap2 -a` copies every contig's bases into its SAM (gigabytes per haplotype); the PAF of the same run carries all the
 * caller uses — target, position, strand, query span, MAPQ, CIGAR, NM — in megabytes, and the bases are a file the user
 * already has.  This reader is a third front end beside svx_bam.h and svx_sam.h: lines and fields on the handle's threads,
 * records ordered in memory, CIGAR text turned into words by svx_cigar_text_parse_dev / svx_cigar_text_parse (svx_sam.h),
 * and `svx_paf_seq_slices` served from the query assembly through svx_fasta_fetch_oriented (svx_text.h).
 *
 * THE RECORD OF A ROW (this reader's definition): a row is presented as the record `minimap2 -a -Y` would have written
 * for it — soft clips, full-length SEQ.  minimap2 is not available where this was written, so the statement below — and
 * not "what minimap2 does" — is what the tests pin.  Columns 1..12 of a row are
 * qname qlen qstart qend strand tname tlen tstart tend matches block mapq, followed by TAG:TYPE:VALUE fields.
 *   names    column 1                              l_seq   qlen (column 2)
 *   tid      column 6 looked up in the dictionary given at open (the reference's .fai: a PAF names only the targets that
 *            have alignments)                       pos     tstart (column 8, 0-based)          mapq   column 12
 *   flag     0x10 when the strand is `-`; 0x100 when the row has `tp:A:S`; otherwise, among the rows of one query name that
 *            are not `tp:A:S` (tag absent, P, I, i), the first IN FILE ORDER is the primary (no further bit) and every later
 *            one has 0x800
 *   cigar    `clip5 S` + the operations of `cg:Z:` + `clip3 S`, clips of length 0 left out; `+` strand: clip5 = qstart,
 *            clip3 = qlen - qend; `-` strand: the two swapped.  As words `len << 4 | op`, written by the pinned device or by
 *            the handle's threads exactly as for SAM (svx_paf_set_device_parse): the reader gathers `<clip5>S`, the tag's
 *            value and `<clip3>S` back to back per record, so the clips take the same path as the rest.
 *   ref_len  Σ len over {M,D,N,=,X}; must equal tend - tstart (columns 9 - 8)
 *   aux      `NM` (as BAM aux C / S / I by value) when the row has `NM:i:`; then, for a row whose query has other rows that
 *            are not `tp:A:S`, `SA:Z:` (sa_off / sa_len) listing those rows in file order, each as
 *            `tname,tstart+1,strand,shortCIGAR,mapq,NM;` (NM 0 for a row without the tag).  shortCIGAR of a row: `clip5 S`,
 *            `m M` with m = min(qend - qstart, tend - tstart), then `(qend - qstart - m) I` or `(tend - tstart - m) D` when
 *            not 0, `clip3 S`; parts of length 0 left out.
 *   voffset  BYTE OFFSET of the line in the file.    blocks_inflated and blocks_spanned are 0.
 * A `tp:A:S` row without `cg:Z:` has no CIGAR words and ref_len 0.
 * ORDER after svx_paf_load: the one svx_sam.h defines — (tid, pos, reverse-strand flag, place in the file) — by the same
 * comparison.  Lines: as svx_sam.h (mapped file cut at line ends, `\r\n` accepted, empty lines skipped).
 *
 * Refused with SVX_E_INVALID and the 1-based line number in svx_paf_last_error: fewer than 12 columns; a number column that
 * is no number or out of range (qstart <= qend <= qlen < 2^31, tstart <= tend <= tlen, MAPQ <= 255); a strand that is not
 * `+` or `-`; a target the dictionary does not have, or has with a length other than column 7; a row that is not `tp:A:S`
 * and has no `cg:Z:` (the message names `minimap2 -c`); a CIGAR the parser rejects; a CIGAR whose query-consuming length
 * differs from qend - qstart or whose ref_len differs from tend - tstart; rows of one query name with different qlen.
 * svx_paf_open refuses an empty file, a file whose first non-empty line starts with `@` (a SAM) and a gzip-compressed one.
 *
 * All functions return SVX_OK (0) or a negative svx_status (svx.h).  A handle is used by one thread at a time.  Pointers
 * handed out stay valid until the next svx_paf_load on the handle or svx_paf_close.
 */
#ifndef SVX_PAF_H_
#define SVX_PAF_H_

#include <stddef.h>
#include <stdint.h>

#include "svx.h"
#include "svx_bam.h"
#include "svx_text.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svx_paf svx_paf;

/* Open `path` (memory-mapped).  names / lengths [n_ref]: the reference dictionary, in the order that numbers tid (the
 * columns 1 and 2 of the reference's .fai).  n_threads <= 0: one per hardware thread, at most 64. */
int svx_paf_open(const char* path, int32_t n_ref, const char* const* names, const int32_t* lengths, int n_threads, svx_paf** out,
                 char* err, size_t err_cap);
void svx_paf_close(svx_paf* paf);
const char* svx_paf_last_error(const svx_paf* paf);
/* text: one `@SQ\tSN:name\tLN:length` line per dictionary entry (no @HD line: nothing is claimed about a sort order) */
int svx_paf_header(const svx_paf* paf, const char** text, uint64_t* l_text, int32_t* n_ref);
int svx_paf_reference(const svx_paf* paf, int32_t tid, const char** name, int32_t* length);

/* As svx_sam_set_pinned_device / svx_sam_set_device_parse / svx_sam_parsed_on_device. */
int svx_paf_set_pinned_device(svx_paf* paf, int device);
int svx_paf_set_device_parse(svx_paf* paf, int on);
int svx_paf_parsed_on_device(const svx_paf* paf);

/* Index the rows on contigs tids[0..n_tids) (NULL: every row) in the ORDER defined above.  Flags and SA strings are always
 * those of the whole file: a row's supplementary partners on other contigs are listed, loaded or not. */
int svx_paf_load(svx_paf* paf, const int32_t* tids, int32_t n_tids);
int svx_paf_get_columns(const svx_paf* paf, svx_bam_columns* out);

/* The assembly the rows' bases come from: an open FASTA handle (plain or bgzip-compressed; it must outlive the slices) and
 * columns 1 and 2 of its .fai.  Checked when slices are first asked for after a load: SVX_E_INVALID with the line number
 * for a loaded row whose query name the assembly does not have, or has with a length other than qlen. */
int svx_paf_set_query(svx_paf* paf, const svx_fasta* query, int32_t n_seq, const char* const* names, const int64_t* lengths);

/* Bases [begin[i], end[i]) of record rec[i]'s SEQ at out + out_off[i], as svx_bam_seq_slices: in BAM orientation, clipped
 * to [0, l_seq], every byte through the mapping of a BAM round trip.  For a `+` row that is query[begin:end]; for a `-` row
 * the reverse complement of query[qlen - end : qlen - begin] (svx_fasta_fetch_oriented, BAM alphabet on). */
int svx_paf_seq_slices(svx_paf* paf, const uint32_t* rec, const uint32_t* begin, const uint32_t* end, uint32_t n,
                       const uint64_t* out_off, uint8_t* out);

/* As svx_bam_device_pool / svx_bam_device_pool_wait. */
int svx_paf_device_pool(svx_paf* paf, const uint32_t** d_cigar, uint64_t* n_ops, void** ready);
int svx_paf_device_pool_wait(svx_paf* paf, double* waited_us);

#ifdef __cplusplus
}
#endif
#endif /* SVX_PAF_H_ */
