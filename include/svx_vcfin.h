/*
 * svx_vcfin.h — read a VCF back: the deletions and insertions of one sample as columns, everything else counted.
 *
 * The reader is what svim-asm-compare stands on and the inverse of the VCF writer for DEL and INS.
 * Plain text is memory-mapped; a `.gz` has to be BGZF (bgzip): its members are inflated and CRC-checked on the handle's
 * threads and the joined text is read the same way.  A gzip file that is not BGZF is refused with a message that names
 * bgzip.  "\r\n" line ends are accepted, empty lines skipped.  The header — the lines that start with '#' in front of the
 * first data line — is kept verbatim; its last line has to be the #CHROM line.
 *
 * CLASSIFICATION.  Every data line falls into exactly one class; the first rule of this list that applies decides:
 *   filtered      with `passonly`: FILTER is neither PASS nor "."
 *   multiallelic  ALT contains ','
 *   DEL / INS / complex    REF and ALT are both strings over letters ("" and "." count as the empty string).  With p the
 *                 length of their longest common prefix (compared without regard to case):
 *                     DEL  when p == len(ALT) < len(REF): the interval [POS-1+p, POS-1+len(REF))
 *                     INS  when p == len(REF) < len(ALT): at POS-1+p, the bytes ALT[p:] in upper case
 *                     complex otherwise (REF == ALT and SNVs among them)
 *                 INFO END and SVLEN are ignored for these records.
 *   DEL           ALT is <DEL>: end = INFO END; start = END - |SVLEN| when INFO has SVLEN, else POS.  SVX_E_INVALID when
 *                 END is missing or not a number, or the interval is empty.
 *   unresolved    ALT is <INS>: no bytes to compare
 *   other         every other ALT (<INV>, <DUP...>, breakends in [ ] notation, "*", ...)
 * and then, for what would be a DEL or an INS:
 *   not_carried   the sample's GT carries no allele 1 (0/0, ./., 0/.)
 * GENOTYPE.  The first ':'-field of the chosen sample column (`sample` by name, the first one when NULL), split on
 * '/' and '|'; haplotype bit h (1 << h, h = 0, 1) is set where allele h is "1"; a one-allele GT "1" sets both.  A file
 * without FORMAT and sample columns: every record is carried and its genotype 0 (unknown).
 *
 * SVX_E_INVALID with "line N: ..." (1-based) for: fewer than 8 columns; a POS that is not a number >= 1; a CHROM that is
 * not among `names`; a POS, a deletion's end or an insertion's place beyond the contig's length; data in front of the
 * #CHROM line or no #CHROM line at all; and for a `sample` the #CHROM line does not have (or a line without that column).
 */
#ifndef SVX_VCFIN_H_
#define SVX_VCFIN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svx_vcfin svx_vcfin;

enum {
    SVX_VCFIN_DEL = 0,
    SVX_VCFIN_INS = 1,
    SVX_VCFIN_MULTIALLELIC = 2,
    SVX_VCFIN_COMPLEX = 3,
    SVX_VCFIN_UNRESOLVED = 4,
    SVX_VCFIN_OTHER = 5,
    SVX_VCFIN_NOT_CARRIED = 6,
    SVX_VCFIN_FILTERED = 7,
    SVX_VCFIN_N_CLASSES = 8
};

/* Everything points into the handle and lives as long as it.  Rows are the DEL and INS records in file order. */
typedef struct svx_vcfin_columns {
    uint64_t n;
    const uint8_t* type;      /* SVX_VCFIN_DEL / SVX_VCFIN_INS */
    const int32_t* contig;    /* index into the names given to svx_vcfin_open */
    const int64_t* start;     /* DEL: [start, end); INS: at start, end = start + inserted bytes */
    const int64_t* end;
    const uint8_t* gt;        /* haplotype bits 1 | 2; 0: unknown (no sample columns) */
    const uint64_t* seq_off;  /* INS: the inserted bytes are seqs[seq_off .. seq_off + seq_len), upper case */
    const uint32_t* seq_len;
    const uint8_t* seqs;
    uint64_t seq_bytes;
    const uint64_t* line_off; /* the record's line in `text`, without its line end */
    const uint32_t* line_len;
    const uint32_t* line_no;  /* 1-based */
    const uint64_t* id_off;   /* the ID column in `text` */
    const uint32_t* id_len;
    const char* text;         /* the file's text (inflated where it was BGZF) */
    uint64_t text_bytes;
    uint64_t header_bytes;    /* text[0 .. header_bytes): the header lines, verbatim with their line ends */
    uint64_t n_lines;         /* data lines */
    uint64_t counts[SVX_VCFIN_N_CLASSES];
} svx_vcfin_columns;

/* Reads the whole file.  names / lengths: the contig dictionary of the genome's .fai.  sample: the sample column by
 * name, NULL for the first.  n_threads <= 0: one per CPU, at most 64.  On failure *out is NULL and `err` holds the
 * message. */
int svx_vcfin_open(const char* path, int32_t n_ref, const char* const* names, const int64_t* lengths, const char* sample,
                   int passonly, int n_threads, svx_vcfin** out, char* err, size_t err_cap);
/* The same file as a list of SITES: the sample columns are not looked at, so no record is SVX_VCFIN_NOT_CARRIED and gt is
 * 0 in every row — a record whose genotype is 0/0 or ./. in every sample is a site like any other. */
int svx_vcfin_open_sites(const char* path, int32_t n_ref, const char* const* names, const int64_t* lengths, int passonly,
                         int n_threads, svx_vcfin** out, char* err, size_t err_cap);
int svx_vcfin_get_columns(const svx_vcfin* v, svx_vcfin_columns* out);
void svx_vcfin_close(svx_vcfin* v);

/*
 * THE SAME FILE AS A LIST OF EDITS (svx_vcfin_open_alleles, svx_vcfin_get_alleles): every sequence-resolved record of one
 * sample — SNVs, MNPs, small and large indels, replacements — as "these reference bytes become those bytes", which is what
 * svim-asm-small-compare replays.  File handling, header, line ends, the genotype rule and the refusals
 * are those of svx_vcfin_open; a record's REF may reach to the contig's end and no further.
 *
 * CLASSIFICATION.  Every data line falls into exactly one class; the first rule of this list that applies decides:
 *   filtered           with `passonly`: FILTER is neither PASS nor "."
 *   multiallelic       ALT contains ','
 *   symbolic_or_other  REF or ALT is not a string over letters ("" and "." count as the empty string): <DEL>, <INS>,
 *                      breakends, "*", ...
 *   no_change          REF and ALT are the same string without regard to case: the edit is empty
 *   not_carried        the sample's GT carries no allele 1
 *   row                everything else.  Both alleles in upper case, p the length of their longest common prefix and s the
 *                      length of the longest common suffix of what is left behind it (prefix first: the rule that makes a
 *                      deletion [POS-1+p, ..) and an insertion lie at POS-1+p above):
 *                          start = POS-1+p    ref_len = len(REF)-p-s    alt = ALT[p : len(ALT)-s]
 * `phased` is 1 when the GT's first separator is '|', when the GT has one allele, when both alleles are 1, and when the
 * file has no genotype for the record (no sample columns or a FORMAT that does not start with GT: gt is 0, unknown, and
 * the record counts as carried on both haplotypes); 0 otherwise (0/1, ./1).
 */
enum {
    SVX_VCFIN_A_ROW = 0,
    SVX_VCFIN_A_MULTIALLELIC = 1,
    SVX_VCFIN_A_SYMBOLIC_OR_OTHER = 2,
    SVX_VCFIN_A_NOT_CARRIED = 3,
    SVX_VCFIN_A_FILTERED = 4,
    SVX_VCFIN_A_NO_CHANGE = 5,
    SVX_VCFIN_A_N_CLASSES = 6
};

/* Everything points into the handle and lives as long as it.  Rows are in file order. */
typedef struct svx_vcfin_alleles {
    uint64_t n;
    const int32_t* contig;        /* index into the names given to svx_vcfin_open_alleles */
    const int64_t* start;         /* the reference bytes [start, start + ref_len) become alts[alt_off .. alt_off + alt_len) */
    const uint32_t* ref_len;
    const uint64_t* alt_off;
    const uint32_t* alt_len;
    const uint8_t* alts;          /* upper case */
    uint64_t alt_bytes;
    const int64_t* pos;           /* POS - 1: where the REF column as written begins on the contig */
    const uint64_t* ref_off;      /* the REF column as written, in `text` ("." has length 0) */
    const uint32_t* ref_text_len;
    const uint8_t* gt;            /* haplotype bits 1 | 2; 0: unknown — the record is CARRIED ON BOTH haplotypes (phased is 1):
                                   * a caller that deals records out by bit has to read 0 as 3, as svim-asm-small-compare does */
    const uint8_t* phased;
    const uint64_t* line_off;     /* as in svx_vcfin_columns */
    const uint32_t* line_len;
    const uint32_t* line_no;
    const uint64_t* id_off;
    const uint32_t* id_len;
    const char* text;
    uint64_t text_bytes;
    uint64_t header_bytes;
    uint64_t n_lines;
    uint64_t counts[SVX_VCFIN_A_N_CLASSES];
} svx_vcfin_alleles;

int svx_vcfin_open_alleles(const char* path, int32_t n_ref, const char* const* names, const int64_t* lengths, const char* sample,
                           int passonly, int n_threads, svx_vcfin** out, char* err, size_t err_cap);
/* SVX_E_INVALID for a handle that svx_vcfin_open_alleles did not make (and svx_vcfin_get_columns for one that it made). */
int svx_vcfin_get_alleles(const svx_vcfin* v, svx_vcfin_alleles* out);

#ifdef __cplusplus
}
#endif
#endif /* SVX_VCFIN_H_ */
