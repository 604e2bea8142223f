/*
 * svx_text.h — C-ABI of the native text side of libsvx.so: indexed-FASTA access and the VCF body
 * (SURVEY.md §8 f-3).  Host code (C++), no device work: the reference does this part through
 * pysam.FastaFile (svim-asm:124; SVIM_COMBINE.py:45-99,467; SVCandidate.py:57-58,105,155,210,301-302)
 * and one Python format call per record (SVCandidate.py get_vcf_entry*, SVIM_COMBINE.py:428-477); at human
 * scale that is 10^5 fetch() calls and 10^5 str.format() calls — here each is one batch call over columns.
 *
 * All functions return SVX_OK (0) or a negative svx_status (svx.h); nothing throws or aborts.
 */
#ifndef SVX_TEXT_H_
#define SVX_TEXT_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ FASTA ---- */
typedef struct svx_fasta svx_fasta;

/* Map `path` read-only.  The caller has parsed `<path>.fai` (five columns: name, length, offset of the first
 * base, bases per line, bytes per line) and passes columns 2-5 for the n_refs sequences.  On failure *out is
 * NULL and a message is copied into err[err_cap] when err != NULL. */
int svx_fasta_open(const char* path, int32_t n_refs, const int64_t* length, const int64_t* offset,
                   const int32_t* line_bases, const int32_t* line_width, svx_fasta** out, char* err, size_t err_cap);
void svx_fasta_close(svx_fasta* fa);

/*
 * pysam.FastaFile.fetch(reference, start, end) for n intervals at once: the bases of sequence ref[i] in
 * [start[i], min(end[i], length)) — line ends skipped — at out + out_off[i]; `upper` != 0 applies ASCII
 * str.upper() on the way (the reference upper-cases every slice it fetches, SVIM_COMBINE.py:45-99,
 * SVCandidate.py:57-58,105,155,210,301-302).  out_off[n + 1] must hold exactly the clipped lengths back to
 * back (the caller knows them from the .fai lengths).  start < 0, end < start or a sequence that is shorter on
 * disk than its index entry says: SVX_E_INVALID.  Intervals are spread over n_threads host threads (<= 0:
 * one per hardware thread, at most 16).
 */
int svx_fasta_fetch_batch(const svx_fasta* fa, const int32_t* ref, const int64_t* start, const int64_t* end,
                          uint32_t n, int upper, const uint64_t* out_off, uint8_t* out, int n_threads);

/*
 * svx_fasta_fetch_batch with a direction per window and, when asked, the alphabet of a BAM record's SEQ: window i holds
 * bases [start[i], min(end[i], length)) of sequence ref[i]; with reverse[i] != 0 (reverse == NULL: none) they are written
 * as their REVERSE COMPLEMENT — output base k is the complement of source base end - 1 - k.  Complement: A<->T, C<->G,
 * M<->K, R<->Y, V<->B, H<->D, in upper and in lower case; S, W, N, `=` and every other byte stay.  Then, with bam_alphabet
 * != 0, every byte (of a reversed window or not) goes through the mapping of a BAM round trip — 4-bit code and back: lower
 * case -> upper, anything outside =ACMGRSVTWYHKDBN -> N — as svx_bam_seq_slices and svx_sam_seq_slices write it; with
 * bam_alphabet == 0 bytes keep their case.  This is how a query assembly serves the SEQ of an alignment that names only a
 * span and a strand (svx_paf.h).  Same arguments, checks and back ends as svx_fasta_fetch_batch: a plain file on the host
 * threads, a bgzip-compressed one on the threads or on the device (svx_fasta_set_device) — the same bytes either way.
 */
int svx_fasta_fetch_oriented(const svx_fasta* fa, const int32_t* ref, const int64_t* start, const int64_t* end,
                             const uint8_t* reverse, uint32_t n, int bam_alphabet, const uint64_t* out_off, uint8_t* out,
                             int n_threads);

/*
 * A bgzip-compressed FASTA (htslib faidx semantics): the .fai columns count UNCOMPRESSED bytes, and
 * gzi_coff / gzi_uoff[n_gzi] are the `<path>.gzi` pairs (compressed offset of a member, uncompressed offset of its
 * first byte; (0, 0) implicit, a final entry at the end of the data allowed).  At open the whole member chain is
 * walked (header, BSIZE, ISIZE): every .gzi entry must lie on a member header with the uncompressed offset the chain
 * gives, the offsets must increase, and the chain must end exactly at the end of the file.  svx_fasta_fetch_batch
 * then inflates every member under its windows once (the build's own decoder, CRC32 and ISIZE checked as htslib's
 * BGZF reader does) on the handle's threads, or on the device (svx_fasta_set_device), and gathers the bases as for a
 * plain file.  A damaged member under a window: SVX_E_INVALID, svx_fasta_last_error names its compressed offset.
 */
int svx_fasta_open_bgzf(const char* path, int32_t n_refs, const int64_t* length, const int64_t* offset,
                        const int32_t* line_bases, const int32_t* line_width, const uint64_t* gzi_coff,
                        const uint64_t* gzi_uoff, uint64_t n_gzi, svx_fasta** out, char* err, size_t err_cap);
/* 1 for a handle of svx_fasta_open_bgzf, 0 otherwise */
int svx_fasta_is_bgzf(const svx_fasta* fa);
/* device >= 0: batch calls that touch at least min_members distinct members inflate the members that are not resident
 * yet on that device (svx_bgzf_inflate_on_stream) and gather the windows there; the inflated members stay resident
 * (up to 6 GiB) until svx_fasta_close.  device < 0: host threads only (the default).  Where no device can be brought
 * up the call runs on the host threads and writes the same bytes.  No effect on a plain file. */
int svx_fasta_set_device(svx_fasta* fa, int device, uint32_t min_members);
/* counters of a compressed handle (all 0 for a plain one): out[SVX_FASTA_STATS] = members inflated on the host, on
 * the device, compressed bytes staged for the device, member look-ups served from the host cache or the device arena,
 * device calls, host calls */
#define SVX_FASTA_STATS 6
int svx_fasta_stats(const svx_fasta* fa, uint64_t* out);
/* the last error of a failed fetch ("" when none) */
const char* svx_fasta_last_error(const svx_fasta* fa);

/* -------------------------------------------------------------------- VCF ---- */
/*
 * The record lines of write_final_vcf (SVIM_COMBINE.py:428-477): one call formats every entry, sorts them the
 * way sorted_nicely does (:369-376 — natural order of the contig names, then start, then end; stable) and
 * numbers the IDs per SV type label in sorted order (:470-475).
 *
 * Entries arrive in the reference's LIST order (:431-464: deletions, inversions, insertions, tandem
 * duplications, interspersed duplications, then two entries per breakend).  Entry e describes candidate row
 * row[e] of the candidate columns in the way kind[e] says:
 */
#define SVX_VCF_DEL 0          /* CandidateDeletion.get_vcf_entry              SVCandidate.py:53-78    */
#define SVX_VCF_INV 1          /* CandidateInversion.get_vcf_entry             :99-125                 */
#define SVX_VCF_INS 2          /* CandidateInsertion.get_vcf_entry             :151-176                */
#define SVX_VCF_DUPTAN_INS 3   /* CandidateDuplicationTandem.get_vcf_entry_as_ins  :203-232            */
#define SVX_VCF_DUPTAN_DUP 4   /*   ... get_vcf_entry_as_dup                   :234-261                */
#define SVX_VCF_DUPINT_INS 5   /* CandidateDuplicationInterspersed.get_vcf_entry_as_ins  :296-321      */
#define SVX_VCF_DUPINT_DUP 6   /*   ... get_vcf_entry_as_dup                   :323-347                */
#define SVX_VCF_BND 7          /* CandidateBreakend.get_vcf_entry              :389-415                */
#define SVX_VCF_BND_REV 8      /*   ... get_vcf_entry_reverse                  :417-443                */

typedef struct svx_vcf_in {
    /* ---- candidate columns (n_rows rows; svim_asm_amd/table.py) */
    uint32_t n_rows;
    const int32_t* sc;        /* source contig id  */
    const int64_t* ss;        /* source start      */
    const int64_t* se;        /* source end        */
    const int32_t* dc;        /* destination contig id */
    const int64_t* ds;
    const int64_t* de;
    const uint8_t* flag;      /* bit 0 complete / fully_covered / cutpaste; bit 1 source 'rev', bit 2 dest 'rev' */
    const int64_t* copies;
    const uint8_t* gt;        /* index into genotypes */
    const int64_t* q_off;     /* inserted sequence = seqs[q_off .. q_off + q_len) */
    const int64_t* q_len;
    const int64_t* r_off;     /* n_rows + 1: reads of row i = read names r_flat[r_off[i] .. r_off[i+1]) */
    const int64_t* r_flat;
    /* ---- stores (the sizes bound every offset above and below: a slice that leaves its pool is SVX_E_INVALID) */
    const uint8_t* seqs;
    uint64_t seqs_bytes;
    const char* names;        /* read-name pool (only read when read_names != 0) */
    const int64_t* name_off;  /* n_names + 1 */
    uint64_t n_names;
    const char* contigs;      /* contig-name pool */
    const int64_t* contig_off; /* n_contigs + 1 */
    const int32_t* contig_rank; /* rank of every contig name under sorted_nicely's natural key (equal keys share one) */
    uint32_t n_contigs;
    const char* genotypes;    /* genotype strings, pool + offsets */
    const int64_t* genotype_off;
    uint32_t n_genotypes;
    /* ---- entries (n_entries; list order) */
    uint32_t n_entries;
    const uint8_t* kind;
    const uint32_t* row;
    /* reference bases of entry e (sequence alleles only; already upper-cased by svx_fasta_fetch_batch):
     * bases[b_off[e] .. b_off[e] + b_len[e]) = the REF allele the entry's formatter fetches; for
     * SVX_VCF_DUPINT_INS a second slice bases[b2_off[e] ...) = the source interval appended to ALT */
    const uint8_t* bases;
    uint64_t bases_bytes;
    const int64_t* b_off;
    const int64_t* b_len;
    const int64_t* b2_off;
    const int64_t* b2_len;
    int sequence_alleles;     /* not options.symbolic_alleles */
    int read_names;           /* options.query_names */
    /* ---- a cohort's merged records (optional; all NULL / 0 for a single sample's file).  Per candidate ROW:
     * sample_text[sample_off[r] .. sample_off[r + 1]) replaces the genotype behind "GT\t" — the tab-joined genotypes
     * of the S samples —, FORMAT is "GT" for every kind (no CN); info_text[info_off[r] .. info_off[r + 1]) is appended
     * to INFO as it is (";NS=..;AC=..;AN=..").  Either may be given without the other. */
    const char* sample_text;
    const int64_t* sample_off;  /* n_rows + 1 */
    uint64_t sample_bytes;
    const char* info_text;
    const int64_t* info_off;    /* n_rows + 1 */
    uint64_t info_bytes;
} svx_vcf_in;

/* Formats into a buffer owned by the library: *text / *n_bytes (every line ends with '\n'); free with
 * svx_vcf_free.  n_lines receives the number of record lines. */
int svx_vcf_format(const svx_vcf_in* in, char** text, uint64_t* n_bytes, uint64_t* n_lines);
void svx_vcf_free(char* text);
/* The same lines written to the file descriptor `fd` behind its current position (where the caller's header lines
 * end; a regular file opened for writing, NOT in append mode): every formatting thread writes its own stretch with
 * pwrite at its final place — no joined buffer, the copies into the page cache run side by side.  The position of
 * `fd` is left behind the last line.  n_bytes receives the bytes written. */
int svx_vcf_write(const svx_vcf_in* in, int fd, uint64_t* n_bytes, uint64_t* n_lines);
/* The same lines into one buffer of the library's behind a copy of prefix[n_prefix] (the header lines): *text holds
 * n_prefix + *n_bytes bytes; free with svx_vcf_free. */
int svx_vcf_format_after(const svx_vcf_in* in, const char* prefix, uint64_t n_prefix, char** text, uint64_t* n_bytes,
                         uint64_t* n_lines);

/* ------------------------------------------------------------------ tabix ---- */
/*
 * The tabix index (VCF preset: sequence column 1, begin 2, end from REF and INFO/END, meta '#') of `text` compressed
 * into BGZF members of 65 280 input bytes each whose sizes are member_len[n_members] (svx_bgzf_compress's).  The
 * index's uncompressed bytes (BGZF-compress them to write the file) in *index, freed with svx_vcf_free; *kind = 1 for
 * a .tbi (min_shift 14, 5 levels), 2 for a .csi (min_shift 14, depth 6) when a record ends beyond 2^29, 0 when the
 * records cannot be indexed — a contig's records not contiguous, or positions that decrease within one: *index stays
 * NULL and err names the first such record.  Names are listed in order of first appearance; the pseudo-bin carries
 * the first / last offsets and the record counts.  Malformed lines: SVX_E_INVALID with err set.
 */
int svx_tabix_build(const uint8_t* text, uint64_t n, const uint32_t* member_len, uint64_t n_members, uint8_t** index,
                    uint64_t* index_len, int* kind, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* SVX_TEXT_H_ */
