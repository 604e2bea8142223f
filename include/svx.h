/*
 * svx.h — C-ABI of libsvx.so: the MI355X (gfx950) hot path of SVIM-asm.
 *
 * The reference (eldariont/svim-asm v1.0.3) is pure Python and has no FFI layer;
 * the boundary a maintainer would bind is the set of Python function seams listed
 * in SURVEY.md §8(b).  Each entry point below names the reference function
 * (file:line under /root/reference/src/svim_asm) whose arithmetic it replaces.
 * INTEGRATION.md shows the ctypes stub that binds them from the reference side.
 *
 * Conventions
 *   - every function returns int: SVX_OK (0) or a negative svx_status; nothing
 *     throws, aborts or keeps hidden global state;
 *   - a context (svx_ctx) = one device + one HIP stream + a growable HBM
 *     workspace.  One thread uses a context at a time; contexts are independent
 *     (8 contexts for the 8 GPUs of a node);
 *   - functions without a suffix take HOST pointers (the library stages them to
 *     HBM, runs the kernels and copies the results back, then synchronises);
 *     functions ending in _dev take DEVICE pointers, enqueue on the context's
 *     stream and do not synchronise (the caller owns the buffers, e.g. torch
 *     tensors, and synchronises the stream it handed in);
 *   - all outputs are written in the reference's deterministic order (prefix-sum
 *     compaction and stable sorts; no atomically-ordered appends).
 *   - there is NO CPU fallback inside this library: without a usable HIP device
 *     svx_ctx_create fails with SVX_E_NODEVICE.
 */
#ifndef SVX_H_
#define SVX_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svx_ctx svx_ctx;

typedef enum svx_status {
    SVX_OK = 0,
    SVX_E_INVALID = -1,   /* bad argument (null pointer, non-monotone offsets, ...) */
    SVX_E_CAPACITY = -2,  /* output buffer too small; *n_out holds the needed count */
    SVX_E_HIP = -3,       /* a HIP runtime call failed; see svx_last_error          */
    SVX_E_NOMEM = -4,     /* HBM / host allocation failed                           */
    SVX_E_TOO_LARGE = -5, /* batch exceeds a documented limit (e.g. >= 2^32 ops)    */
    SVX_E_NODEVICE = -6   /* no HIP device / device index out of range              */
} svx_status;

/* ---------------------------------------------------------------- context -- */

/* Create a context on HIP device `device` with its own non-blocking stream. */
int svx_ctx_create(int device, svx_ctx** out);
/* Same, but enqueue on a caller-owned hipStream_t (e.g. torch's current stream:
 * torch.cuda.current_stream().cuda_stream).  Pass NULL for the default stream. */
int svx_ctx_create_on_stream(int device, void* hip_stream, svx_ctx** out);
void svx_ctx_destroy(svx_ctx* ctx);
/* Block until everything enqueued on the context's stream has finished. */
int svx_ctx_sync(svx_ctx* ctx);
/* Last error text for this context (never NULL; "" when no error). */
const char* svx_last_error(const svx_ctx* ctx);
const char* svx_version(void);
/* Number of visible HIP devices (0 when none / no driver). Never fails. */
int svx_device_count(void);
/* PCI address of a visible device as "domain:bus:device.function" (hipDeviceGetPCIBusId): what a host process needs to
 * find the device's NUMA node (/sys/bus/pci/devices/<address>/numa_node) and keep its threads there — one worker
 * process per GPU of a node (svim-asm-cohort --device k).  `len` >= 16. */
int svx_device_pci_bus_id(int device, char* out, int len);

/* THE SCRATCH CONTRACT.  Every entry point that takes a context carves its scratch out of two long-lived HBM regions
 * of that context (a workspace and a staging region; svx_collect_batch also a page-locked host block).  A region is
 * reallocated only when a call needs more than it has, and nothing outside the first 4 KiB of the workspace (a header
 * of counters that the kernels using them leave as they found them, see DESIGN.md "Scratch contract") is ever cleared:
 * THE CONTENTS OF CONTEXT SCRATCH BETWEEN CALLS ARE UNSPECIFIED.  A call sees what the previous call — of any entry
 * point, of any size — left there, and must write every scratch word before it reads it.
 *
 * The two entries below are a TEST FACILITY for that contract; no product path calls them and neither launches a
 * kernel.  svx_ctx_scratch_fill waits for the context's stream, sets every byte of the workspace behind the header,
 * every byte of the staging region and every byte of the host block to `byte` (low 8 bits; hipMemset / memset), and
 * waits again.  A region that is not allocated yet is skipped; the header, a pending check of a wait between
 * workgroups and everything the caller owns stay as they are.  svx_ctx_scratch_header waits for the stream and copies
 * the 1024 words of the header to `out` (zeros while there is no workspace). */
int svx_ctx_scratch_fill(svx_ctx* ctx, int byte);
int svx_ctx_scratch_header(svx_ctx* ctx, uint32_t out[1024]);

/* svx_cigar_extract* run batches of at most `max_ops` CIGAR ops in TWO kernel launches (tiles of 1024
 * ops; every workgroup of the second kernel scans all tile descriptors itself): the operating point of
 * the svim-asm CLI — one BAM of an assembly (~1.5 M ops) or both haplotype BAMs of a diploid sample
 * (~6 M ops) per call —, where five dependent launches cost more than the work.  Larger batches take the
 * streaming path (tiles of 4096 ops, five launches).  Default and upper limit 2^23 ops; 0 disables the
 * small-batch path; larger values are clamped to 2^23.  Results are identical on both. */
int svx_ctx_set_small_batch_ops(svx_ctx* ctx, uint64_t max_ops);
/* svx_collect_batch* send the split-segment chain of a submission (segment rows -> decision tree -> post-passes,
 * SVIM_inter.py:62-340) out INSIDE the launches of the CIGAR path: rows and decision tree among the workgroups of the
 * tile launch (two-launch path) or of the finish launch (streaming path), the post-passes among the workgroups of
 * the path's last launch.  on != 0 restores the single-purpose launches (svx_segments_rows_dev,
 * svx_segments_classify_dev, svx_segments_postpass_dev behind svx_cigar_extract_dev) — same results; kept for
 * comparison and for submissions whose reads are too uneven for one scratch slice size, which take it by
 * themselves.  Default off. */
int svx_ctx_set_split_chain(svx_ctx* ctx, int on);
/* svx_pair_partition* sort batches of at most `max_candidates` keys in ONE kernel launch (buckets by the
 * leading key bits, every window of buckets sorted inside one workgroup's LDS — merged when the window
 * arrives as a few sorted runs, as PAIR's two haplotype lists do, counted otherwise —, two arrival barriers
 * inside the launch): the PAIR step of one diploid sample is 60-90 k candidates.  Larger batches take the
 * radix path (P + 2 launches).  Default and upper limit 131072; 0 disables the one-launch path.  Results
 * are identical on both.  The launch holds at most min(64, CUs / 4) workgroups, all resident: up to four
 * contexts may run it on one device at the same time.  Should its workgroups (or those of the radix path's
 * partition sweep) ever wait for each other longer than 20 s, they give up: svx_pair_partition re-runs the call on
 * the wait-free plan (below) and succeeds; for the asynchronous entry points the next svx_ctx_sync returns
 * SVX_E_HIP, the outputs of that call are invalid, the context stays usable. */
int svx_ctx_set_pair_single_launch_max(svx_ctx* ctx, uint32_t max_candidates);
/* For callers of the asynchronous svx_pair_partition_dev*: 1 when the SVX_E_HIP that the latest svx_ctx_sync (or a
 * later call on the context) returned was a wait between workgroups that ran out — the outputs of that call are
 * invalid, the context is usable, and the same call enqueued again after svx_ctx_set_pair_wait_free(ctx, 1) cannot
 * fail that way (what svx_pair_partition does by itself for host-pointer callers).  Reading clears the flag. */
int svx_ctx_barrier_timed_out(svx_ctx* ctx);
/* The plan that never waits between workgroups inside a launch: radix passes (P + 1 launches) and the partition
 * sweep as two launches.  Slower than the plans above and independent of who else is resident on the device.
 * svx_pair_partition (host pointers, synchronous) falls back to it by itself when a wait of the faster plans
 * runs out — the call then succeeds, svx_ctx_pair_retries counts such calls —; callers of the asynchronous *_dev
 * entry points, which cannot be re-run behind their back, may select it up front.  Results are identical. */
int svx_ctx_set_pair_wait_free(svx_ctx* ctx, int enabled);
int svx_ctx_pair_retries(const svx_ctx* ctx);

/* Device buffers for callers that have no other owner of HBM (a ctypes binding without torch, the
 * tests): plain hipMalloc / hipFree / hipMemcpyAsync on the context's device and stream.
 * svx_dev_upload and svx_dev_download are ordered on the context's stream with the kernels of the
 * *_dev entry points; svx_dev_download synchronises the stream before it returns. */
int svx_dev_malloc(svx_ctx* ctx, size_t bytes, void** d_out);
int svx_dev_free(svx_ctx* ctx, void* d_ptr);
int svx_dev_upload(svx_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int svx_dev_download(svx_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* Kernel timing with HIP events on the context's stream.  When enabled, every
 * *_dev entry point brackets its kernels with events; after svx_ctx_sync the
 * elapsed GPU time of the last call is returned in milliseconds. */
int svx_ctx_set_timing(svx_ctx* ctx, int enabled);
int svx_ctx_last_kernel_ms(svx_ctx* ctx, float* ms_total, float* ms_dominant);
/* Measurement aid: the read-only streaming rate this device sustains right now — `reps` passes of a kernel that
 * reads d_buf[0 .. bytes) once per pass with the loads of the CIGAR stream (16 bytes per lane, four in flight,
 * nontemporal) and writes nothing; *ms_per_pass = HIP-event time / reps.  bytes / that time is the second
 * denominator a read-mostly kernel's achieved GB/s is quoted against (a device-to-device copy is not a
 * ceiling for such a kernel).  Synchronises the stream.  d_buf 16-byte aligned. */
int svx_hbm_read_probe_dev(svx_ctx* ctx, const void* d_buf, size_t bytes, uint32_t reps, float* ms_per_pass);

/* Pipelining independent batches over two contexts: make everything enqueued on `ctx` from now on
 * wait until the streaming (dominant) kernel of `other`'s most recent svx_cigar_extract*_dev call
 * has finished — the scan/finish tail of that call may still overlap.  The first call only arms
 * `other` (it starts recording an event after its streaming kernel); no-op until one was recorded.
 * Both contexts must live on the same device. */
int svx_ctx_wait_dominant(svx_ctx* ctx, svx_ctx* other);

/* ------------------------------------------------------------ a1 + a2 ------ */
/*
 * CIGAR walk → indel signatures.
 * Replaces analyze_cigar_indel (SVIM_intra.py:8-30) over a whole batch of
 * alignments, fused with the `ref_start + pos_ref` of analyze_alignment_indel
 * (SVIM_intra.py:36-43).  The batch boundary is the per-contig loop of
 * analyze_alignment_file_coordsorted (SVIM_COLLECT.py:61-83).
 *
 *   cigar      BAM-native packed ops, `len << 4 | op`, all alignments back to back
 *              (pysam cigartuples (op,len) == (w & 15, w >> 4)); n_ops = aln_off[n_aln]
 *   aln_off    n_aln + 1 non-decreasing offsets into `cigar` (empty alignments allowed)
 *   ref_start  per-alignment reference_start added to pos_ref, or NULL for the
 *              raw analyze_cigar_indel result (pos_ref relative to the alignment)
 *   min_len    options.min_sv_size; an I/D op emits when len >= min_len
 *
 * Output (SoA, 17 B per signature, in (alignment, op) order):
 *   aln        index of the alignment the op belongs to
 *   ref_pos    ref_start[aln] + running reference offset BEFORE the op
 *   read_pos   running query offset BEFORE the op (counts leading soft clips)
 *   len        op length
 *   type       SVX_SIG_INS (op 1) or SVX_SIG_DEL (op 2)
 *
 * Ops 0(M),7(=),8(X) advance both cursors, 1(I),4(S) the query, 2(D) the
 * reference; 3(N),5(H),6(P),9(B) and codes 10-15 advance nothing
 * (SVIM_intra.py:14-29 has no branch for them).
 *
 * If more than `cap` signatures exist, nothing beyond `cap` is written, *n_out
 * receives the exact count and SVX_E_CAPACITY is returned.
 * Limits: n_ops < 2^32 per call; per-alignment cursor sums < 2^32.
 */
#define SVX_SIG_INS 0
#define SVX_SIG_DEL 1

typedef struct svx_sig_soa {
    uint32_t* aln;
    uint32_t* ref_pos;
    uint32_t* read_pos;
    uint32_t* len;
    uint8_t* type;
} svx_sig_soa;

int svx_cigar_extract(svx_ctx* ctx, const uint32_t* cigar, const uint64_t* aln_off,
                      uint32_t n_aln, const int32_t* ref_start, uint32_t min_len,
                      svx_sig_soa out, uint64_t cap, uint64_t* n_out);

/* SoA input variant named by the north star: op codes and lengths in two arrays
 * (pysam cigartuples flattened as u8 op[], u32 len[]). Same output contract.
 * The PACKED layout above is the fast one: it is what a BAM record holds (no conversion on ingest) and
 * it moves 4 B per op instead of 5.  Both kernels stream at the same HBM rate (≈ 6 TB/s on MI355X:
 * 331 µs for the 1.98 GB of a 395 M-op SoA batch, 265 µs for the 1.58 GB of the same batch packed), so
 * in ops/s — and in the 4 B/op the roofline credits — SoA runs at 4/5 of packed (0.62 vs 0.78 of
 * peak).  Callers that hold packed words should pass them as they are. */
int svx_cigar_extract_soa(svx_ctx* ctx, const uint8_t* op, const uint32_t* len,
                          const uint64_t* aln_off, uint32_t n_aln, const int32_t* ref_start,
                          uint32_t min_len, svx_sig_soa out, uint64_t cap, uint64_t* n_out);

/* Device-pointer variants.  PRECONDITION (not checked: the offsets live in HBM and nothing is read
 * back): d_aln_off[0] == 0, non-decreasing, d_aln_off[n_aln] == n_ops — the host-pointer entry points
 * validate exactly this and return SVX_E_INVALID; with offsets that violate it the behaviour is
 * undefined (alignment indices derived from them index d_ref_start).  A caller that cannot vouch
 * for its offsets should validate them before the upload, as svx_cigar_extract does.
 * n_ops must equal aln_off[n_aln] (the caller knows it;
 * the device copy is not read back).  d_cigar / d_len / d_op must be 16-byte aligned;
 * d_op is fetched as dwords, i.e. it must be readable up to the next multiple of 4 bytes
 * after n_ops (any hipMalloc'ed buffer is); the extra bytes are ignored.  d_n_out: one uint64 in device memory.
 * Exactly min(count, cap) signatures are written. Asynchronous on the ctx stream. */
int svx_cigar_extract_dev(svx_ctx* ctx, const uint32_t* d_cigar, uint64_t n_ops,
                          const uint64_t* d_aln_off, uint32_t n_aln, const int32_t* d_ref_start,
                          uint32_t min_len, svx_sig_soa d_out, uint64_t cap, uint64_t* d_n_out);
int svx_cigar_extract_soa_dev(svx_ctx* ctx, const uint8_t* d_op, const uint32_t* d_len,
                              uint64_t n_ops, const uint64_t* d_aln_off, uint32_t n_aln,
                              const int32_t* d_ref_start, uint32_t min_len, svx_sig_soa d_out,
                              uint64_t cap, uint64_t* d_n_out);

/* Per-alignment CIGAR statistics in the same pass family (pysam/htslib
 * definitions used by SVIM_inter.py:68-79 and SVIM_COLLECT.py:11):
 *   ref_len    Σ len over {M,D,N,=,X}   (reference_end - reference_start, htslib bam_endpos)
 *   q_start    Σ leading S ops (skipping H)        = query_alignment_start
 *   q_end      q_start + Σ len over {M,I,=,X}      = query_alignment_end
 *   read_len   Σ len over {M,I,S,=,X,H}            = infer_read_length()
 *   n_hard     Σ len over H                        = get_cigar_stats()[0][5]
 * Each output array has n_aln entries (any may be NULL to skip). Host pointers. */
typedef struct svx_aln_stats {
    uint32_t* ref_len;
    uint32_t* q_start;
    uint32_t* q_end;
    uint32_t* read_len;
    uint32_t* n_hard;
} svx_aln_stats;

int svx_cigar_stats(svx_ctx* ctx, const uint32_t* cigar, const uint64_t* aln_off, uint32_t n_aln,
                    svx_aln_stats out);
int svx_cigar_stats_dev(svx_ctx* ctx, const uint32_t* d_cigar, uint64_t n_ops,
                        const uint64_t* d_aln_off, uint32_t n_aln, svx_aln_stats d_out);

/* ---------------------------------------------------------------- a3 ------- */
/*
 * Split-segment classification: the adjacent-pair decision tree of
 * analyze_read_segments (SVIM_inter.py:62-258) for a batch of reads.
 *
 * For read r the caller passes its 1 + k segments in the reference's order
 * ([primary] + supplementaries, SVIM_inter.py:64) at segs[read_off[r] ..
 * read_off[r+1]).  q_start/q_end are the values of SVIM_inter.py:68-73 (already
 * flipped for reverse-strand records).  The kernel sorts each read's segments
 * stably by (q_start, q_end) (SVIM_inter.py:83) and classifies each adjacent
 * pair; out[read_off[r] + i] describes sorted pair (i, i+1); the last slot of
 * each read is SVX_RAW_NONE.  read_len[r] = primary.infer_read_length()
 * (SVIM_inter.py:120).
 *
 * Raw records (a0..a5):
 *   SVX_RAW_INS    ref_id, start, end, seq_start, seq_len  (slice of primary.query_sequence)
 *   SVX_RAW_DEL    ref_id, start, end
 *   SVX_RAW_BND    ref_id1, pos1, dir1, ref_id2, pos2, dir2   (dir: 0 'fwd', 1 'rev');
 *                  every BND is also a `translocations` tuple (SVIM_inter.py:136...)
 *   SVX_RAW_TANDEM ref_id, start, end, fully_covered, direction_fwd   (:150-164)
 *   SVX_RAW_INV    ref_id, start, end, side  (0 left_fwd, 1 left_rev, 2 right_fwd, 3 right_rev)
 * The post-passes (tandem merge :261-290, interspersed duplications :293-320,
 * inversion clustering :323-338) consume these records on the host.
 */
#define SVX_RAW_NONE 0
#define SVX_RAW_INS 1
#define SVX_RAW_DEL 2
#define SVX_RAW_BND 3
#define SVX_RAW_TANDEM 4
#define SVX_RAW_INV 5

typedef struct svx_seg {
    int32_t q_start, q_end, ref_id, ref_start, ref_end, is_reverse;
} svx_seg;

typedef struct svx_seg_params {
    int32_t min_sv_size;
    int32_t max_sv_size;
    int32_t query_gap_tolerance;
    int32_t query_overlap_tolerance;
    int32_t reference_gap_tolerance;
    int32_t reference_overlap_tolerance;
} svx_seg_params;

typedef struct svx_raw {
    int32_t kind;
    int32_t a0, a1, a2, a3, a4, a5;
    int32_t pad;
} svx_raw;

int svx_segments_classify(svx_ctx* ctx, const svx_seg* segs, const uint32_t* read_off,
                          uint32_t n_reads, const int32_t* read_len, const svx_seg_params* params,
                          svx_raw* out);
/* _dev: d_segs 8-byte aligned, d_out 16-byte aligned (any hipMalloc'ed buffer is). */
int svx_segments_classify_dev(svx_ctx* ctx, const svx_seg* d_segs, uint32_t n_segs,
                              const uint32_t* d_read_off, uint32_t n_reads,
                              const int32_t* d_read_len, const svx_seg_params* params,
                              svx_raw* d_out);

/*
 * The three per-read post-passes of analyze_read_segments (SVIM_inter.py:260-338) over the raw records
 * of svx_segments_classify: tandem-duplication merge (:261-290), interspersed duplications from pairs of
 * breakends (:293-320), inversion sweep + complete-linkage clustering (:323-338, :42-60).  The INS / DEL /
 * BND records of `raw` ARE candidates already (one each, in slot order); this call adds the derived ones.
 *
 *   raw, read_off   as written by / passed to svx_segments_classify (slot i of read r = raw[read_off[r] + i])
 *   contig_rank     per reference id: rank of the contig NAME under Python str ordering — the inversion
 *                   sweep sorts by (name, start, end) (:323); ids >= n_contigs rank as themselves
 *   params          min_sv_size / max_sv_size bound the interspersed-duplication length (:309,:313)
 *   out, out_off    derived candidates of read r at out[out_off[r] .. out_off[r] + out_cnt[r]), in the
 *                   reference's order: tandem duplications, interspersed duplications, inversions;
 *                   out_off[r+1] - out_off[r] must be at least svx_segments_postpass_bound(slots of r)
 *                   (= s (s + 3) / 2: s tandems, s (s - 1) / 2 breakend pairs, s inversions), else
 *                   SVX_E_CAPACITY
 * Records (a0..a5):
 *   SVX_POST_TANDEM   ref_id, start, end, copies, fully_covered        (CandidateDuplicationTandem)
 *   SVX_POST_DUP_INT  src ref_id, src start, src end, dst ref_id, dst start, dst end
 *   SVX_POST_INV      ref_id, start, end, complete                       (CandidateInversion)
 */
#define SVX_POST_TANDEM 1
#define SVX_POST_DUP_INT 2
#define SVX_POST_INV 3

typedef struct svx_post {
    int32_t kind;
    int32_t a0, a1, a2, a3, a4, a5;
    int32_t pad;
} svx_post;

uint64_t svx_segments_postpass_bound(uint32_t n_slots);
int svx_segments_postpass(svx_ctx* ctx, const svx_raw* raw, const uint32_t* read_off, uint32_t n_reads,
                          const int32_t* contig_rank, uint32_t n_contigs, const svx_seg_params* params,
                          svx_post* out, const uint64_t* out_off, uint32_t* out_cnt);

/* Asynchronous form on device pointers.  The HOST copies `read_off` / `out_off` size the per-read scratch and
 * are validated exactly like above (nothing of them is read after the call returns); d_read_off / d_out_off are
 * the same arrays in HBM.  Enqueues on the context's stream, does not synchronise. */
int svx_segments_postpass_dev(svx_ctx* ctx, const svx_raw* d_raw, const uint32_t* read_off, const uint32_t* d_read_off,
                              uint32_t n_reads, const int32_t* d_contig_rank, uint32_t n_contigs,
                              const svx_seg_params* params, svx_post* d_out, const uint64_t* out_off,
                              const uint64_t* d_out_off, uint32_t* d_out_cnt);

/*
 * Segment rows of chimeric reads straight from CIGARs in HBM: the dictionaries analyze_read_segments builds per
 * alignment (SVIM_inter.py:66-81) — q_start / q_end from query_alignment_start / _end (flipped with
 * infer_read_length() for reverse records), reference_end = reference_start + Σ{M,D,N,=,X} (1 when that is 0,
 * htslib bam_endpos).  Segment j is alignment d_seg_src[j] of (d_cigar, d_aln_off); d_seg_qend[j] >= 0 overrides
 * query_alignment_end (pysam takes it from the stored sequence when the record has one: l_seq minus the trailing
 * soft clips), -1 derives it from the CIGAR.  d_read_len[r] = infer_read_length() of read r's first segment
 * (its primary, SVIM_inter.py:120).  One wave per segment; asynchronous.
 */
int svx_segments_rows_dev(svx_ctx* ctx, const uint32_t* d_cigar, const uint64_t* d_aln_off, const uint32_t* d_seg_src,
                          const int32_t* d_seg_tid, const int32_t* d_seg_pos, const uint8_t* d_seg_rev,
                          const int32_t* d_seg_qend, uint32_t n_segs, const uint32_t* d_read_off, uint32_t n_reads,
                          svx_seg* d_segs, int32_t* d_read_len);

/* ------------------------------------------------------- COLLECT, whole ---- */
/*
 * The device work of analyze_alignment_file_coordsorted (SVIM_COLLECT.py:61-83) for every record of a sample —
 * or of both haplotype BAMs of a diploid sample — as ONE submission: svx_cigar_extract_dev over all records
 * (a1 + a2), svx_segments_rows_dev + svx_segments_classify_dev + svx_segments_postpass_dev over the chimeric reads
 * (a3), enqueued on the context's stream behind the uploads; two read-backs (the counts, then exactly the results).
 *
 *   cigar_parts / part_ops   n_parts host arrays of BAM-native CIGAR words, logically back to back (the pools of
 *                 svx_bam_get_columns: page-locked, uploaded where they lie — no concatenation on the host)
 *   aln_off       n_aln + 1 offsets into that concatenation, EVERY record of the pools (records the caller's
 *                 filters drop are walked too — their signatures are masked by the caller; cheaper than compacting
 *                 the pools); ref_start[n_aln]; min_len = options.min_sv_size
 *   extra_cigar / extra_off   CIGARs of the n_extra SA-derived segments (SVIM_COLLECT.py:33-55)
 *   seg_*[n_segs] one row per segment of every chimeric read, [primary] + supplementaries per read
 *                 (SVIM_inter.py:64): seg_src < n_aln names a record of the pools, otherwise extra alignment
 *                 seg_src - n_aln; seg_tid / seg_pos / seg_rev its reference id, start and strand; seg_qend as in
 *                 svx_segments_rows_dev
 *   read_off      n_reads + 1 offsets into the segment rows
 *   contig_rank, params   as for svx_segments_postpass
 *   part_dev / part_ready   optional (NULL: every part is uploaded from cigar_parts): part_dev[k] != NULL says part k's
 *                 part_ops[k] words are in HBM already, on the context's device (svx_bam_device_pool: the reader
 *                 uploads its pool while it assembles it) — cigar_parts[k] is not read; part_ready[k], when
 *                 part_ready != NULL and the entry is not NULL, is a hipEvent_t the part's producer recorded behind its
 *                 last write: the context's stream waits for it, then moves the words into place device-to-device.
 *                 The submission no longer carries 4 bytes per op over the host link between the walk and the kernels.
 * Output (host arrays):
 *   sig, sig_cap, n_sig    as svx_cigar_extract (SVX_E_CAPACITY with n_sig set when sig_cap is too small)
 *   raw[n_segs]            as svx_segments_classify
 *   post, post_off, post_cnt   as svx_segments_postpass (post_off: n_reads + 1 region offsets, chosen by the caller)
 */
typedef struct svx_collect_in {
    const uint32_t* const* cigar_parts;
    const uint64_t* part_ops;
    uint32_t n_parts;
    const uint64_t* aln_off;
    const int32_t* ref_start;
    uint32_t n_aln;
    uint32_t min_len;
    const uint32_t* extra_cigar;
    const uint64_t* extra_off;
    uint32_t n_extra;
    const uint32_t* seg_src;
    const int32_t* seg_tid;
    const int32_t* seg_pos;
    const uint8_t* seg_rev;
    const int32_t* seg_qend;
    uint32_t n_segs;
    const uint32_t* read_off;
    uint32_t n_reads;
    const int32_t* contig_rank;
    uint32_t n_contigs;
    svx_seg_params params;
    const uint32_t* const* part_dev;
    void* const* part_ready;
} svx_collect_in;

typedef struct svx_collect_out {
    svx_sig_soa sig;
    uint64_t sig_cap;
    uint64_t n_sig;
    svx_raw* raw;
    svx_post* post;
    const uint64_t* post_off;
    uint32_t* post_cnt;
} svx_collect_out;

int svx_collect_batch(svx_ctx* ctx, const svx_collect_in* in, svx_collect_out* out);

/*
 * The kernels of svx_collect_batch on inputs that are already in HBM, asynchronously: what that call enqueues
 * between its uploads and its read-backs — svx_cigar_extract_dev (a1 + a2), then svx_segments_rows_dev,
 * svx_segments_classify_dev and svx_segments_postpass_dev (a3) — on the context's stream, no synchronisation.
 *   d_cigar      the pools' words and, from word n_ops on, the CIGARs of the n_extra SA-derived segments
 *   d_aln_off    n_aln + n_extra + 1 offsets into it (PRECONDITIONS as for svx_cigar_extract_dev)
 *   read_off, post_off   HOST copies (sizes of the per-read scratch and output regions; validated by
 *                svx_collect_batch, here a precondition), d_read_off / d_post_off the same in HBM
 *   d_segs, d_read_len   n_segs rows / n_reads lengths of scratch the chain writes and reads
 *   d_chain_deal, n_chain_blocks   optional: the table svx_chain_deal (below) wrote, uploaded by the caller — which
 *                workgroup computes which reads' rows (8-byte aligned, entries within the submission's reads and
 *                segments: a precondition; the kernel clamps what it indexes with).  Results never depend on it.
 * Outputs as svx_collect_batch, in HBM: d_sig (exactly min(count, sig_cap) signatures), d_n_sig (one uint64),
 * d_raw[n_segs], d_post / d_post_cnt.
 */
typedef struct svx_collect_dev {
    const uint32_t* d_cigar;
    uint64_t n_ops;
    const uint64_t* d_aln_off;
    uint32_t n_aln;
    uint32_t n_extra;
    const int32_t* d_ref_start;
    uint32_t min_len;
    const uint32_t* d_seg_src;
    const int32_t* d_seg_tid;
    const int32_t* d_seg_pos;
    const uint8_t* d_seg_rev;
    const int32_t* d_seg_qend;
    uint32_t n_segs;
    const uint32_t* read_off;
    const uint32_t* d_read_off;
    uint32_t n_reads;
    const int32_t* d_contig_rank;
    uint32_t n_contigs;
    svx_seg_params params;
    svx_sig_soa d_sig;
    uint64_t sig_cap;
    uint64_t* d_n_sig;
    svx_seg* d_segs;
    int32_t* d_read_len;
    svx_raw* d_raw;
    svx_post* d_post;
    const uint64_t* post_off;
    const uint64_t* d_post_off;
    uint32_t* d_post_cnt;
    const uint32_t* d_chain_deal;   /* optional (NULL / 0): the table svx_chain_deal wrote, in HBM */
    uint32_t n_chain_blocks;        /* its return value */
} svx_collect_dev;

int svx_collect_batch_dev(svx_ctx* ctx, const svx_collect_dev* d);

/*
 * Deals the chimeric reads of a submission to the workgroups of the split-segment chain by CIGAR OP COUNT.  The
 * reference takes a read's rows from pysam properties that walk the record's CIGAR (reference_end,
 * query_alignment_start / _end, infer_read_length: SVIM_inter.py:66-81); here a workgroup computes the rows of
 * consecutive reads, and a primary can be anything between a few and 10^5 ops, so equal READ counts leave the launch
 * waiting for the workgroup with the longest primaries.  The caller has every offset in hand when it builds the
 * control block: this helper (host arithmetic, O(n_reads + n_segs)) cuts the reads into consecutive ranges of about
 * equal cost — per segment its CIGAR rounded up to the chain's chunk size, plus a constant per read.
 *   read_off[n_reads + 1], seg_src[n_segs]   as in svx_collect_in
 *   aln_off      offsets of EVERY alignment seg_src can name (svx_collect_dev.d_aln_off's host copy)
 *   deal         out: 2 * (n_reads + 2) words are always enough — {first read, first segment} per workgroup and a
 *                closing {n_reads, n_segs} entry
 * Returns the number of workgroups (entries - 1) — upload the table and pass both as d_chain_deal / n_chain_blocks —,
 * 0 when the submission has too few reads for a table to matter (pass NULL / 0: reads are dealt out in equal
 * counts), or SVX_E_INVALID.  Results never depend on the table; svx_collect_batch builds one itself.
 */
int svx_chain_deal(const uint32_t* read_off, uint32_t n_reads, const uint32_t* seg_src, const uint64_t* aln_off,
                   uint32_t* deal);

/* ------------------------------------------------------------ f-1 on the device ------------------- */
/*
 * BGZF members inflated and checked on the device: what htslib's bgzf_read_block does under every record the
 * reference reads (pysam bam.fetch, SVIM_COLLECT.py:65-68) — inflate the member's raw DEFLATE payload, compare
 * the CRC32 and the length with the member's trailer.  All members of a call at once, a wave per member.
 *   d_in                 compressed payloads (the bytes between a member's header and its 8-byte trailer), anywhere
 *                        in one buffer: member m is d_in[d_in_off[m] .. + d_in_len[m]); the buffer must be readable 3 bytes
 *                        past the end of any member (input words are fetched whole)
 *   d_isize, d_crc       the trailer's ISIZE and CRC32 of every member; a member whose ISIZE exceeds 65536 (no BGZF
 *                        member can) is not decoded: status 2, nothing written
 *   d_out, d_out_off     member m's bytes are written to d_out[d_out_off[m] .. + d_isize[m]); the stretches must be
 *                        separated by at least 8 bytes (and d_out end 8 bytes behind the last one): match copies move
 *                        whole 8-byte words and may touch up to 7 bytes behind a member's end
 *   d_status             per member: 0 ok; 1 malformed stream; 2 length != ISIZE; 3 CRC32 mismatch; 4 input ended early.
 *                        The two paddings above are the only bytes outside a member's own input and output stretch that
 *                        are ever read (3 behind the input) or written (7 behind the output).
 * Asynchronous on the context's stream.
 * Three forms with the same bytes and statuses (svx_inflate.hip).  Shipped: three launches — a WAVE per member parses the bit
 * stream (64 stretches of it decoded at once and resynchronised), storing the literals and writing every match as a token
 * (k_inflate_wparse); a lane per member does the same for whatever the wave parse has left alone — anything but plain
 * fixed / dynamic blocks, every malformed stream — and is the judge of those (k_inflate_parse); a wave per member applies the
 * tokens and takes the CRC-32 (k_inflate_resolve).  The token lists come out of the context's workspace, 175 KB a member,
 * for up to 20 480 members at a time (more members: one set of launches behind the other).  The other two: the lane-per-
 * member parse for every member; and ONE launch, a lane per member that decodes and copies (k_bgzf_inflate, rounds 4-5).
 * svx_bgzf_inflate_set_two_pass chooses for the whole process — this entry and the BAM reader's device leg
 * (svx_bam_set_device_inflate): 0 the one-launch kernel, 2 the lane-per-member parse, any other value the shipped form; it
 * returns the previous choice in the same terms (0 / 2 / 1).  SVX_INFLATE_KERNEL=1|2|3 in the environment starts the process
 * on the one-launch / lane-parse / shipped form.
 */
int svx_bgzf_inflate_dev(svx_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                         const uint32_t* d_isize, const uint32_t* d_crc, uint32_t n_members, uint8_t* d_out,
                         const uint64_t* d_out_off, uint32_t* d_status);
int svx_bgzf_inflate_set_two_pass(int on);
/* Members whose token lists svx_bgzf_inflate_dev keeps at once (default 20 480, 175 KB each; 0: back to the default): a call
 * with more members goes out in slices of that many.  Returns the previous value.  A memory / latency trade-off — a slice
 * costs at least one member's decode latency — and what the tests use to run many slices over few members. */
uint32_t svx_bgzf_inflate_set_arena(uint32_t members);

/*
 * BGZF compression (svx_deflate.hip), the counterpart of svx_bgzf_inflate_dev: the input is cut into blocks of 65 280
 * bytes (htslib's BGZF_BLOCK_SIZE, the last one shorter) and each becomes one gzip member with the BC extra field
 * (BSIZE), raw DEFLATE with dynamic Huffman codes (or a stored block where that would not be smaller: every member is at
 * most 65 536 bytes), CRC32 and ISIZE; the 28-byte EOF member follows.  One workgroup per block; the bytes depend on the
 * input alone.
 *
 * svx_bgzf_deflate_dev: the members of d_in[0 .. n) back to back at d_out (cap >= svx_bgzf_deflate_bound(n), else
 * SVX_E_CAPACITY), then the EOF member; d_member_len[i] = size of member i (ceil(n / 65280) entries), *d_total (device)
 * = bytes written.  n = 0: the EOF member alone.  Enqueued on the context's stream, no synchronisation.
 */
uint64_t svx_bgzf_deflate_bound(uint64_t n);
int svx_bgzf_deflate_dev(svx_ctx* ctx, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap,
                         uint32_t* d_member_len, uint64_t* d_total);
/* Blocks per launch of svx_bgzf_deflate_dev (default 2048; 0: back to the default); returns the previous value. */
uint32_t svx_bgzf_deflate_set_slice(uint32_t blocks);
/* The same container from host bytes: ctx != NULL on that context's device and stream (svx_bgzf_deflate_dev; the
 * context's staging buffers), ctx == NULL with zlib (raw deflate, level 6) on n_threads host threads (<= 0: one per
 * hardware thread, at most 16).  *out (out_len bytes, EOF member included) and *member_len (*n_members data members)
 * are allocated by the library: free both with svx_bgzf_free.  Thread-safe across contexts. */
int svx_bgzf_compress(svx_ctx* ctx, const uint8_t* src, uint64_t n, int n_threads, uint8_t** out, uint64_t* out_len,
                      uint32_t** member_len, uint64_t* n_members);
void svx_bgzf_free(void* p);

/* ------------------------------------------------------------ a5 + a6 ------ */
/*
 * Pair sort + partition: form_partitions (SVIM_COMBINE.py:15-32).
 *
 *   keys[i] = group << 32 | pos, where `group` encodes everything of
 *   Candidate.get_key() (SVCandidate.py:17-19,147-148,292-293,386-387) that
 *   must be EQUAL inside a partition — (type, rank of the contig name under
 *   Python str ordering) — and pos is the non-negative key position.
 *
 * Output: perm[j] = input index of the j-th candidate in stable sorted order
 * (ties keep input order, i.e. hap-1 list then hap-2 list, :17,:182);
 * part_id[j] = partition number of sorted position j; a new partition starts
 * when group differs or |pos - previous pos| > max_dist (strict, :24-26).
 * *n_parts = number of partitions (0 when n == 0).
 */
int svx_pair_partition(svx_ctx* ctx, const uint64_t* keys, uint32_t n, uint32_t max_dist,
                       uint32_t* perm, uint32_t* part_id, uint32_t* n_parts);
int svx_pair_partition_dev(svx_ctx* ctx, const uint64_t* d_keys, uint32_t n, uint32_t max_dist,
                           uint32_t* d_perm, uint32_t* d_part_id, uint32_t* d_n_parts);
/* Same with the caller's knowledge of the key layout: key_bits has a 1 wherever some key may have
 * one (the OR of all keys, or any superset such as `type bits | contig bits | position bits`).
 * Only those bits are sorted on (one launch up to svx_ctx_set_pair_single_launch_max candidates; beyond
 * that P = ceil(live bits / 9) radix passes, P + 2 launches in total), and nothing is read back: fully
 * asynchronous.  svx_pair_partition_dev derives the mask itself with one
 * extra reduction and an 8-byte read-back, which synchronises the stream once. */
int svx_pair_partition_dev_bits(svx_ctx* ctx, const uint64_t* d_keys, uint32_t n, uint32_t max_dist,
                                uint64_t key_bits, uint32_t* d_perm, uint32_t* d_part_id,
                                uint32_t* d_n_parts);

/* ---------------------------------------------------------------- a7 ------- */
/*
 * Batched global (Needleman-Wunsch, unit cost) edit distance, the arithmetic of
 * edlib.align(a, b)["editDistance"] as called by compute_distance
 * (SVIM_COMBINE.py:50,64,76,88,100).  Sequences are bytes in one pool;
 * pair p compares seq[a_off[p] .. a_off[p]+a_len[p]) with
 * seq[b_off[p] .. b_off[p]+b_len[p)).  dist[p] receives the exact distance when
 * it is <= k_max and 0xFFFFFFFF otherwise (complete linkage cut at
 * max_edit_distance only needs "> t").  k_max = 0xFFFFFFFF
 * requests exact distances.
 */
/* The distance is computed in two stages: a wavefront (diagonal-transition, O(n + d^2)) pass resolves
 * every pair whose distance is at most min(k_max, max_edits, max(64, (|a| + |b|) / 32)) — the haplotypes of one
 * variant are long and nearly identical —, the bit-vector kernel (O(n m / 64), banded) the rest.  Both are
 * exact; max_edits (default 1024, at most 4096, 0 = bit-vector kernel only) only moves work between them. */
int svx_ctx_set_edit_wavefront_cap(svx_ctx* ctx, uint32_t max_edits);

int svx_edit_distance_batch(svx_ctx* ctx, const uint8_t* seq, uint64_t seq_bytes,
                            const uint64_t* a_off, const uint32_t* a_len, const uint64_t* b_off,
                            const uint32_t* b_len, uint32_t n_pairs, uint32_t k_max,
                            uint32_t* dist);

/*
 * The same distances with the haplotype strings assembled on the device.  compute_distance
 * (SVIM_COMBINE.py:43-100) aligns  reference[region_start : c.start] + MIDDLE + reference[c.end : region_end]
 * of two candidates; MIDDLE is empty (DEL), the reverse complement of reference[c.start : c.end] (INV),
 * that interval copies + 1 times (DUP_TAN), the inserted sequence (INS) or the source interval (DUP_INT);
 * reference slices are upper-cased (:45-99 `.upper()`), inserted sequences are taken as they are.  Each
 * haplotype is THREE pieces of one byte pool (reference windows — one per partition is enough — and the
 * inserted sequences): bytes pool[off .. off + len), written `repeat` times (0: piece absent), with
 * SVX_PIECE_UPPER (ASCII str.upper()) and / or SVX_PIECE_REVCOMP (read backwards; A<->T, C<->G after
 * the upper-casing, every other byte unchanged — SVIM_COMBINE.py:63).  pieces holds 6 per pair: the
 * three of haplotype a, then the three of b.  Result contract as svx_edit_distance_batch.
 */
#define SVX_PIECE_UPPER 1
#define SVX_PIECE_REVCOMP 2

typedef struct svx_hap_piece {
    uint64_t off;
    uint32_t len;
    uint16_t repeat;
    uint16_t flags;
} svx_hap_piece;

int svx_haplotype_distance_batch(svx_ctx* ctx, const uint8_t* pool, uint64_t pool_bytes,
                                 const svx_hap_piece* pieces, uint32_t n_pairs, uint32_t k_max, uint32_t* dist);

/*
 * The recipes of a PAIR step's jobs from the candidate columns — host arithmetic (threads), the counterpart of the
 * six `reference.fetch` calls and the string concatenations of compute_distance (SVIM_COMBINE.py:43-100) per pair:
 * job j compares rows job_a[j] and job_b[j] (different haplotypes) of partition job_part[j].  Per partition: its SV
 * type (0 DEL, 1 INV, 2 INS, 3 DUP_TAN, 4 DUP_INT), the length of its contig, and ONE reference window in the pool —
 * [win_lo, ...) starting at pool byte win_base — that covers [min start - 100, max end + 100) of all its members.  The
 * pool continues behind the windows at `extra_at` with (in this order) the DUP_INT source intervals the caller fetched
 * (their places per job and haplotype in mid_off / mid_len, n_jobs x 2; NULL without DUP_INT jobs) and the stretches of
 * the inserted-sequence pool the INS jobs' alleles lie in: returned in seq_range as {lo, hi} of the first haplotype
 * table's part and {lo, hi} of the second's (offsets >= seq_split; seq_split < 0: one table) — the caller appends
 * seqs[lo:hi] of both.  pieces receives 6 per job (3 of haplotype a, 3 of b).  worst_copies: the largest `copies` of a
 * tandem job (SVX_E_TOO_LARGE when a piece would repeat more than 65 535 times).
 */
typedef struct svx_recipe_in {
    uint32_t n_rows;
    const uint8_t* type;
    const int64_t* ss;
    const int64_t* se;
    const int64_t* ds;
    const int64_t* q_off;
    const int64_t* q_len;
    const int64_t* copies;
    uint64_t n_jobs;
    const int64_t* job_a;
    const int64_t* job_b;
    const int64_t* job_part;
    uint32_t n_parts;
    const int64_t* part_type;
    const int64_t* part_len;
    const int64_t* win_base;
    const int64_t* win_lo;
    uint64_t extra_at;
    int64_t seq_split;
    const int64_t* mid_off;
    const int64_t* mid_len;
} svx_recipe_in;

int svx_pair_recipes(const svx_recipe_in* in, svx_hap_piece* pieces, int64_t* seq_range, int64_t* worst_copies);
/* The same with the byte pool already in HBM (d_pool: e.g. one upload of the reference windows serving the
 * thresholded and the exact batch of a PAIR step).  pieces and dist stay host arrays and the call synchronises:
 * the stages of the distance computation are planned from read-backs (which pairs the wavefront pass resolved). */
int svx_haplotype_distance_batch_dev(svx_ctx* ctx, const uint8_t* d_pool, uint64_t pool_bytes,
                                     const svx_hap_piece* pieces, uint32_t n_pairs, uint32_t k_max, uint32_t* dist);
/* One call for a PAIR step's whole batch: k_max[p] per pair — the threshold for the pairs of two-member partitions
 * ("<= max_edit_distance?" is all pair_haplotypes needs of them, SVIM_COMBINE.py:120-139), 0xFFFFFFFF (exact) for
 * the pairs of larger partitions, whose dendrogram above the cut decides scipy's label order.  One upload of the
 * pool, one haplotype assembly, one wavefront pass and one bit-vector pass for all of them.  The waits inside the
 * call sleep on a blocking event instead of spinning on the stream. */
int svx_haplotype_distance_batch_mixed(svx_ctx* ctx, const uint8_t* pool, uint64_t pool_bytes,
                                       const svx_hap_piece* pieces, uint32_t n_pairs, const uint32_t* k_max,
                                       uint32_t* dist);

/*
 * Batched complete linkage + flat cut: for every partition p (n_members[p] candidates, condensed
 * distance vector of n(n-1)/2 doubles, partition after partition in `dist`)
 *     fcluster(linkage(y, method="complete"), cutoff, criterion="distance")
 * as the reference calls scipy at SVIM_COMBINE.py:134-135 (haplotype edit distances, cut at
 * max_edit_distance), :155-156 (breakend span-position distance, cut at 0.3) and SVIM_inter.py:47-48
 * (inversion breakpoints of one read, cut at 0.3).  labels (one per member, partition after
 * partition) are scipy's 1-based flat-cluster labels IN SCIPY'S ORDER — the reference takes the
 * coordinates of a paired call from cluster[0] (SVIM_COMBINE.py:184-363), so the order is part of the
 * result.  Distances are compared exactly as doubles (scipy's float64).  Partitions of one member get
 * label 1.  Any partition size is accepted.
 * Partitions of fewer than `group_min` members (svx_ctx_set_linkage_group_min) run one LANE each; larger ones, up to
 * 2048 members, one WORKGROUP each: the same procedure with the nearest-neighbour search, the distance update and
 * the sort of the merges spread over the group, on the full n x n matrix — in LDS up to SVX_LINKAGE_GROUP_LDS_N
 * members, in the context workspace beyond.  Labels are identical on both.
 */
int svx_linkage_cut_batch(svx_ctx* ctx, const double* dist, const uint32_t* n_members, uint32_t n_parts,
                          double cutoff, uint32_t* labels);
#define SVX_LINKAGE_GROUP_LDS_N 128
/* Smallest partition that takes the workgroup-per-partition kernel.  0 restores the default (16: the smallest size
 * measured, from which on the group kernel is the faster one); 0xFFFFFFFF sends every partition down the lane path. */
int svx_ctx_set_linkage_group_min(svx_ctx* ctx, uint32_t n);
/* Asynchronous form: distances, member counts and labels in HBM; the HOST copy of n_members only sizes the scratch
 * of partitions too large for LDS and says which launches have work (not read after the call returns).  No
 * synchronisation. */
int svx_linkage_cut_batch_dev(svx_ctx* ctx, const double* d_dist, const uint32_t* n_members,
                              const uint32_t* d_n_members, uint32_t n_parts, double cutoff, uint32_t* d_labels);

/*
 * Greedy one-to-one assignment, batched.  Partition p holds n_base[p] x n_comp[p] distances, row-major (base-major),
 * partitions back to back; 0xFFFFFFFF = the pair may not match.  Repeat per partition: among the pairs (i, j) with i and
 * j both unmatched and dist < 0xFFFFFFFF take the smallest under the order (dist, i, j); match them; stop when none is
 * left — i.e. the scan of the eligible pairs sorted by (dist, i, j).  Greedy, not optimal: [[1, 2], [2, 100]] gives
 * (0, 0) and (1, 1).
 * match_base / match_comp: per member, partitions back to back, the partner's index inside its partition or 0xFFFFFFFF.
 * All pointers are HOST pointers; the call runs on the context's stream and returns with the outputs written.
 * n_parts == 0 and partitions with n_base == 0 or n_comp == 0 are valid (their members stay unmatched).  SVX_E_INVALID
 * for a null pointer where the counts call for data, SVX_E_TOO_LARGE for a partition of more than 2^20 pairs (nothing
 * launched, the context stays usable).
 * Partitions of fewer than `group_min` pairs (svx_ctx_set_match_group_min) run one LANE each, on the matrix where the
 * call staged it and with the outputs as their only state; larger ones one WORKGROUP each: the matrix in LDS up to
 * SVX_MATCH_LDS_PAIRS pairs (in the context's scratch beyond), a cached minimum per row, and per round a min-reduction
 * over the rows and a rescan of only the rows whose cached column was just taken.  The outputs are identical on both.
 */
int svx_match_greedy_batch(svx_ctx* ctx, const uint32_t* dist, const uint32_t* n_base, const uint32_t* n_comp,
                           uint32_t n_parts, uint32_t* match_base, uint32_t* match_comp);
#define SVX_MATCH_LDS_PAIRS 32768
/* Fewest pairs of a partition that takes the workgroup-per-partition kernel.  0 restores the default (9: 3 x 3 is the
 * smallest size measured from which the group kernel is the faster one); 0xFFFFFFFF sends every
 * partition down the lane path. */
int svx_ctx_set_match_group_min(svx_ctx* ctx, uint32_t pairs);

/*
 * Interval containment, batched: does ONE interval of list l contain query window q, for every (l, q)?
 * A key is contig << 32 | position.  List l owns the entries list_off[l] .. list_off[l+1] of start_key / end_key
 * (list_off[0] = 0, n_lists + 1 offsets), with start_key non-decreasing inside the list; the end keys are in no order.
 *     out[l * n_q + q] = 1  when list l holds an i with start_key[i] <= q_lo[q] and end_key[i] >= q_hi[q],
 *                        0  otherwise
 * — both bounds inclusive, and never the union of two intervals.  All pointers are HOST pointers; the call returns
 * with `out` written.  SVX_E_INVALID (nothing launched, the context stays usable) for a list that is out of order, for
 * an interval or a query whose two keys lie on different contigs, and for q_lo > q_hi.  n_lists == 0, n_q == 0 and
 * empty lists are valid; an empty list answers 0 everywhere.
 * Two launches: an inclusive prefix maximum of end_key inside every list (one workgroup per list,
 * SVX_COVER_SCAN_CHUNK entries per pass, into the context workspace), then per (list, query) the upper bound of q_lo
 * among the start keys and one compare with the prefix maximum in front of it — with the contig in the high word an
 * interval of an earlier contig ends below every key of the query's contig, and one of a later contig is outside the
 * prefix.
 */
#define SVX_COVER_SCAN_CHUNK 1024
int svx_cover_query(svx_ctx* ctx, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off,
                    uint32_t n_lists, const uint64_t* q_lo, const uint64_t* q_hi, uint32_t n_q, uint8_t* out);

/*
 * svx_cover_query's question answered with WHICH interval: inputs, layout and refusals are those of svx_cover_query (one
 * checker serves both), the output is a word per (list, query):
 *     out[l * n_q + q] = the index inside list l of the covering entry, SVX_COVER_NONE when none covers.
 * Of the list's entries with start_key <= q_lo[q] the one with the largest end key is taken, the lowest index among
 * equal end keys; it is the answer when its end key is >= q_hi[q].  So out != SVX_COVER_NONE exactly where
 * svx_cover_query answers 1.  SVX_E_TOO_LARGE for a list of 2^32 - 1 entries or more.
 * Two launches, as svx_cover_query's: the prefix maximum runs as a prefix arg-max over (end key, index) pairs.
 */
#define SVX_COVER_NONE 0xFFFFFFFFu
int svx_cover_locate(svx_ctx* ctx, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off,
                     uint32_t n_lists, const uint64_t* q_lo, const uint64_t* q_hi, uint32_t n_q, uint32_t* out);

/*
 * Lift-over through the CIGAR, batched: where does reference position q_ref[q] lie on the query sequence (SEQ) of
 * alignment q_aln[q]?  `cigar` holds the BAM-native words (len << 4 | op) of n_aln alignments back to back, alignment a
 * owning aln_off[a] .. aln_off[a+1] (aln_off[0] = 0) and starting at reference position ref_start[a].  With r = q_ref[q],
 * walking the ops of the alignment with a reference cursor (M D N = X advance it) and a query cursor that counts SEQ
 * bases (M I S = X advance it; H, P and op codes above 8 advance nothing):
 *     SVX_LIFT_ALIGNED   r lies inside an M / = / X op: out_query = the query offset of the base aligned to r
 *     SVX_LIFT_DELETED   r lies inside a D / N op: out_query = the query offset of the next base behind the op
 *     SVX_LIFT_END       r is the first reference position behind the alignment: out_query = the query offset behind the
 *                        last reference-consuming op (trailing I / S are not counted)
 *     SVX_LIFT_OUTSIDE   anything else (also every position of an alignment without reference-consuming ops): out_query = 0
 * Bases inserted immediately in front of the op that covers r lie to the left of the lifted point.
 * All pointers are HOST pointers (svx_cigar_lift_dev: `d_cigar` is a pool of n_ops words in HBM, complete — a reader's
 * device pool after its wait —, the rest host pointers); the call returns with both outputs written.  SVX_E_INVALID,
 * nothing launched and the context usable, for aln_off[0] != 0, decreasing offsets, q_aln[q] >= n_aln and (dev)
 * aln_off[n_aln] > n_ops; SVX_E_NOMEM when the workspace cannot be had.  n_q == 0, n_aln == 0 and alignments without
 * ops are valid.
 * Four launches, nothing handed between workgroups inside one: the (reference, query) consumption of every op summed per
 * chunk of SVX_LIFT_CHUNK ops; one workgroup's exclusive scan of the chunk sums, SVX_LIFT_CHUNK of them per pass with a
 * carry; the inclusive 64-bit prefixes of both per op into the context workspace (a pool's reference consumption exceeds
 * 2^32); one lane per query: the upper bound of r - ref_start + prefix(first op - 1) among its alignment's reference
 * prefixes.  With n_q == 0 nothing is looked at.
 */
#define SVX_LIFT_OUTSIDE 0
#define SVX_LIFT_ALIGNED 1
#define SVX_LIFT_DELETED 2
#define SVX_LIFT_END 3
#define SVX_LIFT_CHUNK 1024
int svx_cigar_lift(svx_ctx* ctx, const uint32_t* cigar, const uint64_t* aln_off, const int32_t* ref_start, uint32_t n_aln,
                   const uint32_t* q_aln, const int64_t* q_ref, uint32_t n_q, uint32_t* out_query, uint8_t* out_state);
int svx_cigar_lift_dev(svx_ctx* ctx, const uint32_t* d_cigar, uint64_t n_ops, const uint64_t* aln_off, const int32_t* ref_start,
                       uint32_t n_aln, const uint32_t* q_aln, const int64_t* q_ref, uint32_t n_q, uint32_t* out_query,
                       uint8_t* out_state);

/*
 * Single coverage, batched: where does EXACTLY one entry of list l lie over the reference?  The lists are laid out as
 * for svx_cover_query; an entry is the half-open key range [start_key, end_key).  With depth(p) the number of entries
 * of the list with start <= p < end, the list's segments are the maximal ranges [a, b) on which depth is 1 and the one
 * covering entry is the same entry throughout — two entries that abut give two abutting segments, never one —, in
 * ascending order:
 *     seg_lo / seg_hi[seg_off[l] .. seg_off[l+1])     the segments of list l, seg_off[0] = 0, contiguous over the lists
 * The caller provides room for list_off[n_lists] segments (a list never has more segments than entries) and for
 * n_lists + 1 offsets.  All pointers are HOST pointers; the call returns with seg_off and seg_off[n_lists] segments
 * written.  SVX_E_INVALID (nothing launched, the context stays usable) for list_off[0] != 0, decreasing offsets, a list
 * that is out of order, an entry whose two keys lie on different contigs and an entry with end <= start; the message
 * names the list and the entry.  n_lists == 0 and empty lists are valid (seg_off[l+1] == seg_off[l]).
 * Three launches.  With the entries in start order, slot k is [s_k, s_k+1), the last one open to the right; m1 >= m2
 * being the two largest end keys of entries 0..k, depth is 1 inside the slot exactly on
 * [max(s_k, m2), min(s_k+1, m1)): one workgroup per list scans (m1, m2) under "top two of the four",
 * SVX_COVER_SCAN_CHUNK slots per pass, and compacts the non-empty candidates list-locally into the context workspace;
 * an exclusive sum of the lists' counts gives seg_off; a third launch moves every list's segments to their place.
 */
int svx_cover_single(svx_ctx* ctx, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off,
                     uint32_t n_lists, uint64_t* seg_lo, uint64_t* seg_hi, uint64_t* seg_off);

/*
 * Mismatching columns, batched: where do the aligned bases of alignment a differ from the reference?  `cigar`, `aln_off`
 * and `ref_start` are svx_cigar_lift's.  `bases` is ONE pool of n_bases ASCII bytes in any case; alignment a's reference
 * window — the reference bases [ref_start[a], ref_start[a] + ref_len[a]) — lies at bases[ref_off[a] ..], its SEQ in BAM
 * orientation, soft clips included, at bases[qry_off[a] .. qry_off[a] + qry_len[a]).  The definition is this loop:
 *     r = q = 0
 *     for every op (code, len) of alignment a:
 *         if code is M, = or X:
 *             for j in 0 .. len - 1, if r + j < ref_len[a] and q + j < qry_len[a]:
 *                 R = bases[ref_off[a] + r + j] & 0xDF;  Q = bases[qry_off[a] + q + j] & 0xDF
 *                 if R and Q are both one of 'A' 'C' 'G' 'T' and R != Q:
 *                     emit (a, ref_start[a] + r + j, q + j, R, Q)
 *         if code is M D N = X: r += len          (svx_cigar_lift's cursors; note that svx_cigar_extract's
 *         if code is M I S = X: q += len           reference cursor does NOT advance over N)
 *         H, P and codes above 8 advance nothing
 * A column outside either length emits nothing and none of its bytes is compared; a CIGAR that uses more bases than the
 * lengths say is not an error.  Output (SoA, 14 B per event): aln, ref_pos, qry_pos (uint32), ref_base, qry_base (upper
 * case), ascending by (alignment, ref_pos) and identical from run to run — positions are dealt out to lanes and the rows
 * placed by prefix sums, no atomics.  `cap` / `n_out` as for svx_cigar_extract: *n_out always receives the exact count,
 * min(count, cap) rows are written, SVX_E_CAPACITY beyond cap.
 * All pointers are HOST pointers (svx_cigar_mismatch_dev: `d_cigar` is a pool of n_ops words in HBM, complete, as for
 * svx_cigar_lift_dev); the call returns with the rows written.  SVX_E_INVALID — nothing launched, the context usable, the
 * message names the alignment — for aln_off[0] != 0, decreasing offsets, a negative ref_start, ref_start + ref_len above
 * 2^32 - 1, ref_off + ref_len or qry_off + qry_len above n_bases, and (dev) aln_off[n_aln] > n_ops.  n_aln == 0,
 * alignments without ops and zero lengths are valid.  Limits: per-alignment query cursor sums < 2^32; fewer than 2^31 - 1
 * tiles and chunks of ops (SVX_E_TOO_LARGE).
 * Six launches: svx_cigar_lift's three for the 64-bit prefixes; one workgroup per tile of SVX_MISMATCH_TILE reference
 * positions of one alignment's window, 16 positions per lane, counting; one workgroup's exclusive scan of the tile counts;
 * the tile launch again, writing.
 */
#define SVX_MISMATCH_TILE 4096
typedef struct svx_mismatch_soa {
    uint32_t* aln;
    uint32_t* ref_pos;
    uint32_t* qry_pos;
    uint8_t* ref_base;
    uint8_t* qry_base;
} svx_mismatch_soa;
int svx_cigar_mismatch(svx_ctx* ctx, const uint32_t* cigar, const uint64_t* aln_off, const int32_t* ref_start, uint32_t n_aln,
                       const uint8_t* bases, uint64_t n_bases, const uint64_t* ref_off, const uint32_t* ref_len,
                       const uint64_t* qry_off, const uint32_t* qry_len, svx_mismatch_soa out, uint64_t cap, uint64_t* n_out);
int svx_cigar_mismatch_dev(svx_ctx* ctx, const uint32_t* d_cigar, uint64_t n_ops, const uint64_t* aln_off, const int32_t* ref_start,
                           uint32_t n_aln, const uint8_t* bases, uint64_t n_bases, const uint64_t* ref_off, const uint32_t* ref_len,
                           const uint64_t* qry_off, const uint32_t* qry_len, svx_mismatch_soa out, uint64_t cap, uint64_t* n_out);

/*
 * Left shift of small gaps, batched: how many columns can insertion or deletion e move to the left inside its alignment
 * without changing the aligned haplotype?  `bases`, `ref_off`, `ref_len`, `qry_off`, `qry_len` and `ref_start` are
 * svx_cigar_mismatch's.  An event is one row of svx_cigar_extract: ev_aln its alignment, ev_ref_pos / ev_qry_pos the row's
 * ref_pos / read_pos (the first reference position and SEQ offset behind the gap's left edge), ev_len its length, ev_type
 * SVX_SIG_INS or SVX_SIG_DEL; ev_limit is the most steps the event may take — the entry reads no CIGAR, the caller states
 * how far an event may move (up to the column behind the previous gap, say).  With a = ev_aln[e], ref = bases + ref_off[a],
 * qry = bases + qry_off[a], r = ev_ref_pos[e] - ref_start[a], q = ev_qry_pos[e], L = ev_len[e] and up(x) = x & 0xDF, the
 * definition is this loop:
 *     k = 0
 *     while k < ev_limit[e]:
 *         i = k + 1
 *         stop unless i <= r, i <= q, r - i < ref_len[a], q - i < qry_len[a]
 *         R = up(ref[r - i]);  Q = up(qry[q - i])              the aligned column the gap would pass
 *         stop unless R is one of 'A' 'C' 'G' 'T' and R == Q
 *         INS: stop unless q + L - i < qry_len[a];  X = up(qry[q + L - i])
 *         DEL: stop unless r + L - i < ref_len[a];  X = up(ref[r + L - i])
 *         stop unless X == R
 *         k = i
 *     shift[e] = k
 * The shifted event is (ev_ref_pos - k, ev_qry_pos - k, L), an insertion's bases SEQ[ev_qry_pos - k .. ev_qry_pos - k + L).
 * A step whose indices fall outside a range stops the walk: no byte outside [ref_off, ref_off + ref_len) or [qry_off,
 * qry_off + qry_len) takes part in a result.  Events come in any order; shift[e] depends on event e alone and is identical
 * from run to run.
 * All pointers are HOST pointers; the call returns with `shift` written.  SVX_E_INVALID — nothing launched, the context
 * usable, the message names the alignment or the event — for ev_aln >= n_aln, ev_ref_pos < ref_start, a type that is neither
 * SVX_SIG_INS nor SVX_SIG_DEL, ev_len == 0, a negative ref_start, and ref_off + ref_len or qry_off + qry_len above n_bases.
 * n_ev == 0, n_aln == 0 (without events) and ev_limit == 0 are valid.  SVX_E_TOO_LARGE for more than 2^31 - 257 events.
 * Two forms with identical outputs: one LANE per event walks at most `lane_steps` steps (svx_ctx_set_shift_lane_steps); the
 * events that still match with steps left are listed, in event order and without atomics (a workgroup scan, one exclusive
 * sum over workgroups), the host reads the count back, and one WAVE per listed event goes on from there,
 * SVX_SHIFT_WAVE_COLS steps per iteration (four bytes of each stream per lane) and one ballot of the failing lanes.  Three
 * launches, and a fourth where the list is not empty.
 */
#define SVX_SHIFT_WAVE_COLS 256
int svx_indel_shift(svx_ctx* ctx, const uint8_t* bases, uint64_t n_bases, const uint64_t* ref_off, const uint32_t* ref_len,
                    const uint64_t* qry_off, const uint32_t* qry_len, const int32_t* ref_start, uint32_t n_aln,
                    const uint32_t* ev_aln, const uint32_t* ev_ref_pos, const uint32_t* ev_qry_pos, const uint32_t* ev_len,
                    const uint8_t* ev_type, const uint32_t* ev_limit, uint32_t n_ev, uint32_t* shift);
/* Steps the lane form walks before it hands an event that still matches to the wave form.  A negative value restores the
 * default SVX_SHIFT_LANE_STEPS (8: on the one batch measured — 10^6 synthetic events, one in a thousand with a shift of 100
 * to 5000 — the kernels take 0.080 / 0.081 / 0.083 / 0.086 / 0.095 ms at 4 / 8 / 16 / 32 / 64 steps, 0.47 ms with the wave
 * form alone and 1.08 ms with the lane form alone; 8 is the flat bottom's value that keeps every shift of the fixture in
 * the lane form); 0 sends every event with a positive limit to the wave form; INT32_MAX keeps every event
 * in the lane form. */
#define SVX_SHIFT_LANE_STEPS 8
int svx_ctx_set_shift_lane_steps(svx_ctx* ctx, int32_t steps);

/*
 * Haplotype replay, batched: which string do a job's edits make of its reference window, and are two such strings the
 * same?  `bases` is ONE pool of n_bases bytes that holds the windows and the alternative alleles; the entry compares bytes
 * as they are (a caller that wants case ignored hands over one case).  Job j < n_jobs is the window bases[win_off[j] ..
 * win_off[j] + win_len[j]) with the edits ed_first[j] .. ed_first[j + 1] - 1 (n_jobs + 1 entries, ed_first[0] == 0), taken
 * in the given order; edit e replaces the ed_ref_len[e] window bytes from ed_start[e] on (relative to the window) by
 * bases[ed_alt_off[e] .. ed_alt_off[e] + ed_alt_len[e]).  Pair k < n_pairs names two jobs.  The definition is this loop:
 *     p = 0;  string = "";  order = inside = true
 *     for every edit e of job j, in the given order:
 *         order  = false unless ed_start[e] >= p, and, for e not the job's first, ed_start[e] > ed_start[e - 1]
 *         inside = false unless ed_start[e] + ed_ref_len[e] <= win_len[j]
 *         string += win[p : ed_start[e]] + alt(e)
 *         p = ed_start[e] + ed_ref_len[e]
 *     string += win[p : win_len[j]]
 *     status[j]  = 1 unless order, else 2 unless inside, else 0
 *     out_len[j] = len(string) where status[j] == 0, else 0 (and the job has no string)
 *     equal[k]   = 1 iff status[pair_a[k]] == status[pair_b[k]] == 0 and both strings have equal lengths and equal bytes
 * So two edits at one start and an edit that begins inside the one before it are out of order; an edit that begins exactly
 * where the one before it ends is in order; a job paired with itself and two empty strings are equal.  Every output
 * depends on its own job or pair alone and is identical from run to run.
 * Strings: with out != NULL the strings of all jobs, one behind the other in job order, go to `out` and their offsets to
 * out_off (n_jobs + 1 entries; may be NULL); `cap` / `n_out` as for svx_cigar_extract: *n_out (may be NULL) always receives
 * the exact total, min(total, cap) bytes are written, SVX_E_CAPACITY beyond cap.  With out == NULL the strings stay in the
 * workspace, cap is ignored, and out_off and n_out are still served.
 * All pointers are HOST pointers; the call returns with the outputs written.  SVX_E_INVALID — nothing launched, the context
 * usable, the message names the job, the edit or the pair — for ed_first[0] != 0, a decreasing ed_first, ed_first[n_jobs]
 * != n_edits, a window or an alternative allele that ends behind n_bases, a pair index >= n_jobs, and a null pointer where
 * a count is positive.  n_jobs == 0, n_pairs == 0, jobs without edits and windows of length 0 are valid.  SVX_E_TOO_LARGE
 * when the windows plus the alternative alleles of one call (the sum of all win_len and all ed_alt_len, which no total
 * exceeds) pass SVX_REPLAY_MAX_BYTES — the output offsets are 32 bits wide —, or when the pairs' strings (for each pair the
 * shorter member, bounded the same way) pass 2^31 - 1 tiles.
 * Count, scan, emit: one scan over the edits for the bytes in front of each and for the status, one over the jobs for the
 * offsets, then a workgroup per tile of SVX_REPLAY_TILE consecutive OUTPUT BYTES of the whole call, 16 per lane — bytes
 * are dealt out, not jobs —; the pairs' bytes are dealt out the same way and a lane that sees a difference clears the flag.
 * No atomics; twelve launches at most (svim_asm_amd/csrc/svx_replay.hip lists them).
 * Measured once (2026-10-21, one MI355X, tools/replay_probe.py, synthetic: 10^6 phased clusters, 4 * 10^6 jobs and pairs,
 * 2.65 * 10^6 edits, a pool of 101 MB, 393 MB of strings): the call 17.5 ms on a host clock, of which the kernels 1.67 ms
 * (emit and compare 1.44), the uploads alone 4.5 ms (a quarter), and the rest the host's checks over every job, edit and
 * pair, the read-backs and the binding; the plain splice in numpy, one thread: 2.9 s.  DESIGN.md 3.20.
 */
#define SVX_REPLAY_TILE 4096
#define SVX_REPLAY_MAX_BYTES 0xFFFFF000ull
int svx_variant_replay(svx_ctx* ctx, const uint8_t* bases, uint64_t n_bases, const uint64_t* win_off, const uint32_t* win_len,
                       const uint32_t* ed_first, uint32_t n_jobs, const uint32_t* ed_start, const uint32_t* ed_ref_len,
                       const uint64_t* ed_alt_off, const uint32_t* ed_alt_len, uint32_t n_edits, const uint32_t* pair_a,
                       const uint32_t* pair_b, uint32_t n_pairs, uint32_t* out_len, uint8_t* status, uint8_t* equal, uint8_t* out,
                       uint32_t* out_off, uint64_t cap, uint64_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* SVX_H_ */
