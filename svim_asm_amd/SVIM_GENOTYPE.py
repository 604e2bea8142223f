"""Genotype known SV sites in an assembly's alignments (svim-asm-genotype).

SITES are the deletions and insertions of a VCF read as a site list (vcfin.read_sites: the genotype columns do not
matter).  Per site and haplotype:
  * the window — DEL [s - f, e + f), INS [p - f, p + f), clamped to the contig — is looked up among the reference
    intervals of the haplotype's alignments (the records COLLECT visits): all windows against all haplotypes' lists in
    ONE svx_cover_locate, which also says WHICH alignment spans;
  * both ends of every spanned window are lifted through that alignment's CIGAR onto its sequence, all of a haplotype's
    in ONE svx_cigar_lift; the observed bases O = SEQ[lift(lo) : lift(hi)] come from ONE sequence_slices call per file;
  * O is compared with REF = ref[lo:hi] and with ALT = ref[lo:s] + ref[e:hi] (DEL) or ref[lo:p] + seq + ref[p:hi] (INS),
    both assembled on the device from pieces of one pool (reference windows, inserted bytes, observed bytes), all pairs
    of all haplotypes in ONE svx_haplotype_distance_batch_mixed with the site's limit
    L = max(--max_edit_distance, floor(--max_relative_distance * size)) as threshold: exact up to L, "more" beyond; a
    pair whose lengths differ by more than L gets no job and is "more".
The call: `.` not_spanned without a spanning alignment; 1 when d_alt <= L and below d_ref; 0 when d_ref <= L and below
d_alt; `.` ambiguous when both are equal and within L; `.` other_allele when both are "more".  Where several
alignments span a window, svx_cover_locate's choice stands."""
import json
import logging
import os
import time

import numpy as np

from svim_asm_amd import SVIM_COLLECT, SVIM_COMBINE as _combine, _lib, vcfin
from svim_asm_amd.table import T_INS

MORE = 0xFFFFFFFF
CALL_REF, CALL_ALT, NOT_SPANNED, AMBIGUOUS, OTHER_ALLELE = range(5)
CALL_NAMES = ("0", "1", "not_spanned", "ambiguous", "other_allele")
CALL_TEXT = np.array([b"0", b"1", b".", b".", b"."])
_NOT_GENOTYPED = ("multiallelic", "complex", "unresolved", "other", "filtered")
STAGES = ("read", "load", "locate", "lift", "slices", "distances", "write")  # what a `timing` dictionary receives
FORMAT_LINES = (b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
                b'##FORMAT=<ID=DR,Number=.,Type=Integer,Description="Edit distance of each haplotype\'s bases over the site to the '
                b'reference allele (. beyond the limit or without a spanning alignment)">',
                b'##FORMAT=<ID=DA,Number=.,Type=Integer,Description="Edit distance of each haplotype\'s bases over the site to the '
                b'alternative allele (. beyond the limit or without a spanning alignment)">')


def _clock(timing, stage, t0):
    now = time.perf_counter()
    if timing is not None:
        timing[stage] = timing.get(stage, 0.0) + now - t0
    return now


def site_windows(contig, s, e, contig_len, flank):
    """[lo, hi) of every site: [s - flank, e + flank) clamped to the contig (an insertion has s == e)."""
    lo = np.maximum(s - flank, 0)
    hi = np.minimum(e + flank, contig_len[contig])
    return lo, np.maximum(hi, lo)


def limit_of(size, options):
    """Largest distance at which an allele still counts as observed: max(--max_edit_distance, floor(rel * size))."""
    rel = np.floor(float(getattr(options, "max_relative_distance", 0.0) or 0.0) * size).astype(np.int64)
    return np.maximum(int(options.max_edit_distance), rel)


def _haplotype_lists(samples, contigs, ctx):
    """Per haplotype (start_key, end_key, record) of the alignments COLLECT visits, keys on the GENOME's contig indices,
    sorted by start key with ties in loop order."""
    index = {name: i for i, name in enumerate(contigs)}
    out = []
    for s in samples:
        tid, start, end, rec = SVIM_COLLECT._coverage_records_of(s, ctx)
        base = getattr(s.bam, "_bam", s.bam)
        names = list(base.references)
        to_genome = np.array([index.get(n, -1) for n in names] + [-1], dtype=np.int64)
        g = to_genome[tid] if len(tid) else np.zeros(0, np.int64)
        if len(g) and bool((g < 0).any()):
            raise ValueError("the alignments lie on contig '%s', which the genome does not have" % names[int(tid[int(np.flatnonzero(g < 0)[0])])])
        lo_key, hi_key = (g << 32) | start, (g << 32) | end
        if len(lo_key) > 1 and bool((lo_key[1:] < lo_key[:-1]).any()):  # (the genome orders its contigs otherwise)
            o = np.argsort(lo_key, kind="stable")
            lo_key, hi_key, rec = lo_key[o], hi_key[o], rec[o]
        out.append((lo_key.astype(np.uint64), hi_key.astype(np.uint64), rec))
    return out


def _lift(s, ctx, rec, lo, hi):
    """Query offsets of `lo` and `hi` on records `rec` of sample s: ONE cigar_lift, lo then hi."""
    r = s.rec
    base = getattr(r, "base", None)
    pool = base.device_pool(wait=True) if base is not None and hasattr(base, "device_pool") and r.cigar is base._cigar else None
    off = np.asarray(r.cig_off, dtype=np.uint64)
    q_aln, q_ref = np.concatenate((rec, rec)).astype(np.uint32), np.concatenate((lo, hi)).astype(np.int64)
    if pool is not None:
        query, state = ctx.cigar_lift(pool[0], off, r.pos, q_aln, q_ref, n_ops=int(r.cig_off[-1]))
    else:
        query, state = ctx.cigar_lift(r.cigar, off, r.pos, q_aln, q_ref)
    if bool((np.asarray(state) == _lib.LIFT_OUTSIDE).any()):  # (cannot happen: the interval contains the window)
        raise ValueError("a window's end lies outside the alignment that spans it")
    n = len(rec)
    query = np.asarray(query, dtype=np.int64)
    return query[:n], np.maximum(query[n:], query[:n])


def genotype_sites(t, rows, reference, samples, options, ctx, timing=None):
    """t: the sites' CandidateTable (vcfin), rows: the ones to genotype, samples: SVIM_COLLECT._prepare'd haplotypes.
    Returns (call [n_hap, n] of CALL_* codes, d_ref, d_alt [n_hap, n] uint32 with MORE where unknown)."""
    H, n = len(samples), len(rows)
    call = np.full((H, n), NOT_SPANNED, np.uint8)
    d_ref, d_alt = np.full((H, n), MORE, np.uint32), np.full((H, n), MORE, np.uint32)
    if n == 0 or H == 0:
        return call, d_ref, d_alt
    t0 = time.perf_counter()
    contigs = list(t.contigs)
    contig_len = np.asarray(t.contig_len, dtype=np.int64)
    ins = t.type[rows] == T_INS
    contig = np.where(ins, t.dc[rows], t.sc[rows]).astype(np.int64)
    s = np.where(ins, t.ds[rows], t.ss[rows]).astype(np.int64)
    e = np.where(ins, t.ds[rows], t.se[rows]).astype(np.int64)
    q_len = np.where(ins, t.q_len[rows], 0).astype(np.int64)
    q_off = t.q_off[rows].astype(np.int64)
    size = np.where(ins, q_len, e - s)
    limit = limit_of(size, options)
    lo, hi = site_windows(contig, s, e, contig_len, int(options.flank))
    # ---- which alignment spans: every window against every haplotype's list, one call
    lists = _haplotype_lists(samples, contigs, ctx)
    list_off = np.zeros(H + 1, np.uint64)
    np.cumsum([len(l[0]) for l in lists], out=list_off[1:])
    c64 = contig.astype(np.uint64) << np.uint64(32)
    where = np.asarray(ctx.cover_locate(np.concatenate([l[0] for l in lists]), np.concatenate([l[1] for l in lists]), list_off,
                                        c64 | lo.astype(np.uint64), c64 | hi.astype(np.uint64)), dtype=np.int64).reshape(H, n)
    t0 = _clock(timing, "locate", t0)
    # ---- the observed bases: per haplotype one lift and one slice call
    spanned, obs_pool, obs_off = [], [], []
    for h, smp in enumerate(samples):
        k = np.flatnonzero(where[h] != _lib.COVER_NONE)
        spanned.append(k)
        if not len(k):
            obs_pool.append(np.zeros(0, np.uint8))
            obs_off.append(np.zeros(1, np.int64))
            continue
        rec = lists[h][2][where[h][k]]
        t0 = time.perf_counter()
        q_lo, q_hi = _lift(smp, ctx, rec, lo[k], hi[k])
        t0 = _clock(timing, "lift", t0)
        pool, off = smp.rec.sequence_slices(rec, q_lo, q_hi)
        SVIM_COLLECT._verify_pending(smp)
        _clock(timing, "slices", t0)
        obs_pool.append(np.asarray(pool, dtype=np.uint8))
        obs_off.append(np.asarray(off, dtype=np.int64))
    t0 = time.perf_counter()
    # ---- one pool: reference windows, inserted bytes, observed bytes
    win, win_off = _combine._fetch_windows(reference, contigs, contig, lo, hi, False)
    if not np.array_equal(win_off[1:] - win_off[:-1], hi - lo):
        raise ValueError("reference windows shorter than the index says")
    seqs = np.asarray(t.seqs, dtype=np.uint8)
    seq_at = len(win)
    obs_at = seq_at + len(seqs) + np.concatenate(([0], np.cumsum([len(p) for p in obs_pool])))
    pool = np.concatenate([win, seqs] + obs_pool)
    # ---- jobs: (haplotype, spanned site) x (REF, ALT) wherever the lengths differ by no more than the limit
    hap = np.concatenate([np.full(len(k), h, np.int64) for h, k in enumerate(spanned)])
    site = np.concatenate(spanned)
    o_off = np.concatenate([obs_at[h] + obs_off[h][:-1] for h in range(H)])
    o_len = np.concatenate([obs_off[h][1:] - obs_off[h][:-1] for h in range(H)])
    ref_len = (hi - lo)[site]
    alt_len = ref_len + np.where(ins[site], q_len[site], -(e - s)[site])
    up = _lib.PIECE_UPPER
    batches = []
    for is_alt, b_len in ((0, ref_len), (1, alt_len)):
        j = np.flatnonzero(np.abs(o_len - b_len) <= limit[site])
        k = site[j]
        pieces = np.zeros((len(j), 2, 3), dtype=_lib.HAP_PIECE_DTYPE)

        def put(side, slot, off, ln):
            ok = ln > 0
            pieces["off"][:, side, slot] = np.where(ok, off, 0)
            pieces["len"][:, side, slot] = np.where(ok, ln, 0)
            pieces["repeat"][:, side, slot] = ok
            pieces["flags"][:, side, slot] = np.where(ok, up, 0)
        put(0, 0, o_off[j], o_len[j])
        if not is_alt:
            put(1, 0, win_off[:-1][k], (hi - lo)[k])
        else:
            put(1, 0, win_off[:-1][k], (s - lo)[k])
            put(1, 1, seq_at + q_off[k], q_len[k])
            put(1, 2, win_off[:-1][k] + (e - lo)[k], (hi - e)[k])
        batches.append((j, pieces))
    pieces = np.concatenate([b[1].reshape(-1) for b in batches])
    k_max = np.concatenate([limit[site[b[0]]] for b in batches]).astype(np.uint32)
    dist = np.asarray(ctx.haplotype_distance_batch_mixed(pool, pieces, k_max), dtype=np.uint32)
    n_ref_jobs = len(batches[0][0])
    dr, da = np.full(len(site), MORE, np.uint32), np.full(len(site), MORE, np.uint32)
    dr[batches[0][0]] = dist[:n_ref_jobs]
    da[batches[1][0]] = dist[n_ref_jobs:]
    # ---- the call (distances are uint32 with MORE above every limit)
    lim = limit[site]
    within_r, within_a = dr.astype(np.int64) <= lim, da.astype(np.int64) <= lim
    dr, da = np.where(within_r, dr, MORE).astype(np.uint32), np.where(within_a, da, MORE).astype(np.uint32)
    c = np.full(len(site), OTHER_ALLELE, np.uint8)
    c[within_a & (da < dr)] = CALL_ALT
    c[within_r & (dr < da)] = CALL_REF
    c[within_r & within_a & (dr == da)] = AMBIGUOUS
    call[hap, site], d_ref[hap, site], d_alt[hap, site] = c, dr, da
    _clock(timing, "distances", t0)
    return call, d_ref, d_alt


def _distance_text(d):
    return np.array([b"." if x == MORE else b"%d" % x for x in d.tolist()], dtype=object)


def write_vcf(path, sites, rows, call, d_ref, d_alt, sample):
    """SITES' ## lines verbatim, the FORMAT lines of GT, DR and DA (a GT line SITES has is not repeated), a #CHROM line
    with one sample column, every genotyped record's first eight columns verbatim and GT:DR:DA.  Written under a
    temporary name and renamed."""
    header = [l for l in sites.header.split(b"\n") if l.startswith(b"##")]
    has_gt = any(l.startswith(b"##FORMAT=<ID=GT,") for l in header)
    gt = [b"/".join(col) for col in CALL_TEXT[call].T.tolist()] if len(rows) else []
    dr = [b",".join(col) for col in np.stack([_distance_text(d) for d in d_ref]).T.tolist()] if len(rows) else []
    da = [b",".join(col) for col in np.stack([_distance_text(d) for d in d_alt]).T.tolist()] if len(rows) else []
    with open(path + ".tmp", "wb") as fh:
        for line in header:
            fh.write(line.rstrip(b"\r") + b"\n")
        for line in FORMAT_LINES[1 if has_gt else 0:]:
            fh.write(line + b"\n")
        fh.write(b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample.encode("utf-8", "surrogateescape") + b"\n")
        for i, r in enumerate(rows.tolist()):
            fh.write(b"\t".join(sites.lines[r].split(b"\t", 8)[:8]) + b"\tGT:DR:DA\t" + gt[i] + b":" + dr[i] + b":" + da[i] + b"\n")
    os.replace(path + ".tmp", path)


def genotype(sites_path, reference, aln_files, options, out_dir, ctx=None, timing=None):
    """The whole command: writes genotypes.vcf and summary.json into out_dir and returns the summary.  Raises
    vcfin.VcfFormatError / ValueError for inputs that cannot be used.  aln_files: one opened alignment file per haplotype."""
    t0 = time.perf_counter()
    contigs, lengths = list(reference.references), list(reference.lengths)
    sites = vcfin.read_sites(sites_path, contigs, lengths, passonly=options.passonly)
    t = sites.table
    size = np.where(t.type == T_INS, t.q_len, t.se - t.ss).astype(np.int64)
    rows = np.flatnonzero(size >= int(options.min_sv_size))
    t0 = _clock(timing, "read", t0)
    SVIM_COLLECT._load_together(aln_files)
    samples = [SVIM_COLLECT._prepare(f, options) for f in aln_files]
    ctx = ctx or _lib.default_context(getattr(options, "device", 0) or 0)
    _clock(timing, "load", t0)
    logging.info("Genotyping %d of %d records in %d haplotype(s)...", len(rows), sites.n_lines, len(samples))
    call, d_ref, d_alt = genotype_sites(t, rows, reference, samples, options, ctx, timing=timing)
    for s in samples:
        SVIM_COLLECT._verify_pending(s)  # (a haplotype without a slice call: nothing is written on unchecked members)
    t0 = time.perf_counter()
    summary = {"records": int(sites.n_lines), "genotyped": int(len(rows)), "size_filtered": int(len(t) - len(rows)),
               "not_genotyped": {k: int(sites.counts[k]) for k in _NOT_GENOTYPED},
               "haplotypes": [{name: int((call[h] == code).sum()) for code, name in enumerate(CALL_NAMES)} for h in range(len(samples))]}
    os.makedirs(out_dir, exist_ok=True)
    write_vcf(os.path.join(out_dir, "genotypes.vcf"), sites, rows, call, d_ref, d_alt, getattr(options, "sample", None) or "Sample")
    with open(os.path.join(out_dir, "summary.json"), "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    _clock(timing, "write", t0)
    return summary
