"""SNVs and small indels from assembly alignments (svim-asm-small).

Per haplotype, over the records COLLECT visits that store their bases and hold no N op:
  * mismatches: the aligned columns are compared with the reference on the device — per batch of at most --batch_bases
    pool bytes ONE sequence_slices call (every record's whole SEQ), ONE _fetch_windows call (every record's reference
    interval) and ONE svx_cigar_mismatch over the CIGAR pool of the whole file, records outside the batch with both
    lengths 0;
  * indels: ONE svx_cigar_extract with min_len 1; the ops shorter than --min_sv_size are kept (the longer ones are
    svim-asm's); with --left_align ONE svx_indel_shift per batch, on the batch's pool of bases, moves each of them as far
    to the left as its bases allow without passing another gap;
  * alleles, upper case and where the aligner put them — nothing is left-aligned unless --left_align, and nothing is
    normalised beyond that: SNV (POS = ref_pos + 1),
    INS and DEL anchored on the base in front (POS = ref_pos); an indel at its alignment's first reference position
    (no_anchor) and an allele with a base outside ACGT (ambiguous_base) are dropped and counted;
  * an event is kept only when its REF span lies inside ONE single-coverage segment of its haplotype
    (SVIM_CALLABLE.single_segments, all haplotypes in one svx_cover_single); the others are counted as multiply_covered.
The records are the distinct (contig, POS, REF, ALT) of all haplotypes in genome order; a haplotype's allele is 1 where it
carries the record, 0 where the record's span lies inside one of its single-coverage segments and none of its kept events
overlaps it, `.` otherwise; GT is phased (h1|h2), haploid with one input.  Everything past the device calls works on
columns: no Python loop per record."""
import json
import logging
import os

import numpy as np

from svim_asm_amd import SVIM_CALLABLE, SVIM_COLLECT, SVIM_COMBINE as _combine, SVIM_GENOTYPE, _lib

DROPS = ("no_anchor", "ambiguous_base", "multiply_covered")
KINDS = ("SNV", "INS", "DEL")
FORMAT_LINE = b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">'
_GT_TEXT = np.array([b"0", b"1", b"."])
_MASK32 = np.uint64(0xFFFFFFFF)


def _upper(b):
    b = np.asarray(b, dtype=np.uint8)
    return np.where((b >= 97) & (b <= 122), b - 32, b).astype(np.uint8)


def _is_acgt(b):
    return (b == 65) | (b == 67) | (b == 71) | (b == 84)


def _all_acgt(pool, off):
    """Per slice pool[off[i]:off[i + 1]] (none empty): every byte one of ACGT."""
    bad = np.concatenate(([0], np.cumsum(~_is_acgt(pool))))
    return bad[off[1:]] == bad[off[:-1]]


def _strings(pool, start, length, width):
    """The slices pool[start[i] : start[i] + length[i]] as a fixed-width bytes column."""
    n = len(start)
    out = np.zeros((n, width), np.uint8)
    if n and int(length.sum()):
        row = np.repeat(np.arange(n), length)
        col = np.arange(int(length.sum())) - np.repeat(np.cumsum(length) - length, length)
        out[row, col] = pool[np.repeat(start, length) + col]
    return out.view("S%d" % width).reshape(n)


class _Events(object):
    """One haplotype's events as columns: genome contig, POS (1-based), REF, ALT (bytes columns), kind (index into KINDS)."""

    def __init__(self, g, pos, ref, alt, kind):
        self.g, self.pos, self.ref, self.alt, self.kind = g, pos, ref, alt, kind

    def __len__(self):
        return len(self.g)

    def take(self, keep):
        return _Events(self.g[keep], self.pos[keep], self.ref[keep], self.alt[keep], self.kind[keep])

    def span(self):
        lo = (self.g.astype(np.uint64) << np.uint64(32)) | (self.pos - 1).astype(np.uint64)
        return lo, lo + np.char.str_len(self.ref).astype(np.uint64)


def _inside_one(segments, lo, hi):
    """Which spans [lo, hi) lie inside ONE of the sorted, disjoint segments."""
    seg_lo, seg_hi = segments
    if len(seg_lo) == 0:
        return np.zeros(len(lo), bool)
    k = np.searchsorted(seg_lo, lo, side="right").astype(np.int64) - 1
    return (k >= 0) & (hi <= seg_hi[np.maximum(k, 0)])


def _device_pool(r):
    base = getattr(r, "base", None)
    return base.device_pool(wait=True) if base is not None and hasattr(base, "device_pool") and r.cigar is base._cigar else None


def _batches(cost, limit):
    """Consecutive runs of records whose summed cost stays within `limit` (a record above it is a batch of its own)."""
    out, first, total = [], 0, 0
    for k, c in enumerate(cost.tolist()):
        if k > first and total + c > limit:
            out.append((first, k))
            first, total = k, 0
        total += c
    if len(cost) > first:
        out.append((first, len(cost)))
    return out


def _haplotype_events(s, hap_list, reference, contigs, options, ctx, counts):
    """The events of one haplotype before the coverage filter; fills `counts`."""
    r = s.rec
    n = len(r.tid)
    width = int(options.min_sv_size) + 1
    order = np.asarray(s.order, dtype=np.int64)
    l_seq = np.asarray(r.l_seq, dtype=np.int64)
    cig_off = np.asarray(r.cig_off, dtype=np.int64)
    cigar = np.asarray(r.cigar, dtype=np.uint32)
    spliced = np.zeros(n, bool)
    at = np.flatnonzero((cigar[:int(cig_off[-1])] & 15) == 3)
    spliced[np.searchsorted(cig_off, at, side="right") - 1] = True
    no_seq = l_seq[order] == 0
    counts["no_sequence"] = int(no_seq.sum())
    counts["spliced"] = int((spliced[order] & ~no_seq).sum())
    used = order[~no_seq & ~spliced[order]]
    counts["records_used"] = int(len(used))
    # every record's contig and reference interval, from the haplotype's coverage list
    lo_key, hi_key, rec = hap_list
    g_of, start_of, end_of = np.full(n, -1, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    g_of[rec] = (lo_key >> np.uint64(32)).astype(np.int64)
    start_of[rec] = (lo_key & _MASK32).astype(np.int64)
    end_of[rec] = (hi_key & _MASK32).astype(np.int64)
    used = used[g_of[used] >= 0]  # (a record without reference bases has neither columns nor indels)
    pos = np.maximum(np.asarray(r.pos, dtype=np.int64), 0).astype(np.int32)  # (unplaced records: both lengths 0)
    pool = _device_pool(r)
    # ---- indel rows: every I and D op where the aligner put it
    n_ops = np.diff(cig_off)[used]
    sub_off = np.zeros(len(used) + 1, np.uint64)
    np.cumsum(n_ops, out=sub_off[1:])
    total = int(sub_off[-1])
    words = cigar[np.repeat(cig_off[used], n_ops) + np.arange(total) - np.repeat(sub_off[:-1].astype(np.int64), n_ops)] if total else cigar[:0]
    sig = ctx.cigar_extract(words, sub_off, pos[used], min_len=1) if len(used) else None
    if sig is None:
        sig = {k: np.zeros(0, np.int64) for k in ("aln", "ref_pos", "read_pos", "len", "type")}
    s_aln, s_pos, s_len = (np.asarray(sig[k], dtype=np.int64) for k in ("aln", "ref_pos", "len"))
    s_ins = np.asarray(sig["type"]) == 0  # SVX_SIG_INS
    small = s_len < int(options.min_sv_size)
    i_sub = s_aln[small]  # (ascending: the rows come in (alignment, op) order)
    i_rec = used[i_sub]
    i_pos = s_pos[small]
    i_qry = np.asarray(sig["read_pos"], dtype=np.int64)[small]
    i_len = s_len[small]
    i_ins = s_ins[small]
    left_align = bool(getattr(options, "left_align", False))
    if left_align:
        # the most steps of a row: up to the column behind the gap in front of it (large ones included) or behind its
        # alignment's start, in the original placement — a gap never passes another one and keeps one aligned column
        prev_end = pos[used[s_aln]].astype(np.int64)
        same = s_aln[1:] == s_aln[:-1]
        prev_end[1:][same] = (s_pos + np.where(s_ins, 0, s_len))[:-1][same]
        i_limit = np.maximum(0, s_pos - prev_end - 1)[small]
        i_shift = np.zeros(len(i_rec), np.int64)
    # ---- mismatches, and with --left_align the small rows' shifts on the same pool of bases
    parts = []
    for first, last in _batches((end_of - start_of + l_seq)[used], int(options.batch_bases)):
        b = used[first:last]
        seq, seq_off = r.sequence_slices(b, np.zeros(len(b), np.int64), l_seq[b])
        win, win_off = _combine._fetch_windows(reference, contigs, g_of[b], start_of[b], end_of[b], False)
        seq_off, win_off = np.asarray(seq_off, dtype=np.int64), np.asarray(win_off, dtype=np.int64)
        if not np.array_equal(win_off[1:] - win_off[:-1], end_of[b] - start_of[b]):
            raise ValueError("reference windows shorter than the index says")
        ref_off, ref_len, qry_off, qry_len = (np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint32))
        ref_off[b], ref_len[b] = win_off[:-1], win_off[1:] - win_off[:-1]
        qry_off[b], qry_len[b] = len(win) + seq_off[:-1], seq_off[1:] - seq_off[:-1]
        bases = np.concatenate((np.asarray(win, dtype=np.uint8), np.asarray(seq, dtype=np.uint8)))
        if pool is not None:
            ev = ctx.cigar_mismatch(pool[0], cig_off, pos, bases, ref_off, ref_len, qry_off, qry_len, n_ops=int(cig_off[-1]))
        else:
            ev = ctx.cigar_mismatch(cigar, cig_off, pos, bases, ref_off, ref_len, qry_off, qry_len)
        parts.append(ev)
        if left_align:
            lo, hi = (int(x) for x in np.searchsorted(i_sub, (first, last)))
            if hi > lo:
                i_shift[lo:hi] = ctx.indel_shift(bases, ref_off, ref_len, qry_off, qry_len, pos, i_rec[lo:hi], i_pos[lo:hi], i_qry[lo:hi],
                                                 i_len[lo:hi], np.where(i_ins[lo:hi], 0, 1), i_limit[lo:hi])
    cat = lambda key, dtype: np.concatenate([np.asarray(p[key], dtype=dtype) for p in parts]) if parts else np.zeros(0, dtype)
    m_aln = cat("aln", np.int64)
    counts["mismatches"] = int(len(m_aln))
    snv = _Events(g_of[m_aln], cat("ref_pos", np.int64) + 1, cat("ref_base", np.uint8).view("S1").astype("S%d" % width),
                  cat("qry_base", np.uint8).view("S1").astype("S%d" % width), np.zeros(len(m_aln), np.int8))
    # ---- indels
    counts["small_indels"] = int(len(i_rec))
    if left_align:
        i_pos, i_qry = i_pos - i_shift, i_qry - i_shift
        counts["left_aligned"] = int((i_shift > 0).sum())
        counts["shifted_bases"] = int(i_shift.sum())
    anchored = i_pos > start_of[i_rec]
    counts["no_anchor"] = int((~anchored).sum())
    i_rec, i_pos, i_qry, i_len, i_ins = i_rec[anchored], i_pos[anchored], i_qry[anchored], i_len[anchored], i_ins[anchored]
    k = len(i_rec)
    # REF: the anchor, for a deletion with the deleted bases; ALT: the anchor, for an insertion with the inserted bases
    ref_n = np.where(i_ins, 1, 1 + i_len)
    win, win_off = _combine._fetch_windows(reference, contigs, g_of[i_rec], i_pos - 1, i_pos - 1 + ref_n, True) if k else (np.zeros(0, np.uint8), np.zeros(1, np.int64))
    win, win_off = _upper(win), np.asarray(win_off, dtype=np.int64)
    if k and not np.array_equal(win_off[1:] - win_off[:-1], ref_n):
        raise ValueError("reference windows shorter than the index says")
    ins = np.flatnonzero(i_ins)
    seq, seq_off = r.sequence_slices(i_rec[ins], i_qry[ins], i_qry[ins] + i_len[ins]) if len(ins) else (np.zeros(0, np.uint8), np.zeros(1, np.int64))
    seq, seq_off = _upper(seq), np.asarray(seq_off, dtype=np.int64)
    if len(ins) and not np.array_equal(seq_off[1:] - seq_off[:-1], i_len[ins]):
        raise ValueError("an insertion's bases lie behind its record's sequence")
    good = _all_acgt(win, win_off) if k else np.zeros(0, bool)
    if len(ins):
        good[ins] &= _all_acgt(seq, seq_off)
    counts["ambiguous_base"] = int((~good).sum())
    ref = _strings(win, win_off[:-1], ref_n, width)
    alt = _strings(win, win_off[:-1], np.ones(k, np.int64), width)
    if len(ins):
        alt[ins] = np.char.add(alt[ins], _strings(seq, seq_off[:-1], i_len[ins], width)).astype("S%d" % width)
    indel = _Events(g_of[i_rec], i_pos, ref, alt, np.where(i_ins, 1, 2).astype(np.int8)).take(good)
    return _Events(*(np.concatenate((getattr(snv, f), getattr(indel, f))) for f in ("g", "pos", "ref", "alt", "kind")))


def call_small(reference, samples, options, ctx):
    """(records as _Events in output order, genotype codes [n_hap, n_records] (0, 1, 2 for `.`), per-haplotype counts)."""
    contigs = list(reference.references)
    lists = SVIM_GENOTYPE._haplotype_lists(samples, contigs, ctx)
    segments = SVIM_CALLABLE.single_segments([((lo >> np.uint64(32)).astype(np.int64), (lo & _MASK32).astype(np.int64), (hi & _MASK32).astype(np.int64))
                                              for lo, hi, _rec in lists], ctx)
    counts, kept = [], []
    for h, s in enumerate(samples):
        c = {}
        ev = _haplotype_events(s, lists[h], reference, contigs, options, ctx, c)
        SVIM_COLLECT._verify_pending(s)
        inside = _inside_one(segments[h], *ev.span())
        c["multiply_covered"] = int((~inside).sum())
        kept.append(ev.take(inside))
        counts.append(c)
    # ---- the distinct keys, in genome order
    g, pos, ref, alt, kind = (np.concatenate([getattr(e, f) for e in kept]) for f in ("g", "pos", "ref", "alt", "kind"))
    hap = np.concatenate([np.full(len(e), h, np.int64) for h, e in enumerate(kept)])
    o = np.lexsort((alt, ref, pos, g))
    g, pos, ref, alt, kind, hap = g[o], pos[o], ref[o], alt[o], kind[o], hap[o]
    new = np.ones(len(g), bool)
    new[1:] = (g[1:] != g[:-1]) | (pos[1:] != pos[:-1]) | (ref[1:] != ref[:-1]) | (alt[1:] != alt[:-1])
    first = np.flatnonzero(new)
    records = _Events(g[first], pos[first], ref[first], alt[first], kind[first])
    row = np.cumsum(new) - 1
    gt = np.full((len(samples), len(records)), 2, np.int8)
    lo, hi = records.span()
    for h, e in enumerate(kept):
        e_lo, e_hi = e.span()
        e_lo, e_hi = np.sort(e_lo), np.sort(e_hi)
        touched = np.searchsorted(e_lo, hi, side="left") > np.searchsorted(e_hi, lo, side="right")  # an event with lo < hi' and hi > lo'
        gt[h, _inside_one(segments[h], lo, hi) & ~touched] = 0
        gt[h, row[hap == h]] = 1
    return records, gt, counts


def vcf_text(reference, records, gt, sample):
    """small.vcf as bytes: the header, then one line per record, built column by column."""
    contigs, lengths = list(reference.references), list(reference.lengths)
    head = [b"##fileformat=VCFv4.2"] + [("##contig=<ID=%s,length=%d>" % (c, n)).encode("utf-8", "surrogateescape") for c, n in zip(contigs, lengths)]
    head += [FORMAT_LINE, b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample.encode("utf-8", "surrogateescape")]
    text = b"".join(l + b"\n" for l in head)
    if len(records) == 0:
        return text
    names = np.array([c.encode("utf-8", "surrogateescape") for c in contigs])
    calls = _GT_TEXT[gt[0]]
    for h in range(1, len(gt)):
        calls = np.char.add(np.char.add(calls, b"|"), _GT_TEXT[gt[h]])
    add = np.char.add
    line = add(add(names[records.g], b"\t"), records.pos.astype("S"))
    line = add(add(add(add(line, b"\t.\t"), records.ref), b"\t"), records.alt)
    line = add(add(add(line, b"\t.\tPASS\t.\tGT\t"), calls), b"\n")
    return text + b"".join(line.tolist())


def summarise(records, gt, counts):
    calls = _GT_TEXT[gt[0]]
    for h in range(1, len(gt)):
        calls = np.char.add(np.char.add(calls, b"|"), _GT_TEXT[gt[h]])
    texts, n = np.unique(calls, return_counts=True) if len(records) else ([], [])
    order = ("records_used", "no_sequence", "spliced", "mismatches", "small_indels") + DROPS
    order += tuple(k for k in ("left_aligned", "shifted_bases") if counts and k in counts[0])  # (--left_align)
    return {"haplotypes": [{k: int(c[k]) for k in order} for c in counts], "records": int(len(records)),
            "by_type": {name: int((records.kind == k).sum()) for k, name in enumerate(KINDS)},
            "by_genotype": {t.decode(): int(k) for t, k in zip(texts, n)}}


def small(reference, aln_files, options, out_dir, ctx=None):
    """The whole command: writes small.vcf (small.vcf.gz and its index with --bgzip_output) and summary.json into out_dir
    and returns the summary.  Raises ValueError for inputs that cannot be used."""
    SVIM_COLLECT._load_together(aln_files)
    samples = [SVIM_COLLECT._prepare(f, options) for f in aln_files]
    ctx = ctx or _lib.default_context(getattr(options, "device", 0) or 0)
    records, gt, counts = call_small(reference, samples, options, ctx)
    for s in samples:
        SVIM_COLLECT._verify_pending(s)  # (nothing is written on unchecked members)
    summary = summarise(records, gt, counts)
    logging.info("%d records from %d haplotype(s)", len(records), len(samples))
    text = vcf_text(reference, records, gt, getattr(options, "sample", None) or "Sample")
    os.makedirs(out_dir, exist_ok=True)
    if getattr(options, "bgzip_output", False):
        from svim_asm_amd import vcf_bgzf
        path = os.path.join(out_dir, "small.vcf.gz")
        vcf_bgzf.write(path, text, ctx if vcf_bgzf.device_path_wanted() else None)  # (leaves nothing behind when it fails)
    else:
        path = os.path.join(out_dir, "small.vcf")
        with open(path + ".tmp", "wb") as fh:
            fh.write(text)
        os.replace(path + ".tmp", path)
    with open(os.path.join(out_dir, "summary.json"), "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    return summary
