"""Score small-variant calls against a truth VCF by haplotype replay (svim-asm-small-compare).

BASE is the truth, COMP the calls under test.  Both files are read as edits (vcfin.read_alleles).  A record is compared
when it is smaller than --max_size, its REF column equals the genome (ONE fetch per file) and, with --include_bed, it
lies inside ONE line of the BED (svx_cover_query).  Records with the same (contig, start, ref_len, alt bytes) in both
files are exact twins (the first of equal keys inside one file; the others are `duplicate`: compared, never TP, and kept
out of the replay, where they could only collide with their first).  The compared records of both files, sorted by
(contig, start), are cut into clusters wherever a record begins more than --cluster_distance behind the largest end so
far; a cluster with a record that has no twin is replayed on the device: its window [smallest start, largest end) with
each side's edits, per haplotype when every record of the cluster is phased (four jobs, four pairs, the orientation
with more equal pairs, straight on a tie), else all of a side's records at once (two jobs, one pair); an insertion and
the edit that begins where it stands go down as one edit.  ONE
_fetch_windows and ONE svx_variant_replay per batch of at most --batch_bases pool bytes, whole clusters per batch.  A
record is TP iff it has a twin or every haplotype it is carried on (both, where the file has no genotype) agrees.
Everything works on columns: no Python loop per record."""
import json
import logging
import os

import numpy as np

from svim_asm_amd import SVIM_COMBINE as _combine, SVIM_COMPARE, SVIM_SMALL, _lib, vcfin

TYPES = ("SNV", "INS", "DEL", "COMPLEX")
_NOT_READ = ("multiallelic", "symbolic_or_other", "not_carried", "filtered", "no_change")
_POP = np.array([0, 1, 1, 2])
DEFAULT_BATCH_BASES = 1 << 28


class _Side(object):
    """One file's compared records as columns (rows: indices into the reader's rows)."""


def _flat(pool, start, length):
    """pool[start[i] : start[i] + length[i]] for all i, one behind the other."""
    total = int(length.sum())
    if not total:
        return np.zeros(0, np.uint8)
    col = np.arange(total) - np.repeat(np.cumsum(length) - length, length)
    return pool[np.repeat(start, length) + col]


def _select(a, reference, contigs, options, bed, ctx):
    """The compared rows of one file and the counts of the ones that are not."""
    n = len(a)
    ref_len, alt_len = a.ref_len.astype(np.int64), a.alt_len.astype(np.int64)
    small = np.maximum(ref_len, alt_len) < int(options.max_size)
    # the REF column against the genome: one fetch for the whole file
    text_len = a.ref_text_len.astype(np.int64)
    win, win_off = _combine._fetch_windows(reference, contigs, a.contig, a.pos, a.pos + text_len, True) if n else (np.zeros(0, np.uint8), np.zeros(1, np.int64))
    win, win_off = np.asarray(win, dtype=np.uint8), np.asarray(win_off, dtype=np.int64)
    if n and not np.array_equal(win_off[1:] - win_off[:-1], text_len):
        raise ValueError("reference windows shorter than the index says")
    written = SVIM_SMALL._upper(_flat(np.frombuffer(a.text, np.uint8), a.ref_off.astype(np.int64), text_len))
    bad = np.concatenate(([0], np.cumsum(written != SVIM_SMALL._upper(win))))
    matches = bad[win_off[1:]] == bad[win_off[:-1]] if n else np.zeros(0, bool)
    inside = np.ones(n, bool)
    if bed is not None and len(bed[0]) == 0:
        inside[:] = False
    elif bed is not None and n:
        contig = a.contig.astype(np.uint64) << np.uint64(32)
        q_lo = contig | a.start.astype(np.uint64)
        inside = ctx.cover_query(bed[0], bed[1], np.array([0, len(bed[0])], np.uint64), q_lo, q_lo + a.ref_len.astype(np.uint64))[0].astype(bool)
    keep = small & matches & inside
    counts = {"too_large": int((~small).sum()), "ref_mismatch": int((small & ~matches).sum()), "out_of_regions": int((small & matches & ~inside).sum())}
    s = _Side()
    s.rows = np.flatnonzero(keep)
    s.contig, s.start, s.ref_len, s.alt_len = a.contig[s.rows].astype(np.int64), a.start[s.rows], ref_len[s.rows], alt_len[s.rows]
    s.alt_off = a.alt_off[s.rows].astype(np.int64)
    s.gt, s.phased = a.gt[s.rows], a.phased[s.rows].astype(bool)
    s.bits = np.where(s.gt == 0, 3, s.gt).astype(np.int64)  # (no genotype in the file: carried on both haplotypes)
    s.kind = np.where((s.ref_len == 1) & (s.alt_len == 1), 0, np.where(s.ref_len == 0, 1, np.where(s.alt_len == 0, 2, 3)))
    width = max(1, int(options.max_size))
    key = np.zeros(len(s.rows), np.dtype([("contig", "<i8"), ("start", "<i8"), ("ref_len", "<i8"), ("alt", "S%d" % width)]))
    key["contig"], key["start"], key["ref_len"] = s.contig, s.start, s.ref_len
    key["alt"] = SVIM_SMALL._strings(a.alts, s.alt_off, s.alt_len, width)
    s.key = key
    return s, counts


def _twins(b, c):
    """Per side: the twin's index on the other side or -1, and which records repeat an earlier key of their own file."""
    out = []
    firsts = []
    for s in (b, c):
        _, first, inv = np.unique(s.key, return_index=True, return_inverse=True)
        dup = np.ones(len(s.key), bool)
        dup[first] = False
        firsts.append(np.flatnonzero(~dup))
        out.append(dup)
    fb, fc = firsts
    both = np.concatenate((b.key[fb], c.key[fc]))
    _, inv, n = np.unique(both, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).ravel()
    shared = n[inv] == 2
    twin_b, twin_c = np.full(len(b.key), -1, np.int64), np.full(len(c.key), -1, np.int64)
    slot = np.full(len(n), -1, np.int64)
    slot[inv[:len(fb)]] = fb
    hit = np.flatnonzero(shared[len(fb):])
    twin_c[fc[hit]] = slot[inv[len(fb):][hit]]
    twin_b[twin_c[fc[hit]]] = fc[hit]
    return twin_b, twin_c, out[0], out[1]


def _replay(R, reference, contigs, options, ctx, alts):
    """The replayed clusters' jobs, batch by batch.  R: columns of the clustered records in sorted order (side, contig, start,
    ref_len, alt_off, alt_len, bits, cluster index among the replayed ones), the clusters' (contig, lo, hi, phased).
    Returns (status [clusters, 4], equal [clusters, 4]); a union cluster uses jobs 0 (base) and 2 (comp) and pair 0."""
    n_cl = len(R["c_lo"])
    status, equal = np.zeros((n_cl, 4), np.uint8), np.zeros((n_cl, 4), np.uint8)
    rec_first = np.searchsorted(R["cluster"], np.arange(n_cl + 1))
    cost = (R["c_hi"] - R["c_lo"]) + np.add.reduceat(R["alt_len"], rec_first[:-1]) if n_cl else np.zeros(0, np.int64)
    for first, last in SVIM_SMALL._batches(cost, int(options.batch_bases)):
        k = last - first
        lo, hi = rec_first[first], rec_first[last]
        win, win_off = _combine._fetch_windows(reference, contigs, R["c_contig"][first:last], R["c_lo"][first:last], R["c_hi"][first:last], True)
        win, win_off = SVIM_SMALL._upper(win), np.asarray(win_off, dtype=np.int64)
        if not np.array_equal(win_off[1:] - win_off[:-1], (R["c_hi"] - R["c_lo"])[first:last]):
            raise ValueError("reference windows shorter than the index says")
        side, cl, bits = R["side"][lo:hi], R["cluster"][lo:hi] - first, R["bits"][lo:hi]
        alt_len = R["alt_len"][lo:hi]
        alt_pool = np.concatenate([_flat(alts[s], np.where(side == s, R["alt_off"][lo:hi], 0), np.where(side == s, alt_len, 0)) for s in (0, 1)])
        # where each record's bytes went: side 0's records first, then side 1's, each in order
        by_side = np.argsort(side, kind="stable")
        alt_at = np.zeros(hi - lo, np.int64)
        alt_at[by_side] = len(win) + np.cumsum(alt_len[by_side]) - alt_len[by_side]
        phased = R["c_phased"][first:last]
        # one edit per (record, job): job 2 * side + h for a phased cluster's haplotype h, job 2 * side in a union cluster
        idx = np.arange(hi - lo)
        ph = phased[cl]
        e_rec = np.concatenate((idx[~ph], idx[ph & (bits & 1 > 0)], idx[ph & (bits & 2 > 0)]))
        e_hap = np.concatenate((np.zeros(int((~ph).sum()), np.int64), np.zeros(int((ph & (bits & 1 > 0)).sum()), np.int64),
                                np.ones(int((ph & (bits & 2 > 0)).sum()), np.int64)))
        e_job = cl[e_rec] * 4 + side[e_rec] * 2 + e_hap
        o = np.lexsort((e_rec, e_job))  # (records are in (contig, start) order, file order at equal starts)
        e_rec, e_job = e_rec[o], e_job[o]
        pool = np.concatenate((win, alt_pool))
        e_start, e_ref = (R["start"][lo:hi] - R["c_lo"][R["cluster"][lo:hi]])[e_rec], R["ref_len"][lo:hi][e_rec]
        e_at, e_len = alt_at[e_rec], alt_len[e_rec]
        # an insertion and the edit that begins where it stands (`..I D..` and a mismatching column behind an insertion are
        # two records of svim-asm-small with ONE start) are one edit: the inserted bases, then the other's.  Two insertions
        # at one start stay two edits, and out of order.
        join = np.zeros(len(e_rec), bool)
        join[1:] = (e_job[1:] == e_job[:-1]) & (e_start[1:] == e_start[:-1]) & (e_ref[:-1] == 0) & (e_ref[1:] > 0)
        if join.any():
            second = np.flatnonzero(join)
            pool = np.concatenate((pool, _flat(pool, e_at, e_len)))  # every edit's bytes once more, edit by edit: the two lie one behind the other
            e_at = len(pool) - int(e_len.sum()) + np.cumsum(e_len) - e_len
            e_at[second], e_len = e_at[second - 1], e_len.copy()
            e_len[second] += e_len[second - 1]
            keep = np.ones(len(e_rec), bool)
            keep[second - 1] = False
            e_job, e_start, e_ref, e_at, e_len = e_job[keep], e_start[keep], e_ref[keep], e_at[keep], e_len[keep]
        ed_first = np.zeros(4 * k + 1, np.int64)
        np.cumsum(np.bincount(e_job, minlength=4 * k), out=ed_first[1:])
        pa = np.tile(np.array([0, 1, 0, 1]), k) + np.repeat(np.arange(k) * 4, 4)
        pb = np.tile(np.array([2, 3, 3, 2]), k) + np.repeat(np.arange(k) * 4, 4)
        res = ctx.variant_replay(pool, np.repeat(win_off[:-1], 4), np.repeat(win_off[1:] - win_off[:-1], 4), ed_first, e_start, e_ref, e_at, e_len, pa, pb)
        status[first:last] = np.asarray(res["status"]).reshape(k, 4)
        equal[first:last] = np.asarray(res["equal"]).reshape(k, 4)
    if (status == 2).any():
        raise RuntimeError("svx_variant_replay: an edit outside its cluster's window")
    return status, equal


def _write(path, data):
    with open(path + ".tmp", "wb") as fh:
        fh.write(data)
    os.replace(path + ".tmp", path)


def _vcf(a, rows):
    head = a.header if not a.header or a.header.endswith(b"\n") else a.header + b"\n"
    return head + b"".join(a.line(i) + b"\n" for i in rows)


def compare(base_path, comp_path, reference, options, out_dir, ctx=None):
    """The whole comparison; writes summary.json, tp-base.vcf, fn.vcf, tp-comp.vcf, fp.vcf and clusters.tsv into out_dir and
    returns the summary.  Raises vcfin.VcfFormatError / ValueError for inputs that cannot be used."""
    contigs, lengths = list(reference.references), list(reference.lengths)
    files = [vcfin.read_alleles(base_path, contigs, lengths, sample=getattr(options, "base_sample", None), passonly=options.passonly),
             vcfin.read_alleles(comp_path, contigs, lengths, sample=getattr(options, "comp_sample", None), passonly=options.passonly)]
    bed = SVIM_COMPARE.read_bed(options.include_bed, contigs) if getattr(options, "include_bed", None) else None
    ctx = ctx or _lib.default_context(getattr(options, "device", 0) or 0)
    sides, skipped = zip(*[_select(a, reference, contigs, options, bed, ctx) for a in files])
    b, c = sides
    logging.info("Comparing %d of %d base records with %d of %d comp records...", len(b.rows), files[0].n_lines, len(c.rows), files[1].n_lines)
    twin_b, twin_c, dup_b, dup_c = _twins(b, c)
    twin, dup = (twin_b, twin_c), (dup_b, dup_c)
    # ---- clusters over the records of both files that are not duplicates: base in front at equal (contig, start)
    use = [np.flatnonzero(~d) for d in dup]
    side = np.concatenate([np.full(len(u), s, np.int64) for s, u in enumerate(use)])
    own = np.concatenate(use)
    col = lambda f: np.concatenate([getattr(s, f)[u] for s, u in zip(sides, use)])
    contig, start, ref_len = col("contig"), col("start"), col("ref_len")
    o = np.lexsort((start, contig))
    side, own, contig, start, ref_len = side[o], own[o], contig[o], start[o], ref_len[o]
    alt_off, alt_len, bits, phased = col("alt_off")[o], col("alt_len")[o], col("bits")[o], col("phased")[o]
    has_twin = np.concatenate([t[u] >= 0 for t, u in zip(twin, use)])[o]
    n = len(o)
    new = np.ones(n, bool)
    if n > 1:
        # the largest end so far, a contig's records above every earlier contig's: a new contig always opens a cluster
        reach = np.maximum.accumulate((contig << 40) + start + ref_len)[:-1]
        new[1:] = (contig[1:] << 40) + start[1:] > reach + int(options.cluster_distance)
    cl = np.cumsum(new) - 1
    n_cl = int(cl[-1]) + 1 if n else 0
    first = np.flatnonzero(new)
    size = np.diff(np.concatenate((first, [n])))
    c_lo = start[first]
    c_hi = np.maximum.reduceat(start + ref_len, first) if n else np.zeros(0, np.int64)
    over = size > int(options.max_cluster)
    if over.any():
        logging.warning("%d cluster(s) of more than --max_cluster %d records are not replayed: exact twins only", int(over.sum()), int(options.max_cluster))
    open_ = np.add.reduceat((~has_twin).astype(np.int64), first) > 0 if n else np.zeros(0, bool)
    replayed = np.flatnonzero(open_ & ~over)
    c_phased = np.add.reduceat((~phased).astype(np.int64), first) == 0 if n else np.zeros(0, bool)
    r_index = np.full(n_cl, -1, np.int64)
    r_index[replayed] = np.arange(len(replayed))
    in_r = r_index[cl] >= 0 if n else np.zeros(0, bool)
    R = {"side": side[in_r], "start": start[in_r], "ref_len": ref_len[in_r], "alt_off": alt_off[in_r], "alt_len": alt_len[in_r], "bits": bits[in_r],
         "cluster": r_index[cl][in_r] if n else np.zeros(0, np.int64), "c_contig": contig[first][replayed] if n else np.zeros(0, np.int64),
         "c_lo": c_lo[replayed], "c_hi": c_hi[replayed], "c_phased": c_phased[replayed]}
    status, equal = _replay(R, reference, contigs, options, ctx, [f.alts for f in files])
    # ---- the orientation, and which job agrees
    ph = R["c_phased"]
    swapped = ph & (equal[:, 2].astype(int) + equal[:, 3] > equal[:, 0].astype(int) + equal[:, 1])
    agree = np.zeros((len(replayed), 4), bool)  # job 2 * side + h
    eq = equal.astype(bool)
    agree[:, 0] = np.where(swapped, eq[:, 2], eq[:, 0])
    agree[:, 1] = np.where(swapped, eq[:, 3], eq[:, 1])
    agree[:, 2] = np.where(swapped, eq[:, 3], eq[:, 0])
    agree[:, 3] = np.where(swapped, eq[:, 2], eq[:, 1])
    agree[~ph, 1], agree[~ph, 2], agree[~ph, 3] = eq[~ph, 0], eq[~ph, 0], eq[~ph, 0]
    rc, rs, rb = R["cluster"], R["side"], R["bits"]
    by_replay = ((rb & 1 == 0) | agree[rc, 2 * rs]) & ((rb & 2 == 0) | agree[rc, 2 * rs + 1]) if len(rc) else np.zeros(0, bool)
    tp = [t >= 0 for t in twin]
    for s in (0, 1):
        tp[s][own[in_r][(rs == s) & by_replay]] = True
    used_job = np.zeros((len(replayed), 4), bool)
    used_job[:, 0] = used_job[:, 2] = True
    used_job[ph, 1] = used_job[ph, 3] = True
    conflict = [int(((status[:, 2 * s:2 * s + 2] == 1) & used_job[:, 2 * s:2 * s + 2]).sum()) for s in (0, 1)]
    over_rec = [int((over[cl][side == s]).sum()) if n else 0 for s in (0, 1)]
    # ---- the summary
    n_tp = [int(t.sum()) for t in tp]
    summary = SVIM_COMPARE._scores(n_tp[0], len(b.rows) - n_tp[0], n_tp[1], len(c.rows) - n_tp[1])
    summary["by_type"] = {}
    for k, name in enumerate(TYPES):
        tb, tc = tp[0][b.kind == k], tp[1][c.kind == k]
        summary["by_type"][name] = SVIM_COMPARE._scores(int(tb.sum()), int((~tb).sum()), int(tc.sum()), int((~tc).sum()))
    summary["TP_exact"] = {"base": int((twin_b >= 0).sum()), "comp": int((twin_c >= 0).sum())}
    summary["TP_replay"] = {"base": n_tp[0] - summary["TP_exact"]["base"], "comp": n_tp[1] - summary["TP_exact"]["comp"]}
    hit = np.flatnonzero(twin_b >= 0)
    known = (b.gt[hit] != 0) & (c.gt[twin_b[hit]] != 0)
    same = _POP[b.gt[hit]] == _POP[c.gt[twin_b[hit]]]
    summary["gt_compared"], summary["gt_concordant"] = int(known.sum()), int((known & same).sum())
    summary["gt_concordance"] = SVIM_COMPARE._ratio(summary["gt_concordant"], summary["gt_compared"])
    summary["clusters"] = {"all": n_cl, "replayed": int(len(replayed)), "phased": int(ph.sum()), "union": int((~ph).sum()),
                           "straight": int((ph & ~swapped).sum()), "swapped": int(swapped.sum()), "over_max_cluster": int(over.sum())}
    for s, name in enumerate(("base", "comp")):
        d = {"records": files[s].n_lines, "compared": int(len(sides[s].rows))}
        d.update({k: files[s].counts[k] for k in _NOT_READ})
        d.update(skipped[s])
        d.update({"duplicate": int(dup[s].sum()), "conflict": conflict[s], "over_max_cluster": over_rec[s]})
        summary[name] = d
    # ---- the files
    os.makedirs(out_dir, exist_ok=True)
    for name, s, want in (("tp-base.vcf", 0, True), ("fn.vcf", 0, False), ("tp-comp.vcf", 1, True), ("fp.vcf", 1, False)):
        _write(os.path.join(out_dir, name), _vcf(files[s], sides[s].rows[tp[s] == want].tolist()))
    lines = ["#contig\tstart\tend\tmode\torientation\tequal\tbase_records\tcomp_records\n"]
    n_side = [np.bincount(rc[rs == s], minlength=len(replayed)) for s in (0, 1)]
    for k in range(len(replayed)):
        flags = ",".join(str(int(x)) for x in (equal[k] if ph[k] else equal[k, :1]))
        lines.append("%s\t%d\t%d\t%s\t%s\t%s\t%d\t%d\n" % (contigs[int(R["c_contig"][k])], R["c_lo"][k], R["c_hi"][k], "phased" if ph[k] else "union",
                                                       "swapped" if swapped[k] else "straight", flags, n_side[0][k], n_side[1][k]))
    _write(os.path.join(out_dir, "clusters.tsv"), "".join(lines).encode())
    _write(os.path.join(out_dir, "summary.json"), (json.dumps(summary, indent=1) + "\n").encode())
    return summary
