"""Score a call set against a truth VCF (svim-asm-compare).

BASE is the truth, COMP the calls under test.  The deletions and insertions of both files (svim_asm_amd/vcfin.py) that
pass the size and region filters are partitioned together exactly as PAIR partitions the two haplotypes of a sample;
inside a partition every (base, comp) pair gets the haplotype edit distance PAIR and the cohort merge use as "the same
allele" (SVIM_COMBINE._job_distances); a pair is eligible when that distance is within the limit, and the eligible
pairs are assigned one to one, greedily by (distance, base, comp), on the device (svx_match_greedy_batch)."""
import json
import logging
import os
import time

import numpy as np

from svim_asm_amd import SVIM_COMBINE as _combine, _lib, vcfin
from svim_asm_amd.table import CandidateTable, T_DEL, T_INS, TYPE_ORDER

DEFAULT_MAX_PARTITION = 1024
NONE = _lib.MATCH_NONE
_NOT_COMPARED = ("multiallelic", "complex", "unresolved", "other", "not_carried", "filtered")
STAGES = ("read", "partition", "distances", "match", "write")  # what a `timing` dictionary handed to compare() receives


def _clock(timing, stage, t0):
    """Seconds since t0 added to timing[stage] (timing: a caller's dictionary, or None)."""
    now = time.perf_counter()
    if timing is not None:
        timing[stage] = timing.get(stage, 0.0) + now - t0
    return now


def read_bed(path, contigs):
    """The lines of a BED as (start_key, end_key) sorted by key, key = contig index << 32 | position; every line stays a
    line of its own (abutting lines are NOT joined: a record has to lie inside ONE of them)."""
    index = {name: i for i, name in enumerate(contigs)}
    lo, hi = [], []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            f = line.rstrip("\r\n").split("\t")
            if not line.strip() or line.startswith(("#", "track ", "browser ")):
                continue
            try:
                c, s, e = index[f[0]], int(f[1]), int(f[2])
            except (KeyError, IndexError, ValueError):
                raise ValueError("%s: line %d: not `contig start end` with a contig of the genome" % (path, n))
            if not 0 <= s <= e < (1 << 32):
                raise ValueError("%s: line %d: start and end out of order or out of range" % (path, n))
            lo.append((c << 32) | s)
            hi.append((c << 32) | e)
    lo, hi = np.array(lo, np.uint64), np.array(hi, np.uint64)
    o = np.lexsort((hi, lo))
    return lo[o], hi[o]


def _sizes(t):
    return np.where(t.type == T_INS, t.q_len, t.se - t.ss).astype(np.int64)


def _select(records, min_size, bed, ctx):
    """(rows of records.table that are compared, counts of the ones that are not)."""
    t = records.table
    size = _sizes(t)
    big_enough = size >= int(min_size)
    inside = np.ones(len(t), bool)
    if bed is not None and len(bed[0]) == 0:
        inside[:] = False  # a BED without lines holds nothing
    elif bed is not None and len(t):
        ins = t.type == T_INS
        contig = np.where(ins, t.dc, t.sc).astype(np.uint64) << np.uint64(32)
        q_lo = contig | np.where(ins, t.ds, t.ss).astype(np.uint64)
        q_hi = contig | np.where(ins, t.ds, t.se).astype(np.uint64)
        inside = ctx.cover_query(bed[0], bed[1], np.array([0, len(bed[0])], np.uint64), q_lo, q_hi)[0].astype(bool)
    keep = big_enough & inside
    return np.flatnonzero(keep), {"size_filtered": int((~big_enough).sum()), "out_of_regions": int((big_enough & ~inside).sum())}


def limit_of(size_b, size_c, options):
    """Largest edit distance at which the pair still matches: max(--max_edit_distance, floor(rel * max(size_b, size_c)))."""
    rel = np.floor(float(getattr(options, "max_relative_distance", 0.0) or 0.0) * np.maximum(size_b, size_c)).astype(np.int64)
    return np.maximum(int(options.max_edit_distance), rel)


def compare_tables(tb, tc, reference, options, ctx=None, timing=None):
    """tb / tc: the compared rows of BASE and COMP as CandidateTables on the genome's contigs.  timing: a dictionary that
    receives the seconds of the partition, distances and match stages (added to what it holds).
    Returns dict(match_b: per base row the matched comp row or -1, match_c: the converse, dist_b: the pair's distance,
    over_b / over_c: bool, the row sits in a partition over the cap, n_over: such partitions)."""
    ctx = ctx or _lib.default_context(getattr(options, "device", 0) or 0)
    nB, nC = len(tb), len(tc)
    out = {"match_b": np.full(nB, -1, np.int64), "match_c": np.full(nC, -1, np.int64), "dist_b": np.full(nB, -1, np.int64),
           "over_b": np.zeros(nB, bool), "over_c": np.zeros(nC, bool), "n_over": 0}
    if nB == 0 or nC == 0:
        return out
    t0 = time.perf_counter()
    T = CandidateTable.concat([tb, tc], tb.contigs, tb.contig_len)
    n = nB + nC
    # base rows in front: the sort is stable, so base comes before comp at equal keys
    perm, part_id, n_parts = ctx.pair_partition(_combine._keys_of_table(T), options.partition_max_distance)
    order = perm.astype(np.int64)
    p_size = np.bincount(part_id.astype(np.int64), minlength=n_parts).astype(np.int64)
    p_start = np.cumsum(p_size) - p_size
    p_type = T.type[order[p_start]].astype(np.int64)
    part_sorted = np.repeat(np.arange(n_parts), p_size)
    is_comp_sorted = order >= nB
    p_nc = np.bincount(part_sorted, weights=is_comp_sorted, minlength=n_parts).astype(np.int64)
    p_nb = p_size - p_nc
    cap = int(getattr(options, "compare_max_partition", DEFAULT_MAX_PARTITION) or DEFAULT_MAX_PARTITION)
    big = p_size > cap
    for pi in np.flatnonzero(big).tolist():
        rows = order[p_start[pi]:p_start[pi] + p_size[pi]]
        pos = T.key_position()[rows]
        logging.warning("Partition of {0} records (more than --compare_max_partition {1}) left unmatched: {2} {3}:{4}-{5}".format(
            int(p_size[pi]), cap, TYPE_ORDER[p_type[pi]], T.contigs[int(T.key_contig()[rows[0]])], int(pos.min()), int(pos.max())))
    over_sorted = np.repeat(big, p_size)
    over = np.zeros(n, bool)
    over[order] = over_sorted
    out["over_b"], out["over_c"], out["n_over"] = over[:nB], over[nB:], int(big.sum())
    t0 = _clock(timing, "partition", t0)
    # ---- the partitions with something to match: members in partition order, base and comp each in their order
    P = np.flatnonzero((p_nb > 0) & (p_nc > 0) & ~big)
    if not len(P):
        return out
    # position of every member among the base (comp) members of its partition
    in_P = np.zeros(n_parts, bool)
    in_P[P] = True
    sel = in_P[part_sorted]
    rows_sel, part_sel, comp_sel = order[sel], part_sorted[sel], is_comp_sorted[sel]
    b_rows, b_part = rows_sel[~comp_sel], part_sel[~comp_sel]   # sorted by partition, partition order inside
    c_rows, c_part = rows_sel[comp_sel], part_sel[comp_sel]
    nb, nc = p_nb[P], p_nc[P]
    b_start, c_start = np.cumsum(nb) - nb, np.cumsum(nc) - nc
    pairs = nb * nc
    d_off = np.cumsum(pairs) - pairs
    n_pairs = int(pairs.sum())
    # pair k of partition q: base member k // nc, comp member k % nc (row-major, base-major)
    q_of_pair = np.repeat(np.arange(len(P)), pairs)
    k_in = np.arange(n_pairs) - d_off[q_of_pair]
    a = b_rows[b_start[q_of_pair] + k_in // nc[q_of_pair]]
    b = c_rows[c_start[q_of_pair] + k_in % nc[q_of_pair]]
    size = _sizes(T)
    limit = limit_of(size[a], size[b], options)
    # the two haplotype strings differ in length by exactly |size_a - size_b|: beyond the limit no alignment can be within it
    job = np.flatnonzero(np.abs(size[a] - size[b]) <= limit)
    dist = np.full(n_pairs, NONE, np.uint32)
    if len(job):
        src_like = T.type == T_DEL
        kstart, kend = np.where(src_like, T.ss, T.ds), np.where(src_like, T.se, T.ds)
        # one threshold for the call: the largest limit of its jobs.  Every job is "thresholded": exact up to there,
        # "more" beyond — the eligible pairs, which are reported and ordered, are all exact
        top = int(limit[job].max())
        d = _combine._job_distances(ctx, T, order, p_start, p_type, kstart, kend, a[job], b[job], P[q_of_pair[job]],
                                    np.ones(len(job), bool), top, reference, None)
        ok = d <= limit[job]
        dist[job[ok]] = d[ok].astype(np.uint32)
    t0 = _clock(timing, "distances", t0)
    mb, mc = ctx.match_greedy_batch(dist, nb.astype(np.uint32), nc.astype(np.uint32))
    _clock(timing, "match", t0)
    hit = np.flatnonzero(mb != NONE)
    q_of_b = np.repeat(np.arange(len(P)), nb)
    partner = c_rows[c_start[q_of_b[hit]] + mb[hit].astype(np.int64)]
    out["match_b"][b_rows[hit]] = partner - nB
    out["match_c"][partner - nB] = b_rows[hit]
    out["dist_b"][b_rows[hit]] = dist[d_off[q_of_b[hit]] + (hit - b_start[q_of_b[hit]]) * nc[q_of_b[hit]] + mb[hit].astype(np.int64)]
    return out


def _ratio(num, den):
    return None if den == 0 else num / den


def _scores(tp_b, fn, tp_c, fp):
    p, r = _ratio(tp_c, tp_c + fp), _ratio(tp_b, tp_b + fn)
    f1 = None if p is None or r is None or p + r == 0 else 2 * p * r / (p + r)
    return {"TP-base": tp_b, "FN": fn, "TP-comp": tp_c, "FP": fp, "precision": p, "recall": r, "f1": f1}


def _write_vcf(path, records, rows):
    with open(path, "wb") as fh:
        fh.write(records.header)
        if records.header and not records.header.endswith(b"\n"):
            fh.write(b"\n")
        for i in rows:
            fh.write(records.lines[i])
            fh.write(b"\n")


def compare(base_path, comp_path, reference, options, out_dir, ctx=None, timing=None):
    """The whole comparison; writes summary.json, tp-base.vcf, fn.vcf, tp-comp.vcf, fp.vcf and matches.tsv into out_dir
    and returns the summary.  Raises vcfin.VcfFormatError / ValueError for inputs that cannot be used.  timing: a
    dictionary that receives the seconds per stage (STAGES)."""
    t0 = time.perf_counter()
    contigs, lengths = list(reference.references), list(reference.lengths)
    base = vcfin.read_vcf(base_path, contigs, lengths, sample=getattr(options, "base_sample", None), passonly=options.passonly)
    comp = vcfin.read_vcf(comp_path, contigs, lengths, sample=getattr(options, "comp_sample", None), passonly=options.passonly)
    bed = read_bed(options.include_bed, contigs) if getattr(options, "include_bed", None) else None
    ctx = ctx or _lib.default_context(getattr(options, "device", 0) or 0)
    t0 = _clock(timing, "read", t0)
    rows_b, skipped_b = _select(base, options.min_sv_size, bed, ctx)
    rows_c, skipped_c = _select(comp, options.comp_min_sv_size, bed, ctx)
    _clock(timing, "partition", t0)
    logging.info("Comparing %d of %d base records with %d of %d comp records...", len(rows_b), base.n_lines, len(rows_c), comp.n_lines)
    res = compare_tables(base.table.take(rows_b), comp.table.take(rows_c), reference, options, ctx=ctx, timing=timing)
    t0 = time.perf_counter()
    mb, mc = res["match_b"], res["match_c"]
    type_b, type_c = base.table.type[rows_b], comp.table.type[rows_c]
    gt_b, gt_c = base.table.gt[rows_b], comp.table.gt[rows_c]
    summary = _scores(int((mb >= 0).sum()), int((mb < 0).sum()), int((mc >= 0).sum()), int((mc < 0).sum()))
    summary["by_type"] = {}
    for name, ti in (("DEL", T_DEL), ("INS", T_INS)):
        b, c = mb[type_b == ti], mc[type_c == ti]
        summary["by_type"][name] = _scores(int((b >= 0).sum()), int((b < 0).sum()), int((c >= 0).sum()), int((c < 0).sum()))
    hit = np.flatnonzero(mb >= 0)
    known = (gt_b[hit] != 0) & (gt_c[mb[hit]] != 0)
    pop = np.array([0, 1, 1, 2])
    same = pop[gt_b[hit]] == pop[gt_c[mb[hit]]]
    summary["gt_compared"], summary["gt_concordant"] = int(known.sum()), int((known & same).sum())
    summary["gt_concordance"] = _ratio(summary["gt_concordant"], summary["gt_compared"])
    for side, records, rows, skipped, over in (("base", base, rows_b, skipped_b, res["over_b"]), ("comp", comp, rows_c, skipped_c, res["over_c"])):
        d = {"records": records.n_lines, "compared": int(len(rows))}
        d.update({k: records.counts[k] for k in _NOT_COMPARED})
        d.update(skipped)
        d["over_cap"] = int(over.sum())
        summary[side] = d
    summary["partitions_over_cap"] = res["n_over"]
    os.makedirs(out_dir, exist_ok=True)
    _write_vcf(os.path.join(out_dir, "tp-base.vcf"), base, rows_b[mb >= 0].tolist())
    _write_vcf(os.path.join(out_dir, "fn.vcf"), base, rows_b[mb < 0].tolist())
    _write_vcf(os.path.join(out_dir, "tp-comp.vcf"), comp, rows_c[mc >= 0].tolist())
    _write_vcf(os.path.join(out_dir, "fp.vcf"), comp, rows_c[mc < 0].tolist())
    with open(os.path.join(out_dir, "matches.tsv"), "w") as fh:
        fh.write("#base_line\tbase_id\tcomp_line\tcomp_id\ttype\tedit_distance\tbase_gt\tcomp_gt\n")
        for i in hit.tolist():
            rb, rc = int(rows_b[i]), int(rows_c[mb[i]])
            fh.write("%d\t%s\t%d\t%s\t%s\t%d\t%s\t%s\n" % (base.line_no[rb], base.ids[rb], comp.line_no[rc], comp.ids[rc],
                                                       TYPE_ORDER[int(type_b[i])], res["dist_b"][i], vcfin.GENOTYPES[int(gt_b[i])],
                                                       vcfin.GENOTYPES[int(gt_c[mb[i]])]))
    with open(os.path.join(out_dir, "summary.json"), "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    _clock(timing, "write", t0)
    return summary
