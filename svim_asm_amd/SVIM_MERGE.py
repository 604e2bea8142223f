"""Merge the final tables of a cohort's samples into one call set with a genotype per sample (svim-asm-merge).

Input: the tables `svim-asm ... --keep_candidates` leaves as candidates.svxt (CandidateTable.to_wire), one per
sample, in manifest order.  The steps:
  * collapse — rows equal in type, coordinates, flag, copies and, for insertions, the inserted bytes are ONE
    allele with a list of carriers; on the host, a column lexsort plus a compare of the INS bytes (most carriers of
    a common variant hold byte-identical alleles: the distance jobs below are quadratic in the number of distinct
    alleles, not of samples);
  * partition — the distinct alleles' keys through svx_pair_partition, as PAIR does (SVIM_COMBINE.pair_tables);
  * distances — all pairs i < j inside a partition, whoever carries them: the haplotype edit distance of
    compute_distance through the window / recipe / distance code PAIR uses (SVIM_COMBINE._job_distances), the
    span-position distance for breakends;
  * cluster — complete linkage with a flat cut per partition (svx_linkage_cut_batch; partitions of dozens to hundreds
    of alleles take its workgroup kernel), no partition dropped for its size; beyond --merge_max_partition alleles a
    partition is left unclustered, with a warning;
  * records — one per flat cluster: the member with the most carrier haplotypes represents it, every sample gets the
    OR of its rows' haplotypes or "./.".
The VCF comes from the formatter of the single-sample file (svx_vcf_format, include/svx_text.h) with a sample text
and an INFO suffix per record."""
import logging
import os

import numpy as np

from svim_asm_amd import _lib
from svim_asm_amd import SVIM_COMBINE as _combine
from svim_asm_amd.table import CandidateTable, F_DST_REV, F_SRC_REV, T_BND, T_DEL, T_DUP_TAN, T_INS, T_INV, TYPE_ORDER, _ranges

WIRE_NAME = "candidates.svxt"
DEFAULT_MAX_PARTITION = 1024
# genotype matrix codes: bit 0 haplotype 1, bit 1 haplotype 2
GT_TEXT = ("./.", "1/0", "0/1", "1/1")
_HAP_BITS = {"1/0": 1, "0/1": 2, "1/1": 3}
_KEY_COLUMNS = ("type", "sc", "ss", "se", "dc", "ds", "de", "flag", "copies")


def check_same_contigs(tables, sample_names):
    """All tables were called against one reference: same contig names and lengths in the same order."""
    first = tables[0]
    for s in range(1, len(tables)):
        t = tables[s]
        a, b = list(first.contigs), list(t.contigs)
        la, lb = first.contig_len.tolist(), t.contig_len.tolist()
        for i in range(max(len(a), len(b))):
            ca = (a[i], la[i]) if i < len(a) else None
            cb = (b[i], lb[i]) if i < len(b) else None
            if ca != cb:
                raise ValueError("samples %s and %s were not called against the same reference: contig %d is %s in the first and "
                                 "%s in the second" % (sample_names[0], sample_names[s], i,
                                                       "%s (%d bp)" % ca if ca else "missing", "%s (%d bp)" % cb if cb else "missing"))


def _collapse(T):
    """group id of every row of T (rows equal in _KEY_COLUMNS and, for INS, in the inserted bytes share one), ids in
    order of the groups' first rows."""
    n = len(T)
    ins = T.type == T_INS
    q_len = np.where(ins, T.q_len, 0)
    cols = [getattr(T, k).astype(np.int64) for k in _KEY_COLUMNS] + [q_len]
    order = np.lexsort(tuple([np.arange(n)] + cols[::-1]))  # stable: equal rows stay in (sample, row) order
    differs = np.zeros(n, bool)
    differs[0] = True
    for c in cols:
        s = c[order]
        differs[1:] |= s[1:] != s[:-1]
    head_at = np.maximum.accumulate(np.where(differs, np.arange(n), 0))  # position of each row's run head in `order`
    head = order[head_at]
    # insertions with equal coordinates and length: equal only if their bytes are
    cand = np.flatnonzero(~differs & (q_len[order] > 0))
    if len(cand):
        seqs = np.asarray(T.seqs, dtype=np.uint8)
        rows, heads, ln = order[cand], head[cand], q_len[order[cand]]
        same = seqs[_ranges(T.q_off[rows], ln)] == seqs[_ranges(T.q_off[heads], ln)]
        off = np.cumsum(ln) - ln
        equal_head = np.add.reduceat(~same, off) == 0
        odd = cand[~equal_head]
        if len(odd):
            # runs with more than one sequence: a dictionary of the bytes per run (rare: a few loci per cohort)
            by_run = {}
            for at in odd.tolist():
                r = int(order[at])
                seen = by_run.setdefault(int(head_at[at]), {})
                key = seqs[T.q_off[r]:T.q_off[r] + T.q_len[r]].tobytes()
                if key in seen:
                    head[at] = seen[key]
                else:
                    seen[key] = r
                    head[at] = r
    first_row = np.empty(n, np.int64)
    first_row[order] = head
    uniq, group = np.unique(first_row, return_inverse=True)
    return group.reshape(n), uniq


def _hap_bits(T):
    bits = np.array([_HAP_BITS.get(g, 0) for g in T.genotypes], np.uint8)
    out = bits[T.gt] if len(T) else np.zeros(0, np.uint8)
    if len(out) and not out.all():
        raise ValueError("genotype %r in a sample's table" % (T.genotypes[int(T.gt[int(np.flatnonzero(out == 0)[0])])],))
    return out


def merge_tables(tables, sample_names, reference, options, ctx=None):
    """(merged CandidateTable, uint8 matrix [records, samples] of GT_TEXT codes): one record per cluster of alleles."""
    tables = list(tables)
    S = len(tables)
    if S == 0 or len(sample_names) != S:
        raise ValueError("one name per sample table")
    check_same_contigs(tables, sample_names)
    T = CandidateTable.concat(tables, tables[0].contigs, tables[0].contig_len)
    n = len(T)
    if n == 0:
        return T, np.zeros((0, S), np.uint8)
    sample = np.repeat(np.arange(S), [len(t) for t in tables])
    bits = _hap_bits(T)
    # ---- collapse (host: numpy)
    group, first_row = _collapse(T)
    carriers = np.bincount(group, weights=(bits & 1) + (bits >> 1), minlength=len(first_row)).astype(np.int64)
    inp = np.lexsort((first_row, T.type[first_row]))  # by type, then first carrier (sample, row)
    A = T.take(first_row[inp])
    rank_of_group = np.empty(len(inp), np.int64)
    rank_of_group[inp] = np.arange(len(inp))
    allele_of_row = rank_of_group[group]
    carriers = carriers[inp]
    nA = len(A)
    for ti, typ in enumerate(TYPE_ORDER):
        logging.info("Merging {0} distinct of {1} {2}...".format(int((A.type == ti).sum()), int((T.type == ti).sum()), _combine._LOG_NAME[typ]))
    # ---- partition
    ctx = ctx or _lib.default_context(getattr(options, "device", 0) or 0)
    perm, part_id, n_parts = ctx.pair_partition(_combine._keys_of_table(A), options.partition_max_distance)
    order = perm.astype(np.int64)
    p_size = np.bincount(part_id.astype(np.int64), minlength=n_parts).astype(np.int64)
    p_start = np.cumsum(p_size) - p_size
    p_type = A.type[order[p_start]].astype(np.int64)
    threshold = options.max_edit_distance
    cap = int(getattr(options, "merge_max_partition", DEFAULT_MAX_PARTITION) or DEFAULT_MAX_PARTITION)
    big = p_size > cap
    for pi in np.flatnonzero(big).tolist():
        rows = order[p_start[pi]:p_start[pi] + p_size[pi]]
        pos = A.key_position()[rows]
        logging.warning("Partition of {0} distinct alleles (more than --merge_max_partition {1}) left unclustered: {2} {3}:{4}-{5}".format(
            int(p_size[pi]), cap, TYPE_ORDER[p_type[pi]], A.contigs[int(A.key_contig()[rows[0]])], int(pos.min()), int(pos.max())))
    # ---- all pairs i < j of the partitions to cluster, partition after partition (the condensed vectors' order)
    P = np.flatnonzero((p_size >= 2) & ~big)
    label_sorted = np.ones(nA, np.int64)  # label of the allele at sorted position k inside its partition
    unclustered = np.repeat(big, p_size)
    label_sorted[unclustered] = (np.arange(nA) - np.repeat(p_start, p_size))[unclustered] + 1
    if len(P):
        pairs = p_size[P] * (p_size[P] - 1) // 2
        c_off = np.cumsum(pairs) - pairs
        pa, pb = np.empty(int(pairs.sum()), np.int64), np.empty(int(pairs.sum()), np.int64)
        for size in np.unique(p_size[P]).tolist():
            sel = np.flatnonzero(p_size[P] == size)
            iu, ju = np.triu_indices(size, 1)
            at = (c_off[sel][:, None] + np.arange(len(iu))[None, :]).reshape(-1)
            pa[at] = (p_start[P[sel]][:, None] + iu[None, :]).reshape(-1)
            pb[at] = (p_start[P[sel]][:, None] + ju[None, :]).reshape(-1)
        pair_part = np.repeat(P, pairs)
        a, b = order[pa], order[pb]
        cond = np.zeros(len(a), np.float64)
        bnd = p_type[pair_part] == T_BND
        if bool((~bnd).any()):
            src_like = (A.type == T_DEL) | (A.type == T_INV) | (A.type == T_DUP_TAN)
            kstart, kend = np.where(src_like, A.ss, A.ds), np.where(src_like, A.se, A.ds)
            cond[~bnd] = _combine._job_distances(ctx, A, order, p_start, p_type, kstart, kend, a[~bnd], b[~bnd], pair_part[~bnd],
                                                 (p_size[pair_part] == 2)[~bnd], threshold, reference, None)
        if bool(bnd.any()):
            x, y = a[bnd], b[bnd]
            same = (A.flag[x] & (F_SRC_REV | F_DST_REV)) == (A.flag[y] & (F_SRC_REV | F_DST_REV))
            d = (np.abs(A.ss[x] - A.ss[y]) + np.abs(A.ds[x] - A.ds[y])).astype(np.float64) / 3000.0
            cond[bnd] = np.where(same, d, float(_combine.BREAKEND_MISMATCH_DISTANCE))
        # ---- cluster: one launch per kind of distance
        p_bnd = p_type[P] == T_BND
        for sel, cut in ((~p_bnd, float(threshold)), (p_bnd, 0.3)):
            if not bool(sel.any()):
                continue
            labels = ctx.linkage_cut_batch(cond[np.repeat(sel, pairs)], p_size[P[sel]].astype(np.uint32), cut).astype(np.int64)
            label_sorted[_ranges(p_start[P[sel]], p_size[P[sel]])] = labels
    # ---- records: clusters in (partition, label) order, members in partition order
    part_sorted = np.repeat(np.arange(n_parts), p_size)
    o = np.lexsort((np.arange(nA), label_sorted, part_sorted))
    cl_new = np.ones(nA, bool)
    cl_new[1:] = (part_sorted[o][1:] != part_sorted[o][:-1]) | (label_sorted[o][1:] != label_sorted[o][:-1])
    cluster_sorted = np.empty(nA, np.int64)
    cluster_sorted[o] = np.cumsum(cl_new) - 1
    n_rec = int(cl_new.sum())
    cluster_of_allele = np.empty(nA, np.int64)
    cluster_of_allele[order] = cluster_sorted
    # the representative: most carrier haplotypes, ties to the earliest in partition order
    support = carriers[order]
    pick = np.lexsort((np.arange(nA), -support, cluster_sorted))
    head = np.ones(nA, bool)
    head[1:] = cluster_sorted[pick][1:] != cluster_sorted[pick][:-1]
    merged = A.take(order[pick[head]])
    G = np.zeros((n_rec, S), np.uint8)
    np.bitwise_or.at(G, (cluster_of_allele[allele_of_row], sample), bits)
    return merged, G


# ------------------------------------------------------------------------------ output
def _cohort_header(version, table, types_to_output, options, sample_names):
    class _Quiet(object):  # the header of a single sample without READS (query names are not merged)
        pass
    quiet = _Quiet()
    quiet.__dict__.update(vars(options))
    quiet.query_names = False
    quiet.sample = "\t".join(sample_names)
    for line in _combine._header_lines(version, table.contigs, table.contig_len.tolist(), types_to_output, quiet):
        if line.startswith("##FORMAT=<ID=CN,"):
            continue
        if line.startswith("##FILTER=<ID=not_fully_covered"):
            yield '##INFO=<ID=NS,Number=1,Type=Integer,Description="Number of samples with the variant">'
            yield '##INFO=<ID=AC,Number=A,Type=Integer,Description="Number of haplotypes that carry the variant">'
            yield '##INFO=<ID=AN,Number=1,Type=Integer,Description="Number of haplotypes of the samples with the variant">'
        yield line


def _cohort_texts(G):
    """Per record: the tab-joined genotypes and ';NS=..;AC=..;AN=..' as (pool, offsets) each."""
    ns = (G != 0).sum(axis=1)
    ac = ((G & 1) + (G >> 1)).sum(axis=1)
    codes = np.array([g.encode() for g in GT_TEXT])
    sample_lines = [b"\t".join(row) for row in codes[G].tolist()] if len(G) else []
    info_lines = [(";NS=%d;AC=%d;AN=%d" % (a, b, 2 * a)).encode() for a, b in zip(ns.tolist(), ac.tolist())]
    out = []
    for lines in (sample_lines, info_lines):
        off = np.zeros(len(lines) + 1, np.int64)
        if lines:
            np.cumsum([len(x) for x in lines], out=off[1:])
        out.append((b"".join(lines), off))
    return tuple(out)


def write_cohort_vcf(merged, G, sample_names, version, types_to_output, reference, options, ctx=None):
    """OUT_DIR/cohort.vcf, or cohort.vcf.gz and its index with options.bgzip_output; returns the path."""
    class _Quiet(object):
        pass
    quiet = _Quiet()
    quiet.__dict__.update(vars(options))
    if getattr(options, "query_names", False):
        logging.info("--query_names is ignored: read names are not carried into the merged file")
    quiet.query_names = False
    header = "".join(line + "\n" for line in _cohort_header(version, merged, types_to_output, options, sample_names))
    header = header.encode("utf-8", "surrogateescape")
    cohort = _cohort_texts(G)
    if getattr(options, "bgzip_output", False):
        from svim_asm_amd import vcf_bgzf
        path = os.path.join(options.working_dir, "cohort.vcf.gz")
        lib, buf = _lib.load(), None
        try:
            buf = _combine.vcf_body(merged, types_to_output, reference, quiet, prefix=header, cohort=cohort)
            if ctx is None and vcf_bgzf.device_path_wanted():
                ctx = _lib.default_context(getattr(options, "device", 0) or 0)
            vcf_bgzf.write(path, buf if buf is not None else header, ctx)
        except BaseException:
            for p in (path, path + ".tbi", path + ".csi"):
                if os.path.exists(p):
                    os.remove(p)
            raise
        finally:
            if buf is not None:
                lib.svx_vcf_free(buf[0])
        return path
    path = os.path.join(options.working_dir, "cohort.vcf")
    with open(path + ".tmp", "wb") as out:
        out.write(header)
        _combine.vcf_body(merged, types_to_output, reference, quiet, sink=out, cohort=cohort)
    os.replace(path + ".tmp", path)
    return path


# ------------------------------------------------------------------------------ the persisted tables
def keep_candidates(table, working_dir):
    """WORKING_DIR/candidates.svxt = table.to_wire(), written under a temporary name and renamed."""
    path = os.path.join(working_dir, WIRE_NAME)
    with open(path + ".tmp", "wb") as out:
        out.write(table.to_wire())
    os.replace(path + ".tmp", path)
    return path


def read_candidates(sample_dir):
    path = os.path.join(sample_dir, WIRE_NAME)
    hint = " (run svim-asm haploid|diploid or svim-asm-cohort with --keep_candidates)"
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError as e:
        raise ValueError("%s: %s%s" % (path, e.strerror or e, hint))
    try:
        if len(blob) < 8:
            raise ValueError("truncated table message")
        return CandidateTable.from_wire(blob)
    except (ValueError, KeyError) as e:
        raise ValueError("%s: not a complete candidate table: %s%s" % (path, e, hint))
