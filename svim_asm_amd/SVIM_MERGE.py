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
and an INFO suffix per record.

With --genotype_non_carriers a sample without a row in a record's cluster is genotyped from the
coverage its run kept (`--keep_coverage`: coverage.svxt, the reference interval of every alignment COLLECT visited, a
list per haplotype): a haplotype is `0` where ONE alignment contains the record's window and `.` where none does —
every window of every record against every list of every sample in one svx_cover_query."""
import json
import logging
import os
import struct

import numpy as np

from svim_asm_amd import _lib
from svim_asm_amd import SVIM_COMBINE as _combine
from svim_asm_amd.table import CandidateTable, F_DST_REV, F_SRC_REV, T_BND, T_DEL, T_DUP_TAN, T_INS, T_INV, TYPE_ORDER, _ranges

WIRE_NAME = "candidates.svxt"
COVERAGE_NAME = "coverage.svxt"
COVERAGE_MAGIC = b"SVXCOVER"
COVERAGE_VERSION = 1
DEFAULT_MAX_PARTITION = 1024
# genotype matrix codes: bit 0 haplotype 1, bit 1 haplotype 2
GT_TEXT = ("./.", "1/0", "0/1", "1/1")
# a non-carrier's text by its coverage code (genotype_non_carriers): bit 0 haplotype 1 covers, bit 1 haplotype 2
NON_CARRIER_TEXT = ("./.", "0/.", "./0", "0/0")
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
_INFO_CARRIERS = ('##INFO=<ID=NS,Number=1,Type=Integer,Description="Number of samples with the variant">',
                  '##INFO=<ID=AC,Number=A,Type=Integer,Description="Number of haplotypes that carry the variant">',
                  '##INFO=<ID=AN,Number=1,Type=Integer,Description="Number of haplotypes of the samples with the variant">')
_INFO_GENOTYPED = ('##INFO=<ID=NS,Number=1,Type=Integer,Description="Number of samples with at least one called allele '
                   '(carriers, and non-carriers with a haplotype whose assembly spans the locus)">',
                   '##INFO=<ID=AC,Number=A,Type=Integer,Description="Number of haplotypes that carry the variant (a '
                   'non-carrier adds none)">',
                   '##INFO=<ID=AN,Number=1,Type=Integer,Description="Number of called alleles: both haplotypes of a carrier, '
                   'of a non-carrier the haplotypes with one alignment across the locus (genotype 0)">')


def _cohort_header(version, table, types_to_output, options, sample_names, genotyped=False):
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
            for info in (_INFO_GENOTYPED if genotyped else _INFO_CARRIERS):
                yield info
        yield line


def _cohort_texts(G, C=None):
    """Per record: the tab-joined genotypes and ';NS=..;AC=..;AN=..' as (pool, offsets) each.  C: the coverage codes of
    genotype_non_carriers — a sample without a row then reads NON_CARRIER_TEXT[C] and counts in NS / AN by what was
    called; a carrier's genotype stays."""
    ns = (G != 0).sum(axis=1)
    ac = ((G & 1) + (G >> 1)).sum(axis=1)
    an = 2 * ns
    which = G
    texts = GT_TEXT
    if C is not None:
        if C.shape != G.shape:
            raise ValueError("coverage codes of %r for genotypes of %r" % (C.shape, G.shape))
        ref = np.where(G == 0, C & 3, 0).astype(np.uint8)
        ns = ns + (ref != 0).sum(axis=1)
        an = an + ((ref & 1) + (ref >> 1)).sum(axis=1)
        which = np.where(G == 0, len(GT_TEXT) + ref, G)
        texts = GT_TEXT + NON_CARRIER_TEXT
    codes = np.array([g.encode() for g in texts])
    sample_lines = [b"\t".join(row) for row in codes[which].tolist()] if len(G) else []
    info_lines = [(";NS=%d;AC=%d;AN=%d" % (a, b, c)).encode() for a, b, c in zip(ns.tolist(), ac.tolist(), an.tolist())]
    out = []
    for lines in (sample_lines, info_lines):
        off = np.zeros(len(lines) + 1, np.int64)
        if lines:
            np.cumsum([len(x) for x in lines], out=off[1:])
        out.append((b"".join(lines), off))
    return tuple(out)


def write_cohort_vcf(merged, G, sample_names, version, types_to_output, reference, options, ctx=None, C=None):
    """OUT_DIR/cohort.vcf, or cohort.vcf.gz and its index with options.bgzip_output; returns the path.  C: the matrix of
    genotype_non_carriers (None: non-carriers stay ./. and the file is the one written without the option)."""
    class _Quiet(object):
        pass
    quiet = _Quiet()
    quiet.__dict__.update(vars(options))
    if getattr(options, "query_names", False):
        logging.info("--query_names is ignored: read names are not carried into the merged file")
    quiet.query_names = False
    header = "".join(line + "\n" for line in _cohort_header(version, merged, types_to_output, options, sample_names,
                                                                 genotyped=C is not None))
    header = header.encode("utf-8", "surrogateescape")
    cohort = _cohort_texts(G, C)
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


# ------------------------------------------------------------------------------ the persisted coverage
class Coverage(object):
    """The reference intervals of one sample's alignments: `lists` — one (tid, start, end) triple of int64 columns per
    haplotype, 1 for a haploid run, 2 for a diploid one in input order — each ordered by (tid, start); `end` is pos +
    ref_len, the first base behind the alignment."""

    def __init__(self, contigs, contig_len, lists):
        self.contigs = [str(c) for c in contigs]
        self.contig_len = np.asarray(contig_len, dtype=np.int64).reshape(len(self.contigs))
        self.lists = [tuple(np.ascontiguousarray(a, dtype=np.int64) for a in triple) for triple in lists]
        for tid, start, end in self.lists:
            if not len(tid) == len(start) == len(end):
                raise ValueError("coverage message: columns of %d, %d and %d intervals" % (len(tid), len(start), len(end)))

    def to_wire(self):
        """Magic, version, then the framing of CandidateTable.to_wire: a length-prefixed JSON head and raw little-endian
        arrays (no pickle)."""
        n = [len(t[0]) for t in self.lists]
        off = np.zeros(len(n) + 1, np.uint64)
        if n:
            np.cumsum(n, out=off[1:])
        cat = lambda k: np.concatenate([t[k] for t in self.lists]) if self.lists else np.zeros(0, np.int64)
        arrays = [("contig_len", self.contig_len.astype("<i8")), ("list_off", off.astype("<u8")),
                  ("tid", cat(0).astype("<i4")), ("start", cat(1).astype("<i8")), ("end", cat(2).astype("<i8"))]
        head = json.dumps({"contigs": self.contigs, "lists": len(self.lists),
                           "arrays": [[k, a.dtype.str, int(a.size)] for k, a in arrays]}).encode()
        return b"".join([COVERAGE_MAGIC, struct.pack("<IQ", COVERAGE_VERSION, len(head)), head] + [a.tobytes() for _, a in arrays])

    @staticmethod
    def from_wire(blob):
        view = memoryview(blob)
        at = len(COVERAGE_MAGIC)
        if len(view) < at + 12:
            raise ValueError("truncated coverage message")
        if bytes(view[:at]) != COVERAGE_MAGIC:
            raise ValueError("not a coverage message (no %s in front)" % COVERAGE_MAGIC.decode())
        version, n_head = struct.unpack_from("<IQ", view, at)
        at += 12
        if version != COVERAGE_VERSION:
            raise ValueError("coverage message of version %d (this reader: %d)" % (version, COVERAGE_VERSION))
        if n_head > len(view) - at:
            raise ValueError("truncated coverage message")
        head = json.loads(bytes(view[at:at + n_head]).decode())
        at += n_head
        want = {"contig_len": "<i8", "list_off": "<u8", "tid": "<i4", "start": "<i8", "end": "<i8"}
        got = {}
        for k, dt, n in head["arrays"]:
            if want.get(k) != dt or not isinstance(n, int) or n < 0:
                raise ValueError("coverage message: array %r of type %r" % (k, dt))
            nbytes = n * np.dtype(dt).itemsize
            if at + nbytes > len(view):
                raise ValueError("truncated coverage message")
            got[k] = np.frombuffer(view[at:at + nbytes], dtype=dt).astype(np.int64)
            at += nbytes
        if set(got) != set(want):
            raise ValueError("coverage message: arrays %s" % sorted(got))
        off, L = got["list_off"], head["lists"]
        if not isinstance(L, int) or len(off) != L + 1 or (L and (off[0] != 0 or bool((off[1:] < off[:-1]).any()))) or \
                not len(got["tid"]) == len(got["start"]) == len(got["end"]) == (int(off[-1]) if L else 0):
            raise ValueError("coverage message: offsets of %d lists do not match %d intervals" % (len(off) - 1, len(got["tid"])))
        lists = [tuple(got[k][int(off[l]):int(off[l + 1])] for k in ("tid", "start", "end")) for l in range(L)]
        return Coverage(head["contigs"], got["contig_len"], lists)


def keep_coverage(contigs, contig_len, lists, working_dir):
    """WORKING_DIR/coverage.svxt = Coverage(...).to_wire(), written under a temporary name and renamed."""
    path = os.path.join(working_dir, COVERAGE_NAME)
    with open(path + ".tmp", "wb") as out:
        out.write(Coverage(contigs, contig_len, lists).to_wire())
    os.replace(path + ".tmp", path)
    return path


def read_coverage(sample_dir):
    path = os.path.join(sample_dir, COVERAGE_NAME)
    hint = " (run svim-asm haploid|diploid or svim-asm-cohort with --keep_coverage)"
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError as e:
        raise ValueError("%s: %s%s" % (path, e.strerror or e, hint))
    try:
        return Coverage.from_wire(blob)
    except (ValueError, KeyError, TypeError) as e:
        raise ValueError("%s: not a complete coverage file: %s%s" % (path, e, hint))


# ------------------------------------------------------------------------------ non-carriers
def check_coverage_contigs(merged, coverages, sample_names):
    """Every coverage file was taken against the tables' reference: the first difference by name, as check_same_contigs."""
    a, la = list(merged.contigs), merged.contig_len.tolist()
    for name, cov in zip(sample_names, coverages):
        b, lb = list(cov.contigs), cov.contig_len.tolist()
        for i in range(max(len(a), len(b))):
            ca = (a[i], la[i]) if i < len(a) else None
            cb = (b[i], lb[i]) if i < len(b) else None
            if ca != cb:
                raise ValueError("the coverage of sample %s was not taken against the reference of the candidate tables: contig %d is "
                                 "%s in the tables and %s in its coverage" % (name, i, "%s (%d bp)" % ca if ca else "missing",
                                                                             "%s (%d bp)" % cb if cb else "missing"))


def record_windows(merged, margin):
    """The windows a haplotype has to span to count as reference at each record, as (record, contig, lo, hi) int64
    columns in record order: [ss - m, se + m] on sc for DEL / INV / DUP_TAN, [ds - m, ds + m] on dc for INS / DUP_INT,
    both [ss - m, ss + m] on sc and [ds - m, ds + m] on dc for BND; clamped to [0, contig length]."""
    n = len(merged)
    typ = merged.type
    src_like = (typ == T_DEL) | (typ == T_INV) | (typ == T_DUP_TAN)
    bnd = typ == T_BND
    ss, se, ds = merged.ss.astype(np.int64), merged.se.astype(np.int64), merged.ds.astype(np.int64)
    contig = np.where(src_like | bnd, merged.sc, merged.dc).astype(np.int64)
    lo = np.where(src_like | bnd, ss, ds) - margin
    hi = np.where(src_like, se, np.where(bnd, ss, ds)) + margin
    rec = np.arange(n, dtype=np.int64)
    b = np.flatnonzero(bnd)
    # a breakend's second window right behind its first
    at = np.argsort(np.concatenate([rec, rec[b]]), kind="stable")
    rec = np.concatenate([rec, rec[b]])[at]
    contig = np.concatenate([contig, merged.dc.astype(np.int64)[b]])[at]
    lo = np.concatenate([lo, ds[b] - margin])[at]
    hi = np.concatenate([hi, ds[b] + margin])[at]
    length = merged.contig_len[contig]
    lo = np.maximum(lo, 0)
    hi = np.where(length >= 0, np.minimum(hi, length), hi)  # (-1: a contig the header does not have)
    lo = np.minimum(lo, hi)
    return rec, contig, lo, hi


def genotype_non_carriers(merged, coverages, options, ctx=None, sample_names=None):
    """uint8 matrix [records, samples]: bit 0 — ONE alignment of the sample's haplotype 1 contains every window of the
    record (record_windows), bit 1 — one of haplotype 2 does; a sample with one list (a haploid run) answers both bits
    from it.  The windows of a breakend may lie in different alignments; two alignments that abut inside a window do
    not cover it.  `coverages`: a Coverage per sample (read_coverage), in column order (`sample_names`: for the messages).
    All windows of all records go to the device in one svx_cover_query against all lists of all samples."""
    coverages = list(coverages)
    S, n = len(coverages), len(merged)
    names = list(sample_names) if sample_names is not None else ["#%d" % (k + 1) for k in range(S)]
    check_coverage_contigs(merged, coverages, names)
    for name, cov in zip(names, coverages):
        if len(cov.lists) not in (1, 2):
            raise ValueError("the coverage of sample %s has %d lists (1: haploid, 2: diploid)" % (name, len(cov.lists)))
    C = np.zeros((n, S), np.uint8)
    if n == 0 or S == 0:
        return C
    margin = getattr(options, "genotype_margin", None)
    margin = int(options.partition_max_distance if margin is None else margin)
    if margin < 0:
        raise ValueError("--genotype_margin %d" % margin)
    rec, contig, lo, hi = record_windows(merged, margin)
    lists = [t for cov in coverages for t in cov.lists]
    first_list = np.cumsum([0] + [len(cov.lists) for cov in coverages])
    list_off = np.zeros(len(lists) + 1, np.uint64)
    np.cumsum([len(t[0]) for t in lists], out=list_off[1:])
    key = lambda k: (np.concatenate([t[0] for t in lists]).astype(np.uint64) << np.uint64(32)) | \
        np.concatenate([t[k] for t in lists]).astype(np.uint64)
    ctx = ctx or _lib.default_context(getattr(options, "device", 0) or 0)
    c64 = contig.astype(np.uint64) << np.uint64(32)
    inside = np.asarray(ctx.cover_query(key(1), key(2), list_off, c64 | lo.astype(np.uint64), c64 | hi.astype(np.uint64)), dtype=np.uint8)
    # a record's windows are adjacent: all of them
    first = np.searchsorted(rec, np.arange(n), side="left")
    last = np.searchsorted(rec, np.arange(n), side="right") - 1
    per_record = inside[:, first] & inside[:, last]  # [lists, records]
    for k, cov in enumerate(coverages):
        h1 = per_record[first_list[k]]
        h2 = per_record[first_list[k] + len(cov.lists) - 1]
        C[:, k] = h1 | (h2 << 1)
    return C
