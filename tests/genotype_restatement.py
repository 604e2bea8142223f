"""Plain-loop restatement of svim-asm-genotype: the yardstick of tests/test_genotype_host.py and
tests/test_gpu_genotype.py.  Python strings, tuples and loops: the VCF is parsed line by line, the alignments come from
the pure-Python BAM reader, the spanning alignment is found by scanning the list, positions are lifted by the loop of
tests/lift_restatement.py and the distances are the textbook dynamic programme.

  sites_of(path, ...)              the DEL and INS records of a VCF that are genotyped
  alignments_of(path, ...)         the eligible alignments of a BAM in list order
  call(site, alignments, ...)      (call text, reason or None, d_ref or None, d_alt or None) of one haplotype
  expected_vcf / expected_summary  the command's two files"""
import math

from tests import lift_restatement as LR

REF_OPS = (0, 2, 3, 7, 8)  # M D N = X


def edit_distance_within(a, b, limit):
    """The edit distance of a and b when it is <= limit, else None.  The textbook row-by-row programme, kept to the
    cells with |i - j| <= limit: a path that leaves that band holds more than `limit` insertions or deletions, so every
    alignment of cost <= limit lies inside it and the banded minimum is the true distance whenever either is <= limit."""
    if abs(len(a) - len(b)) > limit:
        return None
    # a common prefix and a common suffix take no part in the distance (an optimal alignment may match them base for
    # base): without them the flanks of a window cost nothing here, and the suite stays quick
    p = 0
    while p < min(len(a), len(b)) and a[p] == b[p]:
        p += 1
    a, b = a[p:], b[p:]
    q = 0
    while q < min(len(a), len(b)) and a[len(a) - 1 - q] == b[len(b) - 1 - q]:
        q += 1
    a, b = a[:len(a) - q], b[:len(b) - q]
    big = limit + 1
    prev = {j: j for j in range(0, min(len(b), limit) + 1)}
    for i in range(1, len(a) + 1):
        cur = {}
        for j in range(max(0, i - limit), min(len(b), i + limit) + 1):
            if j == 0:
                cur[j] = i
                continue
            best = prev.get(j - 1, big) + (a[i - 1] != b[j - 1])
            up = prev.get(j, big) + 1
            left = cur.get(j - 1, big) + 1
            cur[j] = min(best, up, left, big)
        prev = cur
    d = prev.get(len(b), big)
    return d if d <= limit else None


def sites_of(path, min_size=50, passonly=False):
    """[(columns, kind, contig, s, e, seq)] of the data lines that are genotyped, in file order: DEL [s, e), INS at
    s == e with `seq`; what vcfin classes otherwise, and records below min_size, are left out."""
    out = []
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        cols = line.rstrip("\r\n").split("\t")
        chrom, pos, ref, alt = cols[0], int(cols[1]), cols[3], cols[4]
        if passonly and cols[6] not in ("PASS", "."):
            continue
        if "," in alt:
            continue
        ref = "" if ref == "." else ref
        if alt == "<DEL>":
            info = dict(kv.split("=", 1) for kv in cols[7].split(";") if "=" in kv)
            e = int(info["END"])
            s = e - abs(int(info["SVLEN"])) if "SVLEN" in info else pos
            kind, seq = "DEL", ""
        elif alt == "<INS>":
            continue
        else:
            alt = "" if alt == "." else alt
            if not (ref + alt).isalpha() and ref + alt:
                continue
            p = 0
            while p < min(len(ref), len(alt)) and ref[p].upper() == alt[p].upper():
                p += 1
            if p == len(alt) and len(alt) < len(ref):
                kind, s, e, seq = "DEL", pos - 1 + p, pos - 1 + len(ref), ""
            elif p == len(ref) and len(ref) < len(alt):
                kind, s, e, seq = "INS", pos - 1 + p, pos - 1 + p, alt[p:].upper()
            else:
                continue
        if (len(seq) if kind == "INS" else e - s) < min_size:
            continue
        out.append((cols, kind, chrom, s, e, seq))
    return out


def alignments_of(path, contigs, min_mapq=20):
    """[(contig, start, end, ops, SEQ)] of the records COLLECT visits (mapped, not secondary, mapq >= min_mapq, with
    reference bases), ordered by (index of the contig in `contigs`, start), ties in file order."""
    from svim_asm_amd import bamio
    f = bamio.AlignmentFile(path, reader="python")
    out = []
    for contig in f.references:
        for a in f.fetch(contig=contig):
            if a.is_unmapped or a.is_secondary or a.mapping_quality < min_mapq:
                continue
            ops = [(op, n) for op, n in a.cigartuples]
            ref_len = sum(n for op, n in ops if op in REF_OPS)
            if ref_len:
                out.append((contig, a.reference_start, a.reference_start + ref_len, ops, a.query_sequence or ""))
    out.sort(key=lambda t: (contigs.index(t[0]), t[1]))  # (stable)
    return out


def spanning(alignments, contig, lo, hi):
    """svx_cover_locate's choice: of the alignments on the contig with start <= lo the one that ends last, the first in
    list order among equal ends — if it reaches hi."""
    best = None
    for a in alignments:
        if a[0] == contig and a[1] <= lo and (best is None or a[2] > best[2]):
            best = a
    return best if best is not None and best[2] >= hi else None


def call(site, alignments, ref_seqs, flank=100, max_edit_distance=200, max_relative_distance=0.0):
    _cols, kind, contig, s, e, seq = site
    size = len(seq) if kind == "INS" else e - s
    limit = max(max_edit_distance, int(math.floor(max_relative_distance * size)))
    ref = ref_seqs[contig]
    lo = max(0, s - flank)
    hi = max(min(len(ref), e + flank), lo)
    a = spanning(alignments, contig, lo, hi)
    if a is None:
        return ".", "not_spanned", None, None
    q_lo, state_lo = LR.lift(a[3], a[1], lo)
    q_hi, state_hi = LR.lift(a[3], a[1], hi)
    assert state_lo != LR.OUTSIDE and state_hi != LR.OUTSIDE
    observed = a[4][q_lo:max(q_hi, q_lo)].upper()
    ref_allele = ref[lo:hi].upper()
    alt_allele = (ref[lo:s] + seq + ref[e:hi]).upper()
    d_ref = edit_distance_within(observed, ref_allele, limit)
    d_alt = edit_distance_within(observed, alt_allele, limit)
    if d_ref is None and d_alt is None:
        return ".", "other_allele", None, None
    if d_alt is not None and (d_ref is None or d_alt < d_ref):
        return "1", None, d_ref, d_alt
    if d_ref is not None and (d_alt is None or d_ref < d_alt):
        return "0", None, d_ref, d_alt
    return ".", "ambiguous", d_ref, d_alt


def genotypes(sites, haplotypes, ref_seqs, **kw):
    """[[call(...) per haplotype] per site]."""
    return [[call(site, alns, ref_seqs, **kw) for alns in haplotypes] for site in sites]


def sample_text(calls):
    text = lambda d: "." if d is None else str(d)
    return "%s:%s:%s" % ("/".join(c[0] for c in calls), ",".join(text(c[2]) for c in calls), ",".join(text(c[3]) for c in calls))


FORMAT_IDS = ("GT", "DR", "DA")


def expected_vcf(sites_path, sites, results, sample="Sample"):
    """genotypes.vcf as text: SITES' ## lines, the ##FORMAT lines of GT, DR and DA that SITES lacks (only GT can be there
    already) — taken from the product's constants, their wording is not restated —, #CHROM with one sample, the records."""
    from svim_asm_amd import SVIM_GENOTYPE
    head = [l.rstrip("\r\n") for l in open(sites_path) if l.startswith("##")]
    has_gt = any(l.startswith("##FORMAT=<ID=GT,") for l in head)
    fmt = [l.decode() for l in SVIM_GENOTYPE.FORMAT_LINES]
    assert [l.split(",")[0] for l in fmt] == ["##FORMAT=<ID=%s" % k for k in FORMAT_IDS]
    lines = head + fmt[1 if has_gt else 0:] + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample]
    for site, calls in zip(sites, results):
        lines.append("\t".join(site[0][:8]) + "\tGT:DR:DA\t" + sample_text(calls))
    return "".join(l + "\n" for l in lines)


def expected_haplotype_counts(results, n_haplotypes):
    out = []
    for h in range(n_haplotypes):
        counts = {"0": 0, "1": 0, "not_spanned": 0, "ambiguous": 0, "other_allele": 0}
        for calls in results:
            text, reason = calls[h][0], calls[h][1]
            counts[reason if reason else text] += 1
        out.append(counts)
    return out
