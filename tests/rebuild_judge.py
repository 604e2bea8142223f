"""The plain reference of the rebuild tests (tests/test_small_rebuild_host.py, tests/test_gpu_small_rebuild.py): loops
over Python strings and lists.  It imports nothing from the product and nothing from the restatements of the kernels or of
the commands — what it judges by is the property itself: the reference with a haplotype's records applied, over a stretch
that haplotype covers once, is the contig.

  depth(alignments, lengths, min_mapq)   per contig a counter per base over the visited records with reference bases
  stretches(alignment, depth)            the maximal runs of depth 1 inside one alignment
  read_vcf(path)                         [(contig, POS, REF, ALT, [allele per haplotype])]
  stripped(record)                       (pos0, ref_len, bases) without the anchor
  clipped(edit, lo, hi)                  the part of an edit inside [lo, hi); an insertion at lo belongs to the stretch in front
  rebuild(reference, lo, hi, edits)      reference[lo:hi] in upper case with the edits applied, right to left
  aligned_bases(alignment, lo, hi)       the contig's bases aligned to [lo, hi), by walking the CIGAR
  one_left(edit, reference)              the same gap one base further left (an insertion's bases rotated)
  truth_vcf(...)                         the truth in ANOTHER spelling, for svim-asm-small-compare"""

REF_OPS, QRY_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)


def ref_length(ops):
    n = 0
    for op, length in ops:
        if op in REF_OPS:
            n += length
    return n


def is_visited(a, min_mapq):
    return not (a.flag & 4) and not (a.flag & 256) and a.mapq >= min_mapq


def depth(alignments, lengths, min_mapq=20):
    """{contig: [count per base]} — single coverage is depth == 1.  (The reference of svx_cover_single here.)"""
    out = {c: [0] * n for c, n in lengths.items()}
    for a in alignments:
        if is_visited(a, min_mapq):
            for p in range(a.start, a.start + ref_length(a.ops)):
                out[a.contig][p] += 1
    return out


def stretches(a, depth_of):
    """[(lo, hi)]: every maximal run of depth 1 inside the alignment's reference interval."""
    d, out, lo = depth_of[a.contig], [], None
    end = a.start + ref_length(a.ops)
    for p in range(a.start, end + 1):
        single = p < end and d[p] == 1
        if single and lo is None:
            lo = p
        if not single and lo is not None:
            out.append((lo, p))
            lo = None
    return out


def read_vcf(path):
    out = []
    with open(path) as fh:
        for line in fh:
            if line.startswith("#"):
                continue
            f = line.rstrip("\n").split("\t")
            assert len(f) == 10 and f[2] == "." and f[5] == "." and f[6] == "PASS" and f[7] == "." and f[8] == "GT", line
            out.append((f[0], int(f[1]), f[3], f[4], f[9].split("|")))
    return out


def kind_of(ref, alt):
    return "SNV" if len(ref) == len(alt) == 1 else "INS" if len(ref) == 1 else "DEL"


def stripped(record):
    contig, pos, ref, alt = record[:4]
    if len(ref) == 1 and len(alt) == 1:
        assert ref != alt
        return pos - 1, 1, alt
    assert ref[0] == alt[0] and (len(ref) == 1 or len(alt) == 1), "an indel is anchored on the base in front and changes one side only"
    return pos, len(ref) - 1, alt[1:]


def clipped(edit, lo, hi):
    """The edit's part inside [lo, hi), or None.  An insertion AT lo follows the base lo - 1: it belongs to the stretch that
    holds that base; one at hi belongs to this one."""
    pos, ref_len, bases = edit
    if ref_len == 0:
        return edit if lo < pos <= hi else None
    a, b = max(pos, lo), min(pos + ref_len, hi)
    if a >= b:
        return None
    if len(bases) == 0:
        return a, b - a, ""
    assert ref_len == 1 and len(bases) == 1
    return edit


def rebuild(reference, lo, hi, edits, strict=True):
    """reference[lo:hi] in upper case with the edits (pos, ref_len, bases) applied, right to left.  No two edits may overlap;
    an insertion may stand at a deletion's first or last boundary (in front of what is deleted, or behind it: the same
    string).  With strict=False overlapping edits give None."""
    order = sorted(edits, key=lambda e: (e[0], 1 if e[1] else 0))
    for x, y in zip(order, order[1:]):
        fine = x[0] + x[1] <= y[0] and not (x[1] == 0 and y[1] == 0 and x[0] == y[0])
        if not fine:
            assert not strict, "two edits of one haplotype overlap: %r %r" % (x, y)
            return None
    s = list(reference[lo:hi].upper())
    for pos, ref_len, bases in reversed(order):
        assert lo <= pos and pos + ref_len <= hi
        s[pos - lo:pos - lo + ref_len] = list(bases)
    return "".join(s)


def aligned_bases(a, lo, hi):
    """The contig's bases aligned to the reference positions [lo, hi) of alignment `a`, inserted bases included (those at lo
    excluded, those at hi included: `clipped`'s rule)."""
    out, r, q = [], a.start, 0
    for op, n in a.ops:
        if op in (0, 7, 8):
            for j in range(n):
                if lo <= r + j < hi:
                    out.append(a.seq[q + j])
        elif op == 1 and lo < r <= hi:
            out.append(a.seq[q:q + n])
        if op in REF_OPS:
            r += n
        if op in QRY_OPS:
            q += n
    return "".join(out)


def one_left(edit, reference):
    """The gap one base further left: a deletion's range moves, an insertion's bases rotate (the base it passes goes in
    front, the last one is left behind)."""
    pos, ref_len, bases = edit
    if ref_len:
        return pos - 1, ref_len, ""
    return pos - 1, 0, reference[pos - 1].upper() + bases[:-1]


def one_right(edit, reference):
    pos, ref_len, bases = edit
    if ref_len:
        return pos + 1, ref_len, ""
    return pos + 1, 0, bases[1:] + reference[pos].upper()


# ------------------------------------------------------------------------------------------------ the truth, spelled otherwise
def respelled(edits, reference, lo, hi, margin=2):
    """One haplotype's kept truth edits inside one stretch [lo, hi), as the records of another caller: every ISOLATED small
    gap as far RIGHT as it goes (the string stays the same, it stays `margin` columns clear of its neighbours and inside
    the stretch), two SNVs in neighbouring columns as one 2-base record.  Returns [(pos0, REF, ALT)]."""
    edits = sorted(edits, key=lambda e: (e[0], 1 if e[1] else 0))
    before = rebuild(reference, lo, hi, edits)
    out = []
    for k, e in enumerate(edits):
        left = edits[k - 1][0] + edits[k - 1][1] if k else lo
        right = edits[k + 1][0] if k + 1 < len(edits) else hi
        if len(e[2]) == 1 and e[1] == 1:
            out.append(e)
            continue
        isolated = e[0] - left > margin and right - (e[0] + e[1]) > margin and e[0] - 1 >= lo
        while isolated:
            # one base to the right leaves the string as it is iff the base that enters the gap at its right end is the one
            # that leaves it at its left end (the whole result is rebuilt and compared below)
            leaves = reference[e[0]].upper() if e[1] else e[2][0]
            if e[0] + e[1] + 1 + margin >= right or leaves not in "ACGT" or reference[e[0] + e[1]].upper() != leaves:
                break
            e = one_right(e, reference)
        out.append(e)
    assert rebuild(reference, lo, hi, out) == before
    records, k = [], 0
    while k < len(out):
        pos, ref_len, bases = out[k]
        if ref_len == 1 and len(bases) == 1:
            nxt = out[k + 1] if k + 1 < len(out) else None
            if nxt is not None and nxt[0] == pos + 1 and nxt[1] == 1 and len(nxt[2]) == 1:
                records.append((pos, reference[pos:pos + 2].upper(), bases + nxt[2]))
                k += 2
                continue
            records.append((pos, reference[pos].upper(), bases))
        else:
            anchor = reference[pos - 1].upper()
            records.append((pos - 1, anchor + reference[pos:pos + ref_len].upper(), anchor + bases))
        k += 1
    return records


def write_truth_vcf(path, order, lengths, per_haplotype):
    """per_haplotype: per haplotype [(contig, pos0, REF, ALT)].  Phased genotypes; equal records of both haplotypes are one
    line (1|1)."""
    carried = {}
    for h, records in enumerate(per_haplotype):
        for rec in records:
            carried.setdefault(rec, set()).add(h)
    lines = ["##fileformat=VCFv4.2"] + ["##contig=<ID=%s,length=%d>" % (c, lengths[c]) for c in order]
    lines += ['##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ttruth"]
    for rec in sorted(carried, key=lambda r: (order.index(r[0]), r[1], r[2], r[3])):
        gt = "|".join("1" if h in carried[rec] else "0" for h in range(len(per_haplotype)))
        lines.append("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t%s" % (rec[0], rec[1] + 1, rec[2], rec[3], gt))
    with open(path, "w") as fh:
        fh.write("".join(l + "\n" for l in lines))
    return path


def write_bed(path, rows):
    with open(path, "w") as fh:
        for contig, lo, hi in rows:
            fh.write("%s\t%d\t%d\n" % (contig, lo, hi))
    return path
