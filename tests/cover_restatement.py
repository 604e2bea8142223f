"""Plain-loop restatement of the non-carrier genotyping of the cohort merge: the yardstick of
tests/test_cover_host.py and tests/test_gpu_cover.py.  Tuples and loops only — no searchsorted, no prefix maximum, no
numpy: for every (list, query) the list's intervals are scanned one by one.

  cover(lists, queries)            svx_cover_query: lists of (start_key, end_key), queries of (lo_key, hi_key)
  windows(candidate, m, length)    the windows one haplotype has to span at a record
  haplotype_is_reference(...)      every window inside ONE interval (not necessarily the same one for both ends of a BND)
  sample_text / counts             the genotype column of a sample and NS / AC / AN of a record"""


def key(contig, position):
    return (contig << 32) | position


def cover(lists, queries):
    """out[l][q] = 1 when some (start, end) of lists[l] has start <= lo and end >= hi for queries[q] = (lo, hi)."""
    out = []
    for intervals in lists:
        row = []
        for lo, hi in queries:
            hit = 0
            for start, end in intervals:
                if start <= lo and end >= hi:
                    hit = 1
                    break
            row.append(hit)
        out.append(row)
    return out


def windows(candidate, margin, contig_length):
    """[(contig name, lo, hi)] of a candidate object (svim_asm_amd.SVCandidate): what one alignment has to contain.
    contig_length: name -> length."""
    t = candidate.type
    if t in ("DEL", "INV", "DUP_TAN"):
        raw = [(candidate.source_contig, candidate.source_start - margin, candidate.source_end + margin)]
    elif t in ("INS", "DUP_INT"):
        raw = [(candidate.dest_contig, candidate.dest_start - margin, candidate.dest_start + margin)]
    elif t == "BND":
        raw = [(candidate.source_contig, candidate.source_start - margin, candidate.source_start + margin),
               (candidate.dest_contig, candidate.dest_start - margin, candidate.dest_start + margin)]
    else:
        raise ValueError(t)
    out = []
    for contig, lo, hi in raw:
        if lo < 0:
            lo = 0
        if hi > contig_length[contig]:
            hi = contig_length[contig]
        out.append((contig, lo, hi))
    return out


def haplotype_is_reference(wins, intervals):
    """intervals: [(contig name, start, end)] of one haplotype's alignments."""
    for contig, lo, hi in wins:
        inside = False
        for c, start, end in intervals:
            if c == contig and start <= lo and end >= hi:
                inside = True
        if not inside:
            return False
    return True


def sample_text(carrier_text, wins, haplotypes):
    """The genotype of one sample at one record: the carrier's own where it has a row ("./." = it has none), else 0 or .
    per haplotype; a sample with one haplotype answers both sides from it."""
    if carrier_text != "./.":
        return carrier_text
    sides = [haplotypes[0], haplotypes[-1]]
    return "/".join("0" if haplotype_is_reference(wins, h) else "." for h in sides)


def counts(texts):
    """(NS, AC, AN) of a record from its samples' texts."""
    ns = ac = an = 0
    for t in texts:
        alleles = t.split("/")
        called = [a for a in alleles if a != "."]
        if called:
            ns += 1
        an += len(called)
        ac += sum(a == "1" for a in called)
    return ns, ac, an
