"""PAF text written from the format's description alone (twelve tab-separated columns — qname qlen qstart qend strand
tname tlen tstart tend matches block mapq — then TAG:TYPE:VALUE fields, of which the reader under test uses tp:A, cg:Z and
NM:i), for the tests of the native PAF reader.  One record model serves both renderings of the differential tests: an
`Aln` becomes a SAM line (tests/sam_text_writer.py: soft clips, full-length SEQ, SA as include/svx_paf.h defines it) and a
PAF row plus the query's sequence in a FASTA.  Nothing here calls the code under test."""
import random

from tests import sam_text_writer as stw

_COMP = bytes.maketrans(b"ATCGMKRYVBHDatcgmkryvbhd", b"TAGCKMYRBVDHtagckmyrbvdh")


def revcomp(seq):
    """Reverse complement of an ASCII sequence (bytes or str): A<->T C<->G M<->K R<->Y V<->B H<->D in either case, every
    other byte unchanged."""
    b = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
    out = b.translate(_COMP)[::-1]
    return out.decode("latin-1") if isinstance(seq, str) else out


class Aln(object):
    """One alignment of query `qname` (length qlen): query span [qstart, qend) ON THE QUERY'S OWN STRAND, strand, target
    name and 0-based start, MAPQ, the CIGAR between the clips as (length, operator letter) pairs, NM (None: no tag),
    tp ('P', 'S', 'I', 'i' or None: no tag)."""

    def __init__(self, qname, qlen, qstart, qend, strand, tname, tstart, mapq, ops, nm=None, tp="P"):
        self.qname, self.qlen, self.qstart, self.qend, self.strand = qname, qlen, qstart, qend, strand
        self.tname, self.tstart, self.mapq, self.ops, self.nm, self.tp = tname, tstart, mapq, list(ops), nm, tp

    @property
    def tend(self):
        return self.tstart + sum(l for l, o in self.ops if o in "MDN=X")

    @property
    def clips(self):
        """(clip5, clip3) of the record in BAM orientation."""
        a, b = self.qstart, self.qlen - self.qend
        return (a, b) if self.strand == "+" else (b, a)

    def core(self):
        return "".join("%d%s" % (l, o) for l, o in self.ops)

    def cigar(self):
        c5, c3 = self.clips
        return ("%dS" % c5 if c5 else "") + self.core() + ("%dS" % c3 if c3 else "")

    def short_cigar(self):
        c5, c3 = self.clips
        q, t = self.qend - self.qstart, self.tend - self.tstart
        m = min(q, t)
        return (("%dS" % c5 if c5 else "") + ("%dM" % m if m else "") + ("%dI" % (q - m) if q > m else "") +
                ("%dD" % (t - m) if t > m else "") + ("%dS" % c3 if c3 else ""))

    def sa_element(self):
        return "%s,%d,%s,%s,%d,%d;" % (self.tname, self.tstart + 1, self.strand, self.short_cigar(), self.mapq, self.nm or 0)


def flags_and_sa(alns):
    """Per alignment (in the given = file order): (flag, SA string or None) by the definition of include/svx_paf.h."""
    groups = {}
    for k, a in enumerate(alns):
        if a.tp != "S":
            groups.setdefault(a.qname, []).append(k)
    out = []
    for k, a in enumerate(alns):
        flag = 0x10 if a.strand == "-" else 0
        if a.tp == "S":
            out.append((flag | 0x100, None))
            continue
        g = groups[a.qname]
        if g[0] != k:
            flag |= 0x800
        out.append((flag, "".join(alns[j].sa_element() for j in g if j != k) if len(g) > 1 else None))
    return out


def paf_row(a, tlen, with_cg=True, extra=()):
    q, t = a.qend - a.qstart, a.tend - a.tstart
    cols = [a.qname, a.qlen, a.qstart, a.qend, a.strand, a.tname, tlen, a.tstart, a.tend, min(q, t), max(q, t), a.mapq]
    tags = (["tp:A:%s" % a.tp] if a.tp else []) + (["NM:i:%d" % a.nm] if a.nm is not None else []) + list(extra)
    if with_cg:
        tags.append("cg:Z:" + a.core())
    return "\t".join([str(c) for c in cols] + tags)


def sam_line(a, flag, sa, query_seq):
    """The record `a` stands for, as a SAM line: soft clips, full-length SEQ in BAM orientation."""
    seq = query_seq if a.strand == "+" else revcomp(query_seq)
    aux = (["NM:i:%d" % a.nm] if a.nm is not None else []) + (["SA:Z:" + sa] if sa else [])
    return stw.record_line(a.qname, flag, a.tname, a.tstart, a.mapq, a.cigar(), seq, aux)


def write_paf(path, rows, shuffle_seed=None, eol="\n"):
    rows = list(rows)
    if shuffle_seed is not None:
        random.Random(shuffle_seed).shuffle(rows)
    with open(path, "w", newline="") as f:
        f.write("".join(r + eol for r in rows))
    return path


def write_fasta(path, names, seqs, line=60):
    """FASTA + .fai, written here (not by the product): `line` bases per line, 0 = the whole sequence on one line."""
    with open(path, "wb") as fh, open(path + ".fai", "w") as fai:
        for name, seq in zip(names, seqs):
            b = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
            fh.write(b">" + name.encode() + b"\n")
            off = fh.tell()
            w = line if line > 0 else max(1, len(b))
            for p in range(0, len(b), w):
                fh.write(b[p:p + w] + b"\n")
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (name, len(b), off, w, w + 1))
    return path


def alns_of_bam(bam_path):
    """(alignments in file order, {query name: sequence on the query's own strand}, the records' flags, references,
    lengths) of a BAM whose
    records have no hard clips and full-length SEQ (records flagged unmapped are left out).  Each record becomes the Aln
    whose record it is: clips off the CIGAR's ends, the span turned to the query's strand, tp:A:S for a secondary one;
    asserts the lossless-conversion conditions."""
    from svim_asm_amd import bamio
    bam = bamio.AlignmentFile(bam_path, reader="python")
    alns, seqs, flags = [], {}, []
    for r in bam.fetch():
        if r.flag & 4:
            continue  # (a record flagged unmapped, which every caller skips, has no row in a PAF: minimap2 writes none)
        ops = [(int(w) >> 4, stw.OPS[int(w) & 15]) for w in r.cigar_words]
        assert ops and all(o != "H" for _, o in ops), "hard clip or no CIGAR"
        c5 = ops.pop(0)[0] if ops[0][1] == "S" else 0
        c3 = ops.pop()[0] if ops and ops[-1][1] == "S" else 0
        seq = r.query_sequence
        qlen = len(seq)
        assert qlen == c5 + c3 + sum(l for l, o in ops if o in "MI=X"), "SEQ is not full-length"
        rev = bool(r.flag & 0x10)
        own = revcomp(seq) if rev else seq
        assert seqs.setdefault(r.query_name, own) == own, "records of one query disagree on its sequence"
        nm = stw.aux_values(r._tags_raw).get("NM")
        a = Aln(r.query_name, qlen, c3 if rev else c5, qlen - c5 if rev else qlen - c3, "-" if rev else "+",
                bam.references[r.reference_id], r.reference_start, r.mapping_quality, ops, nm=nm,
                tp="S" if r.flag & 0x100 else "P")
        alns.append(a)
        flags.append(r.flag)
    return alns, seqs, flags, list(bam.references), list(bam.lengths)


def bam_as_paf(bam_path, paf_path, fasta_path, shuffle_seed=1, line=60, eol="\n"):
    """The records of a BAM as PAF rows (shuffled, but a query's primary record stays in front of its supplementary
    ones: file order is what makes a row the primary) + the query FASTA with its .fai."""
    alns, seqs, flags, refs, lens = alns_of_bam(bam_path)
    tlen = dict(zip(refs, lens))
    order = list(range(len(alns)))
    if shuffle_seed is not None:
        random.Random(shuffle_seed).shuffle(order)
    # the primary of every query first among that query's rows; everything else where the shuffle put it
    first = {}
    for pos, k in enumerate(order):
        if not flags[k] & 0x900:
            first[alns[k].qname] = pos
    placed = list(order)
    for pos, k in enumerate(order):
        q = alns[k].qname
        if flags[k] & 0x800 and q in first and pos < first[q]:
            placed[pos], placed[first[q]] = placed[first[q]], placed[pos]
            first[q] = pos
    write_paf(paf_path, [paf_row(alns[k], tlen[alns[k].tname]) for k in placed], eol=eol)
    names = sorted(seqs)
    write_fasta(fasta_path, names, [seqs[n] for n in names], line=line)
    return paf_path, fasta_path
