"""Plain-loop restatement of svim-asm-small: the yardstick of tests/test_small_host.py and
tests/test_gpu_small.py.  Python strings, tuples and loops; the alignments come from the pure-Python BAM reader, the
mismatching columns from the loop of tests/mismatch_restatement.py, the single-coverage segments from the loops of
tests/callable_restatement.py.  It writes small.vcf and summary.json itself and shares no code with the product.

An alignment is (contig, start, ops, SEQ or "") — a record COLLECT visits (mapped, not secondary, MAPQ >= --min_mapq)."""
import json
import os

from tests import callable_restatement as CR, mismatch_restatement as MM

COUNTS = ("records_used", "no_sequence", "spliced", "mismatches", "small_indels", "no_anchor", "ambiguous_base", "multiply_covered")


def alignments_of(path, min_mapq=20):
    """The records COLLECT visits, contig by contig in the header's order, file order inside."""
    from svim_asm_amd import bamio
    f = bamio.AlignmentFile(path, reader="python")
    out = []
    for contig in f.references:
        for a in f.fetch(contig=contig):
            if a.is_unmapped or a.is_secondary or a.mapping_quality < min_mapq:
                continue
            out.append((contig, a.reference_start, [(op, n) for op, n in a.cigartuples], a.query_sequence or ""))
    return out


def ref_length(ops):
    return sum(n for op, n in ops if op in MM.REF_OPS)


def events_of(alignments, ref_seqs, min_sv_size, counts):
    """[(contig, POS, REF, ALT, kind)] of one haplotype before the coverage filter."""
    out = []
    for contig, start, ops, seq in alignments:
        if not seq:
            counts["no_sequence"] += 1
            continue
        if any(op == 3 for op, _ in ops):
            counts["spliced"] += 1
            continue
        counts["records_used"] += 1
        ref = ref_seqs[contig]
        window = ref[start:start + ref_length(ops)]
        for ref_pos, _qry_pos, R, Q in MM.mismatches(ops, start, window.encode("latin-1"), seq.encode("latin-1")):
            counts["mismatches"] += 1
            out.append((contig, ref_pos + 1, chr(R), chr(Q), "SNV"))
        r = q = 0
        for op, n in ops:
            if op in (1, 2) and n < min_sv_size and ref_length(ops):
                counts["small_indels"] += 1
                at = start + r
                if r == 0:
                    counts["no_anchor"] += 1
                else:
                    anchor = ref[at - 1].upper()
                    if op == 1:
                        allele = (contig, at, anchor, anchor + seq[q:q + n].upper(), "INS")
                    else:
                        allele = (contig, at, ref[at - 1:at + n].upper(), anchor, "DEL")
                    if set(allele[2] + allele[3]) <= set("ACGT"):
                        out.append(allele)
                    else:
                        counts["ambiguous_base"] += 1
            if op in MM.REF_OPS:
                r += n
            if op in MM.QRY_OPS:
                q += n
    return out


def segments_of(alignments, contigs):
    """The single-coverage segments of one haplotype as (lo_key, hi_key): every visited record with reference bases covers."""
    entries = [(CR.key(contigs.index(c), s), CR.key(contigs.index(c), s + ref_length(ops))) for c, s, ops, _ in alignments if ref_length(ops)]
    entries.sort(key=lambda e: e[0])  # (stable)
    return CR.single_one(entries)


def inside_one(segments, lo, hi):
    return any(a <= lo and hi <= b for a, b in segments)


def span(contigs, event):
    lo = CR.key(contigs.index(event[0]), event[1] - 1)
    return lo, lo + len(event[2])


def call(haplotypes, ref_seqs, contigs, min_sv_size=40):
    """(records [(contig, POS, REF, ALT, kind)], genotype texts, counts per haplotype)."""
    counts, kept, segments = [], [], []
    for alignments in haplotypes:
        c = dict.fromkeys(COUNTS, 0)
        segs = segments_of(alignments, contigs)
        good = []
        for e in events_of(alignments, ref_seqs, min_sv_size, c):
            if inside_one(segs, *span(contigs, e)):
                good.append(e)
            else:
                c["multiply_covered"] += 1
        counts.append(c)
        kept.append(good)
        segments.append(segs)
    records = sorted(set(e for good in kept for e in good), key=lambda e: (contigs.index(e[0]), e[1], e[2], e[3]))
    texts = []
    for rec in records:
        lo, hi = span(contigs, rec)
        alleles = []
        for good, segs in zip(kept, segments):
            if rec in good:
                alleles.append("1")
            elif inside_one(segs, lo, hi) and not any(span(contigs, e)[0] < hi and span(contigs, e)[1] > lo for e in good):
                alleles.append("0")
            else:
                alleles.append(".")
        texts.append("|".join(alleles))
    return records, texts, counts


def vcf_text(records, texts, contigs, lengths, sample="Sample"):
    lines = ["##fileformat=VCFv4.2"] + ["##contig=<ID=%s,length=%d>" % (c, n) for c, n in zip(contigs, lengths)]
    lines += ['##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample]
    for (contig, pos, ref, alt, _kind), gt in zip(records, texts):
        lines.append("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t%s" % (contig, pos, ref, alt, gt))
    return "".join(l + "\n" for l in lines)


def summary_of(records, texts, counts):
    by_genotype = {}
    for t in sorted(texts):
        by_genotype[t] = by_genotype.get(t, 0) + 1
    return {"haplotypes": [{k: c[k] for k in COUNTS} for c in counts], "records": len(records),
            "by_type": {kind: sum(1 for r in records if r[4] == kind) for kind in ("SNV", "INS", "DEL")}, "by_genotype": by_genotype}


def write(out_dir, haplotypes, ref_seqs, contigs, sample="Sample", min_sv_size=40):
    """out_dir/small.vcf and out_dir/summary.json; returns (records, texts, summary)."""
    records, texts, counts = call(haplotypes, ref_seqs, contigs, min_sv_size)
    summary = summary_of(records, texts, counts)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "small.vcf"), "w") as fh:
        fh.write(vcf_text(records, texts, contigs, [len(ref_seqs[c]) for c in contigs], sample))
    with open(os.path.join(out_dir, "summary.json"), "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    return records, texts, summary
