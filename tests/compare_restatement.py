"""svim-asm-compare stated once more, slowly, in plain Python — the yardstick of tests/test_vcfin.py,
tests/test_compare_host.py and tests/test_gpu_compare.py.  Nothing here comes from the product: the VCF lines are taken
apart with str.split by the classification written in include/svx_vcfin.h, records are dictionaries, partitions are
formed by a loop over sorted keys, distances are the textbook edit distance over strings built the way the reference's
compute_distance builds them (SVIM_COMBINE.py:35-102), and the matching is tests/match_restatement.py."""
import gzip
import re

import numpy as np

from tests import match_restatement

NONE = match_restatement.NONE
CLASSES = ("DEL", "INS", "multiallelic", "complex", "unresolved", "other", "not_carried", "filtered")
GT_TEXT = ("./.", "1/0", "0/1", "1/1")


class Refused(Exception):
    def __init__(self, line, what):
        Exception.__init__(self, "line %d: %s" % (line, what))
        self.line = line


def read_fasta(path):
    seqs, name = {}, None
    for line in open(path):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.strip())
    return {k: "".join(v) for k, v in seqs.items()}


def _genotype(text):
    alleles = re.split(r"[/|]", text)
    if len(alleles) == 1:
        return 3 if alleles[0] == "1" else 0
    return (1 if alleles[0] == "1" else 0) | (2 if alleles[1] == "1" else 0)


def parse_vcf(path, lengths, sample=None, passonly=False):
    """lengths: {contig: length}.  Returns dict(header: bytes, records: [dict] of ALL data lines with their class, the DEL
    and INS ones with contig / start / end / seq / gt, every one with line (1-based), id and text (bytes))."""
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    header, records, n, sample_col, seen_chrom, at = b"", [], 0, None, False, 0
    for piece in raw.split(b"\n"):
        whole = piece + b"\n"
        n += 1
        last = at + len(whole) > len(raw)
        at += len(whole)
        if piece.endswith(b"\r"):
            piece = piece[:-1]
        if not piece:
            if not records and not last:
                header += whole
            continue
        if piece.startswith(b"#") and not records:
            header += whole if not last else piece
            if piece.startswith(b"#CHROM"):
                seen_chrom = True
                cols = piece.decode().split("\t")
                sample_col = 9 if len(cols) > 9 else None
                if sample is not None:
                    if sample not in cols[9:]:
                        raise Refused(n, "no sample %s" % sample)
                    sample_col = 9 + cols[9:].index(sample)
            else:
                seen_chrom = False
            continue
        if not seen_chrom:
            raise Refused(n, "no #CHROM line in front of the records")
        f = piece.decode("latin-1").split("\t")
        if len(f) < 8:
            raise Refused(n, "fewer than 8 columns")
        rec = {"line": n, "id": f[2], "text": piece}
        records.append(rec)
        if f[0] not in lengths:
            raise Refused(n, "unknown contig")
        if not f[1].isdigit() or not f[1].isascii() or int(f[1]) < 1:
            raise Refused(n, "POS")
        pos, L = int(f[1]), lengths[f[0]]
        if pos > L:
            raise Refused(n, "POS beyond the contig")
        ref, alt = f[3], f[4]
        if passonly and f[6] not in ("PASS", "."):
            rec["class"] = "filtered"
            continue
        if "," in alt:
            rec["class"] = "multiallelic"
            continue
        info = dict(kv.split("=", 1) for kv in f[7].split(";") if "=" in kv)
        if alt == "<DEL>":
            if not info.get("END", "").isdigit():
                raise Refused(n, "END")
            end, start = int(info["END"]), pos
            if "SVLEN" in info:
                if not info["SVLEN"].lstrip("+-").isdigit() or len(info["SVLEN"].lstrip("+-")) < len(info["SVLEN"]) - 1:
                    raise Refused(n, "SVLEN")
                start = end - abs(int(info["SVLEN"]))
            if start < 0 or start >= end:
                raise Refused(n, "empty interval")
            if end > L:
                raise Refused(n, "END beyond the contig")
            rec.update({"class": "DEL", "contig": f[0], "start": start, "end": end, "seq": ""})
        elif alt == "<INS>":
            rec["class"] = "unresolved"
            continue
        else:
            ref = "" if ref == "." else ref
            alt = "" if alt == "." else alt
            letters = re.compile(r"^[A-Za-z]*$")
            if not letters.match(ref) or not letters.match(alt):
                rec["class"] = "other"
                continue
            p = 0
            while p < min(len(ref), len(alt)) and ref[p].upper() == alt[p].upper():
                p += 1
            if p == len(alt) < len(ref):
                rec.update({"class": "DEL", "contig": f[0], "start": pos - 1 + p, "end": pos - 1 + len(ref), "seq": ""})
                if rec["end"] > L:
                    raise Refused(n, "deletion beyond the contig")
            elif p == len(ref) < len(alt):
                seq = alt[p:].upper()
                rec.update({"class": "INS", "contig": f[0], "start": pos - 1 + p, "end": pos - 1 + p + len(seq), "seq": seq})
                if rec["start"] > L:
                    raise Refused(n, "insertion beyond the contig")
            else:
                rec["class"] = "complex"
                continue
        rec["gt"] = 0
        if sample_col is not None:
            if len(f) <= sample_col:
                raise Refused(n, "no column for the sample")
            if f[8].split(":")[0] == "GT":
                rec["gt"] = _genotype(f[sample_col].split(":")[0])
                if rec["gt"] == 0:
                    rec["class"] = "not_carried"
    if not seen_chrom:
        raise Refused(n, "no #CHROM line")
    return {"header": header, "records": records}


def counts_of(parsed):
    return {c: sum(1 for r in parsed["records"] if r["class"] == c) for c in CLASSES}


def rows_of(parsed):
    return [r for r in parsed["records"] if r["class"] in ("DEL", "INS")]


# ------------------------------------------------------------------------------------------------- distances
def edit_distance(a, b):
    """Levenshtein distance, the textbook recurrence row by row: new[j] = min(prev[j] + 1, prev[j-1] + (a[i] != b[j]),
    new[j-1] + 1); the last term, a running minimum along the row, as min over k <= j of (t[k] - k) + j."""
    if not a or not b:
        return len(a) + len(b)
    bb = np.frombuffer(b.encode("latin-1"), dtype=np.uint8)
    idx = np.arange(len(b) + 1)
    prev = idx.copy()
    for i, ch in enumerate(a.encode("latin-1"), 1):
        t = np.empty(len(b) + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (bb != ch))
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev[-1])


def haplotypes(r1, r2, seqs):
    """The two strings compute_distance aligns for two deletions or two insertions."""
    s = seqs[r1["contig"]]

    def up(start, end):
        end = min(end, len(s))
        return s[start:end].upper() if start < end else ""
    if r1["class"] == "DEL":
        lo = max(0, min(r1["start"], r2["start"]) - 100)
        hi = min(len(s), max(r1["end"], r2["end"]) + 100)
        return [up(lo, r["start"]) + up(r["end"], hi) for r in (r1, r2)]
    lo = max(0, min(r1["start"], r2["start"]) - 100)
    hi = min(len(s), max(r1["start"], r2["start"]) + 100)
    return [up(lo, r["start"]) + r["seq"] + up(r["start"], hi) for r in (r1, r2)]


def size_of(r):
    return r["end"] - r["start"]


def key_of(r, contig_rank):
    """Candidate.get_key(): (type, contig, interval midpoint) for a deletion, (type, contig, position) for an insertion."""
    return (0 if r["class"] == "DEL" else 2, contig_rank[r["contig"]], (r["start"] + r["end"]) // 2 if r["class"] == "DEL" else r["start"])


def inside_one_line(r, bed):
    """bed: [(contig, lo, hi)].  A deletion [s, e) is inside [lo, hi) when lo <= s and e <= hi, an insertion at p when
    lo <= p <= hi — ONE line, never the union of two."""
    if r["class"] == "DEL":
        return any(c == r["contig"] and lo <= r["start"] and r["end"] <= hi for c, lo, hi in bed)
    return any(c == r["contig"] and lo <= r["start"] <= hi for c, lo, hi in bed)


def compare(base, comp, seqs, bed=None, partition_max_distance=1000, max_edit_distance=200, max_relative_distance=0.0,
            min_sv_size=50, comp_min_sv_size=30, compare_max_partition=1024, record=None, compiled_distance=None):
    """base / comp: parse_vcf results.  Returns dict(summary integers, the four lists of records, matches).
    record: a list that receives, per partition handed to the matching, (n_base, n_comp, the distance matrix as a list).
    compiled_distance: a callable on two byte strings (the compiled full DP of the oracle) in place of the textbook
    recurrence above, which it must equal (tests/test_gpu_compare.py pins that) — for partitions of 10^4 pairs."""
    contig_rank = {name: k for k, name in enumerate(sorted(seqs))}
    out = {"base": {}, "comp": {}}
    members = []
    for side, parsed, least in (("base", base, min_sv_size), ("comp", comp, comp_min_sv_size)):
        rows = rows_of(parsed)
        small = [r for r in rows if size_of(r) < least]
        rest = [r for r in rows if size_of(r) >= least]
        outside = [r for r in rest if bed is not None and not inside_one_line(r, bed)]
        kept = [r for r in rest if bed is None or inside_one_line(r, bed)]
        out[side] = {"records": len(parsed["records"]), "compared": len(kept), "size_filtered": len(small),
                     "out_of_regions": len(outside), "over_cap": 0}
        out[side].update({c: n for c, n in counts_of(parsed).items() if c not in ("DEL", "INS")})
        members += [(side, r) for r in kept]
    # base rows first, then a stable sort by key: base before comp at equal keys
    members.sort(key=lambda m: key_of(m[1], contig_rank))
    partitions = []
    for m in members:
        k = key_of(m[1], contig_rank)
        if partitions and key_of(partitions[-1][-1][1], contig_rank)[:2] == k[:2] and \
                k[2] - key_of(partitions[-1][-1][1], contig_rank)[2] <= partition_max_distance:
            partitions[-1].append(m)
        else:
            partitions.append([m])
    matched, n_over = [], 0
    for part in partitions:
        B = [r for side, r in part if side == "base"]
        C = [r for side, r in part if side == "comp"]
        if len(part) > compare_max_partition:
            n_over += 1
            out["base"]["over_cap"] += len(B)
            out["comp"]["over_cap"] += len(C)
            continue
        if not B or not C:
            continue
        dist = []
        for b in B:
            for c in C:
                limit = max(max_edit_distance, int(np.floor(max_relative_distance * max(size_of(b), size_of(c)))))
                ha, hb = haplotypes(b, c, seqs)
                d = edit_distance(ha, hb) if compiled_distance is None else int(compiled_distance(ha.encode("latin-1"), hb.encode("latin-1")))
                dist.append(d if d <= limit else NONE)
        if record is not None:
            record.append((len(B), len(C), list(dist)))
        mb, mc = match_restatement.match_one(dist, len(B), len(C))
        for i, j in enumerate(mb):
            if j != NONE:
                matched.append((B[i], C[j], dist[i * len(C) + j]))
    matched.sort(key=lambda m: m[0]["line"])
    hit_b = {id(b) for b, _, _ in matched}
    hit_c = {id(c) for _, c, _ in matched}
    kept_b = sorted((r for side, r in members if side == "base"), key=lambda r: r["line"])
    kept_c = sorted((r for side, r in members if side == "comp"), key=lambda r: r["line"])
    out["tp_base"] = [r for r in kept_b if id(r) in hit_b]
    out["fn"] = [r for r in kept_b if id(r) not in hit_b]
    out["tp_comp"] = [r for r in kept_c if id(r) in hit_c]
    out["fp"] = [r for r in kept_c if id(r) not in hit_c]
    out["matches"] = matched
    out["partitions_over_cap"] = n_over
    pop = (0, 1, 1, 2)
    both = [(b, c) for b, c, _ in matched if b["gt"] and c["gt"]]
    out["gt_compared"] = len(both)
    out["gt_concordant"] = sum(1 for b, c in both if pop[b["gt"]] == pop[c["gt"]])
    return out


def vcf_bytes(parsed, rows):
    header = parsed["header"]
    if header and not header.endswith(b"\n"):
        header += b"\n"
    return header + b"".join(r["text"] + b"\n" for r in rows)


def matches_tsv(result):
    lines = ["#base_line\tbase_id\tcomp_line\tcomp_id\ttype\tedit_distance\tbase_gt\tcomp_gt\n"]
    for b, c, d in result["matches"]:
        lines.append("%d\t%s\t%d\t%s\t%s\t%d\t%s\t%s\n" % (b["line"], b["id"], c["line"], c["id"], b["class"], d, GT_TEXT[b["gt"]],
                                                       GT_TEXT[c["gt"]]))
    return "".join(lines)
