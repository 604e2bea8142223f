"""svx_variant_replay stated once more, in plain Python: the loop of include/svx.h, job by job and pair by pair, on bytes
objects and Python integers.  Nothing here is shared with the product."""

OK, OUT_OF_ORDER, NOT_INSIDE = 0, 1, 2


def replay_job(win, edits):
    """(status, string) of one job.  `win`: bytes; `edits`: (start, ref_len, alt bytes) in the given order.  The string is
    None where the status is not 0."""
    p, parts, order, inside = 0, [], True, True
    prev = None
    for start, ref_len, alt in edits:
        if start < p or (prev is not None and start <= prev):
            order = False
        if start + ref_len > len(win):
            inside = False
        parts.append(win[p:start] if start > p else b"")
        parts.append(bytes(alt))
        p = start + ref_len
        prev = start
    parts.append(win[p:])
    if not order:
        return OUT_OF_ORDER, None
    if not inside:
        return NOT_INSIDE, None
    return OK, b"".join(parts)


def replay_batch(bases, win_off, win_len, ed_first, ed_start, ed_ref_len, ed_alt_off, ed_alt_len, pair_a=(), pair_b=()):
    """The entry point's outputs for its arguments: dict(out_len, status, equal: lists; strings: a bytes or None per job;
    out: the strings one behind the other; out_off: their offsets, one more than jobs; total)."""
    pool = bytes(bytearray(bases))
    n_jobs = len(win_off)
    status, strings = [], []
    for j in range(n_jobs):
        win = pool[int(win_off[j]):int(win_off[j]) + int(win_len[j])]
        edits = [(int(ed_start[e]), int(ed_ref_len[e]), pool[int(ed_alt_off[e]):int(ed_alt_off[e]) + int(ed_alt_len[e])])
                 for e in range(int(ed_first[j]), int(ed_first[j + 1]))]
        st, s = replay_job(win, edits)
        status.append(st)
        strings.append(s)
    out_len = [len(s) if s is not None else 0 for s in strings]
    out_off = [0]
    for n in out_len:
        out_off.append(out_off[-1] + n)
    equal = []
    for a, b in zip(pair_a, pair_b):
        a, b = int(a), int(b)
        equal.append(1 if strings[a] is not None and strings[b] is not None and strings[a] == strings[b] else 0)
    return {"out_len": out_len, "status": status, "equal": equal, "strings": strings, "out": b"".join(s or b"" for s in strings),
            "out_off": out_off, "total": out_off[-1]}


def splice_brute(win, edits):
    """The string by brute force, for edits known to be in order and inside: every window position is kept or dropped, and
    every alternative allele is put in front of the position its edit starts at."""
    drop, put = set(), {}
    for start, ref_len, alt in edits:
        drop.update(range(start, start + ref_len))
        put.setdefault(start, []).append(bytes(alt))
    out = bytearray()
    for i in range(len(win) + 1):
        for alt in put.get(i, ()):
            out += alt
        if i < len(win) and i not in drop:
            out.append(win[i])
    return bytes(out)


# ------------------------------------------------------------------------------------------- the reader, stated once more
ALLELE_CLASSES = ("rows", "multiallelic", "symbolic_or_other", "not_carried", "filtered", "no_change")


class Refused(ValueError):
    pass


def _letters(s):
    return all("a" <= ch.lower() <= "z" for ch in s)


def parse_alleles(path, len_of, sample=None, passonly=False):
    """include/svx_vcfin.h's second reader in plain Python: dict(header: bytes, rows: a dictionary per row in file order,
    counts: {class: data lines}, n_lines).  Raises Refused("line N: ...") where the reader refuses."""
    import gzip
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    lines, at = [], 0
    while at < len(raw):
        nl = raw.find(b"\n", at)
        end = len(raw) if nl < 0 else nl
        lines.append((at, raw[at:end][:-1] if raw[at:end].endswith(b"\r") else raw[at:end], len(raw) if nl < 0 else nl + 1))
        at = len(raw) if nl < 0 else nl + 1
    header_end, k, chrom = 0, 0, None
    while k < len(lines) and (not lines[k][1] or lines[k][1].startswith(b"#")):
        if lines[k][1].startswith(b"#CHROM"):
            chrom = lines[k][1].decode().split("\t")
        header_end = lines[k][2]
        k += 1
    if chrom is None:
        raise Refused("line %d: no #CHROM line" % (k + 1))
    col = 9 if len(chrom) > 9 else -1
    if sample is not None:
        if sample not in chrom[9:]:
            raise Refused("line %d: no sample %s" % (k, sample))
        col = 9 + chrom[9:].index(sample)
    out = {"header": raw[:header_end], "rows": [], "counts": dict.fromkeys(ALLELE_CLASSES, 0), "n_lines": 0}
    for no in range(k, len(lines)):
        off, text, _ = lines[no]
        if not text:
            continue
        out["n_lines"] += 1
        f = text.decode("latin-1").split("\t")
        bad = lambda what: Refused("line %d: %s" % (no + 1, what))
        if len(f) < 8:
            raise bad("fewer than 8 columns")
        if f[0] not in len_of:
            raise bad("contig")
        if not f[1].isdigit() or int(f[1]) < 1:
            raise bad("POS")
        pos = int(f[1])
        if pos > len_of[f[0]]:
            raise bad("POS beyond")
        if passonly and f[6] not in ("PASS", "."):
            out["counts"]["filtered"] += 1
            continue
        if "," in f[4]:
            out["counts"]["multiallelic"] += 1
            continue
        ref, alt = ("" if f[3] == "." else f[3]), ("" if f[4] == "." else f[4])
        if not _letters(ref) or not _letters(alt):
            out["counts"]["symbolic_or_other"] += 1
            continue
        R, A = ref.upper(), alt.upper()
        if R == A:
            out["counts"]["no_change"] += 1
            continue
        p = 0
        while p < min(len(R), len(A)) and R[p] == A[p]:
            p += 1
        s = 0
        while s < min(len(R), len(A)) - p and R[len(R) - 1 - s] == A[len(A) - 1 - s]:
            s += 1
        if pos - 1 + len(R) > len_of[f[0]]:
            raise bad("REF ends beyond")
        gt, phased = 0, 1
        if col >= 0:
            if len(f) <= col:
                raise bad("no column for the sample")
            if f[8] == "GT" or f[8].startswith("GT:"):
                g = f[col].split(":")[0]
                alleles = g.replace("|", "/").split("/")
                gt = sum(1 << h for h, a in enumerate(alleles[:2]) if a == "1")
                if len(alleles) == 1 and gt == 1:
                    gt = 3
                seps = [ch for ch in g if ch in "/|"]
                phased = 1 if not seps or seps[0] == "|" or gt == 3 else 0
                if gt == 0:
                    out["counts"]["not_carried"] += 1
                    continue
        out["counts"]["rows"] += 1
        id_off = off + len(f[0].encode("latin-1")) + 1 + len(f[1]) + 1
        out["rows"].append({"contig": f[0], "start": pos - 1 + p, "ref_len": len(R) - p - s, "alt": A[p:len(A) - s], "pos": pos - 1,
                            "ref_text": ref, "gt": gt, "phased": phased, "line": no + 1, "id": f[2], "text": text, "id_off": id_off})
    return out


# ------------------------------------------------------------------------------------------ the command, stated once more
TYPES = ("SNV", "INS", "DEL", "COMPLEX")


def _type_of(r):
    if r["ref_len"] == 1 and len(r["alt"]) == 1:
        return "SNV"
    return "INS" if r["ref_len"] == 0 else "DEL" if not r["alt"] else "COMPLEX"


def _score(tp_b, fn, tp_c, fp):
    p = None if tp_c + fp == 0 else tp_c / (tp_c + fp)
    r = None if tp_b + fn == 0 else tp_b / (tp_b + fn)
    f1 = None if p is None or r is None or p + r == 0 else 2 * p * r / (p + r)
    return {"TP-base": tp_b, "FN": fn, "TP-comp": tp_c, "FP": fp, "precision": p, "recall": r, "f1": f1}


def clusters_of(records, distance):
    """records: dictionaries with contig index `c`, `start`, `ref_len`, sorted by (c, start).  Lists of records."""
    out, reach = [], None
    for r in records:
        if reach is None or r["c"] != out[-1][0]["c"] or r["start"] > reach + distance:
            out.append([])
            reach = r["start"] + r["ref_len"]
        out[-1].append(r)
        reach = max(reach, r["start"] + r["ref_len"])
    return out


def compare_small(out_dir, base_path, comp_path, ref_seqs, contigs, max_size=50, cluster_distance=50, max_cluster=4096, bed=None,
                  base_sample=None, comp_sample=None, passonly=False):
    """svim-asm-small-compare with dictionaries, loops and string splicing; writes the six files itself and returns
    (summary, details: replayed clusters as dictionaries).  `bed`: [(contig, start, end)] or None."""
    import json
    import os
    len_of = {c: len(ref_seqs[c]) for c in contigs}
    parsed = [parse_alleles(base_path, len_of, sample=base_sample, passonly=passonly), parse_alleles(comp_path, len_of, sample=comp_sample, passonly=passonly)]
    sides, skipped = [], []
    for P in parsed:
        kept, n = [], {"too_large": 0, "ref_mismatch": 0, "out_of_regions": 0}
        for r in P["rows"]:
            r = dict(r, c=contigs.index(r["contig"]), tp=False, twin=None, dup=False)
            if max(r["ref_len"], len(r["alt"])) >= max_size:
                n["too_large"] += 1
            elif ref_seqs[r["contig"]][r["pos"]:r["pos"] + len(r["ref_text"])].upper() != r["ref_text"].upper():
                n["ref_mismatch"] += 1
            elif bed is not None and not any(c == r["contig"] and lo <= r["start"] and r["start"] + r["ref_len"] <= hi for c, lo, hi in bed):
                n["out_of_regions"] += 1
            else:
                kept.append(r)
        sides.append(kept)
        skipped.append(n)
    # exact twins: the first record of a key in each file
    firsts = []
    for kept in sides:
        seen = {}
        for r in kept:
            k = (r["c"], r["start"], r["ref_len"], r["alt"])
            if k in seen:
                r["dup"] = True
            else:
                seen[k] = r
        firsts.append(seen)
    for k, rb in firsts[0].items():
        if k in firsts[1]:
            rb["twin"], firsts[1][k]["twin"] = firsts[1][k], rb
            rb["tp"] = firsts[1][k]["tp"] = True
    exact = [sum(1 for r in kept if r["twin"] is not None) for kept in sides]
    for s, kept in enumerate(sides):
        for r in kept:
            r["side"] = s
    pool = sorted([r for kept in sides for r in kept if not r["dup"]], key=lambda r: (r["c"], r["start"]))  # (stable: base first, file order)
    cls = clusters_of(pool, cluster_distance)
    details, n_over, over_rec, conflict = [], 0, [0, 0], [0, 0]
    for cl in cls:
        if len(cl) > max_cluster:
            n_over += 1
            for r in cl:
                over_rec[r["side"]] += 1
            continue
        if all(r["twin"] is not None for r in cl):
            continue
        lo, hi = min(r["start"] for r in cl), max(r["start"] + r["ref_len"] for r in cl)
        win = ref_seqs[contigs[cl[0]["c"]]][lo:hi].upper().encode()
        phased = all(r["phased"] for r in cl)

        def string(side, h):
            listed = [(r["start"] - lo, r["ref_len"], r["alt"].encode()) for r in cl
                      if r["side"] == side and (h is None or (r["gt"] or 3) >> h & 1)]
            edits = []
            for i, e in enumerate(listed):
                # an insertion and the edit that begins where it stands are one edit (two insertions there are not)
                if i and listed[i - 1][1] == 0 and e[1] > 0 and listed[i - 1][0] == e[0]:
                    edits[-1] = (e[0], e[1], listed[i - 1][2] + e[2])
                else:
                    edits.append(e)
            st, s = replay_job(win, edits)
            assert st != NOT_INSIDE
            if st == OUT_OF_ORDER:
                conflict[side] += 1
            return s
        if phased:
            S = {(s, h): string(s, h) for s in (0, 1) for h in (0, 1)}
            same = lambda a, b: 1 if S[a] is not None and S[a] == S[b] else 0
            flags = [same((0, 0), (1, 0)), same((0, 1), (1, 1)), same((0, 0), (1, 1)), same((0, 1), (1, 0))]
            swapped = flags[2] + flags[3] > flags[0] + flags[1]
            partner = {(0, 0): 2, (0, 1): 3, (1, 1): 2, (1, 0): 3} if swapped else {(0, 0): 0, (0, 1): 1, (1, 0): 0, (1, 1): 1}
            for r in cl:
                if all(flags[partner[(r["side"], h)]] for h in (0, 1) if (r["gt"] or 3) >> h & 1):
                    r["tp"] = True
        else:
            sb, sc = string(0, None), string(1, None)
            flags, swapped = [1 if sb is not None and sb == sc else 0], False
            if flags[0]:
                for r in cl:
                    r["tp"] = True
        details.append({"contig": contigs[cl[0]["c"]], "lo": lo, "hi": hi, "mode": "phased" if phased else "union",
                        "orientation": "swapped" if swapped else "straight", "flags": flags,
                        "n": [sum(1 for r in cl if r["side"] == s) for s in (0, 1)]})
    b, c = sides
    count = lambda rows, want: sum(1 for r in rows if r["tp"] == want)
    summary = _score(count(b, True), count(b, False), count(c, True), count(c, False))
    summary["by_type"] = {}
    for name in TYPES:
        tb, tc = [r for r in b if _type_of(r) == name], [r for r in c if _type_of(r) == name]
        summary["by_type"][name] = _score(count(tb, True), count(tb, False), count(tc, True), count(tc, False))
    summary["TP_exact"] = {"base": exact[0], "comp": exact[1]}
    summary["TP_replay"] = {"base": count(b, True) - exact[0], "comp": count(c, True) - exact[1]}
    pop = {1: 1, 2: 1, 3: 2}
    known = [(r["gt"], r["twin"]["gt"]) for r in b if r["twin"] is not None and r["gt"] and r["twin"]["gt"]]
    summary["gt_compared"], summary["gt_concordant"] = len(known), sum(1 for x, y in known if pop[x] == pop[y])
    summary["gt_concordance"] = None if not known else summary["gt_concordant"] / len(known)
    n_ph = sum(1 for d in details if d["mode"] == "phased")
    n_sw = sum(1 for d in details if d["orientation"] == "swapped")
    summary["clusters"] = {"all": len(cls), "replayed": len(details), "phased": n_ph, "union": len(details) - n_ph, "straight": n_ph - n_sw,
                           "swapped": n_sw, "over_max_cluster": n_over}
    for s, name in enumerate(("base", "comp")):
        d = {"records": parsed[s]["n_lines"], "compared": len(sides[s])}
        for k in ("multiallelic", "symbolic_or_other", "not_carried", "filtered", "no_change"):
            d[k] = parsed[s]["counts"][k]
        d.update(skipped[s])
        d.update({"duplicate": sum(1 for r in sides[s] if r["dup"]), "conflict": conflict[s], "over_max_cluster": over_rec[s]})
        summary[name] = d
    os.makedirs(out_dir, exist_ok=True)
    for name, s, want in (("tp-base.vcf", 0, True), ("fn.vcf", 0, False), ("tp-comp.vcf", 1, True), ("fp.vcf", 1, False)):
        head = parsed[s]["header"]
        with open(os.path.join(out_dir, name), "wb") as fh:
            fh.write(head if not head or head.endswith(b"\n") else head + b"\n")
            for r in sides[s]:
                if r["tp"] == want:
                    fh.write(r["text"] + b"\n")
    with open(os.path.join(out_dir, "clusters.tsv"), "w") as fh:
        fh.write("#contig\tstart\tend\tmode\torientation\tequal\tbase_records\tcomp_records\n")
        for d in details:
            fh.write("%s\t%d\t%d\t%s\t%s\t%s\t%d\t%d\n" % (d["contig"], d["lo"], d["hi"], d["mode"], d["orientation"],
                                                       ",".join(str(x) for x in d["flags"]), d["n"][0], d["n"][1]))
    with open(os.path.join(out_dir, "summary.json"), "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    return summary, details
