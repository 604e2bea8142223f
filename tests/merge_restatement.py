"""The cohort merge stated once more, slowly, in plain Python — the yardstick of
tests/test_merge_host.py and tests/test_gpu_merge.py.  Nothing here comes from svim_asm_amd.SVIM_MERGE: alleles are
collapsed in a dictionary, partitions are formed by a loop over sorted keys, distances are a textbook dynamic-programming
edit distance over strings built the way the reference's compute_distance builds them (SVIM_COMBINE.py:35-102), the
clustering is scipy's linkage / fcluster, and scipy's clusters are reordered only by the rules of the merge:
clusters in label order, members in partition order."""
import numpy as np

TYPE_ORDER = ("DEL", "INV", "INS", "DUP_TAN", "DUP_INT", "BND")
_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
_BITS = {"1/0": 1, "0/1": 2, "1/1": 3}
GT_TEXT = ("./.", "1/0", "0/1", "1/1")


def read_fasta(path):
    seqs, name = {}, None
    for line in open(path):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.strip())
    return {k: "".join(v) for k, v in seqs.items()}


def allele_key(c):
    """What makes two rows the same allele: type, coordinates, flag, copies and, for insertions, the inserted bytes."""
    t = c.type
    if t == "DEL":
        return (t, c.source_contig, c.source_start, c.source_end)
    if t == "INV":
        return (t, c.source_contig, c.source_start, c.source_end, bool(c.complete))
    if t == "INS":
        return (t, c.dest_contig, c.dest_start, c.dest_end, c.sequence)
    if t == "DUP_TAN":
        return (t, c.source_contig, c.source_start, c.source_end, c.copies, bool(c.fully_covered))
    if t == "DUP_INT":
        return (t, c.source_contig, c.source_start, c.source_end, c.dest_contig, c.dest_start, c.dest_end, bool(c.cutpaste))
    return (t, c.source_contig, c.source_start, c.source_direction, c.dest_contig, c.dest_start, c.dest_direction)


def edit_distance(a, b):
    """Levenshtein distance, row by row: new[j] = min(prev[j] + 1, prev[j-1] + (a[i] != b[j]), new[j-1] + 1); the last
    term, a running minimum along the row, as min over k <= j of (t[k] - k) + j."""
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


_textbook_edit_distance = edit_distance


def haplotypes(c1, c2, seqs):
    """The two strings compute_distance aligns."""
    def up(contig, start, end):
        s = seqs[contig]
        end = min(end, len(s))
        return s[start:end].upper() if start < end else ""
    typ = c1.type
    if typ in ("DEL", "INV", "DUP_TAN"):
        contig = c1.source_contig
        lo = max(0, min(c1.source_start, c2.source_start) - 100)
        hi = min(len(seqs[contig]), max(c1.source_end, c2.source_end) + 100)
        out = []
        for c in (c1, c2):
            if typ == "DEL":
                middle = ""
            elif typ == "INV":
                middle = "".join(_COMPLEMENT.get(x, x) for x in reversed(up(contig, c.source_start, c.source_end)))
            else:
                middle = up(contig, c.source_start, c.source_end) * (c.copies + 1)
            out.append(up(contig, lo, c.source_start) + middle + up(contig, c.source_end, hi))
        return out
    contig = c1.dest_contig
    lo = max(0, min(c1.dest_start, c2.dest_start) - 100)
    hi = min(len(seqs[contig]), max(c1.dest_start, c2.dest_start) + 100)
    out = []
    for c in (c1, c2):
        middle = c.sequence if typ == "INS" else up(c.source_contig, c.source_start, c.source_end)
        out.append(up(contig, lo, c.dest_start) + middle + up(contig, c.dest_start, hi))
    return out


def distance(c1, c2, seqs, edit_distance=None):
    """edit_distance: a callable on two byte strings (the compiled full DP of the oracle, say) in place of the textbook
    one above, which it must equal (tests/test_merge_host.py pins that)."""
    if c1.type == "BND":
        if c1.source_direction == c2.source_direction and c1.dest_direction == c2.dest_direction:
            return (abs(c1.source_start - c2.source_start) + abs(c1.dest_start - c2.dest_start)) / 3000
        return 99999
    a, b = haplotypes(c1, c2, seqs)
    if edit_distance is None:
        return _textbook_edit_distance(a, b)
    return int(edit_distance(a.encode("latin-1"), b.encode("latin-1")))


def merge(samples, seqs, partition_max_distance=1000, max_edit_distance=200, merge_max_partition=1024, edit_distance=None,
          record=None):
    """samples: one list of Candidate objects per sample, each with its single-sample genotype.
    Returns ([(allele_key of the representative, [genotype text per sample])] in record order, number of partitions left
    unclustered).  record: a list that receives, per clustered partition, (type, [allele keys in partition order],
    condensed distance vector)."""
    S = len(samples)
    # ---- collapse: a dictionary; a distinct allele remembers its first carrier and all carriers
    alleles = {}
    for s, cands in enumerate(samples):
        for row, c in enumerate(cands):
            a = alleles.setdefault(allele_key(c), {"obj": c, "first": (s, row), "carriers": []})
            a["carriers"].append((s, _BITS[c.genotype]))
    records, unclustered = [], 0
    for typ in TYPE_ORDER:
        mine = sorted((a for a in alleles.values() if a["obj"].type == typ), key=lambda a: a["first"])
        mine.sort(key=lambda a: a["obj"].get_key())  # stable: equal keys stay in first-carrier order
        # ---- partitions: a new one when the contig changes or the next key position is too far
        partitions = []
        for a in mine:
            key = a["obj"].get_key()
            if partitions and partitions[-1][-1]["obj"].get_key()[1] == key[1] and \
                    key[2] - partitions[-1][-1]["obj"].get_key()[2] <= partition_max_distance:
                partitions[-1].append(a)
            else:
                partitions.append([a])
        for part in partitions:
            n = len(part)
            if n == 1:
                labels = [1]
            elif n > merge_max_partition:
                labels = list(range(1, n + 1))
                unclustered += 1
            else:
                from scipy.cluster.hierarchy import fcluster, linkage
                cond = [float(distance(part[i]["obj"], part[j]["obj"], seqs, edit_distance))
                        for i in range(n - 1) for j in range(i + 1, n)]
                if record is not None:
                    record.append((typ, [allele_key(a["obj"]) for a in part], cond))
                cut = 0.3 if typ == "BND" else max_edit_distance
                labels = fcluster(linkage(np.array(cond), method="complete"), cut, criterion="distance").tolist()
            for label in sorted(set(labels)):
                members = [a for a, l in zip(part, labels) if l == label]  # in partition order
                support = [sum(bin(b).count("1") for _, b in a["carriers"]) for a in members]
                rep = members[support.index(max(support))]  # ties: the earliest
                gts = [0] * S
                for a in members:
                    for s, b in a["carriers"]:
                        gts[s] |= b
                records.append((allele_key(rep["obj"]), [GT_TEXT[g] for g in gts]))
    return records, unclustered
