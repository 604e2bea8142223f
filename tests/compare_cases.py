"""Seeded call-set pairs for tests/test_compare_host.py and tests/test_gpu_compare.py, against tests/golden/config1/ref.fa.

A case is dict(base: [line], comp: [line], options: {...}, bed: [(contig, lo, hi)] or None); `write` turns it into the two
VCF files (and the BED) the command reads.  Lines are sequence-resolved unless a record says symbolic."""
import os

import numpy as np

from tests import compare_restatement as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config1")
REF = os.path.join(GOLD, "ref.fa")
SEQS = R.read_fasta(REF)
LEN_OF = {k: len(v) for k, v in SEQS.items()}
HEADER = "##fileformat=VCFv4.2\n##source=tests/compare_cases.py\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
DEFAULTS = dict(include_bed=None, partition_max_distance=1000, max_edit_distance=200, max_relative_distance=0.0, min_sv_size=50,
                comp_min_sv_size=30, compare_max_partition=1024, base_sample=None, comp_sample=None, passonly=False, device=0)


def deletion(contig, start, end, name, gt="1/1", symbolic=False, flt="PASS"):
    s = SEQS[contig]
    if symbolic:
        return "%s\t%d\t%s\tN\t<DEL>\t.\t%s\tSVTYPE=DEL;END=%d;SVLEN=%d\tGT\t%s" % (contig, max(start, 1), name, flt, end, start - end, gt)
    first = start - 1 if start > 0 else 0
    return "%s\t%d\t%s\t%s\t%s\t.\t%s\tSVTYPE=DEL\tGT\t%s" % (contig, first + 1, name, s[first:end], s[first:start] or ".", flt, gt)


def insertion(contig, at, seq, name, gt="1/1", flt="PASS"):
    s = SEQS[contig]
    first = at - 1 if at > 0 else 0
    return "%s\t%d\t%s\t%s\t%s\t.\t%s\tSVTYPE=INS\tGT\t%s" % (contig, first + 1, name, s[first:at] or ".", s[first:at] + seq, flt, gt)


def random_bases(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(0, 4, n))


def mutate(rng, seq, n_sub):
    s = list(seq)
    for at in rng.choice(len(s), n_sub, replace=False).tolist():
        s[at] = "ACGT"[("ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def tandem_site(contig="chr1", period=50, need=5):
    """(start, run): ref[i] == ref[i + period] for i in [start, start + run) — a deletion of `period` bases at start .. start + run
    leaves the same haplotype."""
    s = SEQS[contig]
    run = 0
    for i in range(1000, len(s) - period):
        run = run + 1 if s[i] == s[i + period] else 0
        if run >= need:
            return i - run + 1, run
    raise AssertionError("no tandem site")


def deletion_distance(contig, a, b):
    """The textbook distance of two deletions a = (start, end) and b (for cases that sit on both sides of a limit)."""
    recs = [{"class": "DEL", "contig": contig, "start": s, "end": e, "seq": ""} for s, e in (a, b)]
    return R.edit_distance(*R.haplotypes(recs[0], recs[1], SEQS))


def synthetic_cases():
    rng = np.random.default_rng(20)
    cases = {}
    # ---- the same deletion at two offsets inside a tandem repeat: distance 0
    at, run = tandem_site()
    cases["tandem_shift"] = dict(base=[deletion("chr1", at, at + 50, "b1")], comp=[deletion("chr1", at + run, at + run + 50, "c1", gt="0/1")])
    # ---- 2 base against 1 comp in one partition: the nearer one wins, the other is FN
    cases["two_base_one_comp"] = dict(base=[deletion("chr2", 30000, 30080, "b1"), deletion("chr2", 30020, 30100, "b2")],
                                      comp=[deletion("chr2", 30018, 30098, "c1")])
    # ---- a het against a hom call; symbolic against sequence-resolved; unknown genotypes never enter the concordance
    ins = random_bases(rng, 120)
    cases["genotypes"] = dict(base=[deletion("chr1", 50000, 50200, "b1", gt="0/1"), insertion("chr1", 60000, ins, "b2", gt="1|1"),
                                    deletion("chr1", 70000, 70100, "b3", gt="1/0", symbolic=True), insertion("chr10", 500, ins, "b4", gt="0|1")],
                              comp=[deletion("chr1", 50000, 50200, "c1", gt="1/1", symbolic=True), insertion("chr1", 60000, mutate(rng, ins, 6), "c2", gt="1/1"),
                                    deletion("chr1", 70000, 70100, "c3", gt="0/1"), insertion("chr10", 500, ins, "c4", gt="1/0")])
    # ---- both sides of --max_edit_distance: the same two files, the limit at the pair's distance and one below
    b, c = deletion("chr10", 40000, 40060, "b1"), deletion("chr10", 40007, 40067, "c1")
    d = deletion_distance("chr10", (40000, 40060), (40007, 40067))
    assert d > 1
    cases["at_the_limit"] = dict(base=[b], comp=[c], options=dict(max_edit_distance=d))
    cases["over_the_limit"] = dict(base=[b], comp=[c], options=dict(max_edit_distance=d - 1))
    # ---- the relative limit: floor(0.1 * 600) = 60 lets a pair in that --max_edit_distance 10 keeps out
    b, c = deletion("chr10", 80000, 80600, "b1"), deletion("chr10", 80020, 80620, "c1")
    d = deletion_distance("chr10", (80000, 80600), (80020, 80620))
    assert 10 < d <= 60
    big_b, big_c = deletion("chr10", 90000, 90600, "b2"), deletion("chr10", 90150, 90750, "c2")
    assert deletion_distance("chr10", (90000, 90600), (90150, 90750)) > 60
    cases["relative_limit"] = dict(base=[b, big_b], comp=[c, big_c], options=dict(max_edit_distance=10, max_relative_distance=0.1))
    cases["relative_limit_off"] = dict(base=[b, big_b], comp=[c, big_c], options=dict(max_edit_distance=10))
    # ---- a size difference that skips the job: 500 against 60 bases in one partition (and a pair that does match)
    cases["size_skip"] = dict(base=[deletion("chr2", 50000, 50500, "b1"), deletion("chr2", 50300, 50360, "b2")],
                              comp=[deletion("chr2", 50200, 50260, "c1"), deletion("chr2", 50001, 50501, "c2")])
    # ---- records at --min_sv_size / --comp_min_sv_size and one below
    cases["sizes"] = dict(base=[deletion("chr1", 10000, 10050, "b50"), deletion("chr1", 20000, 20049, "b49"), insertion("chr1", 30000, random_bases(rng, 50), "bi50")],
                          comp=[deletion("chr1", 10000, 10050, "c50"), deletion("chr1", 20000, 20049, "c49"), deletion("chr1", 40000, 40030, "c30"),
                                deletion("chr1", 45000, 45029, "c29"), insertion("chr1", 30000, random_bases(rng, 30), "ci30")])
    # ---- --include_bed: inside one line, touching its ends, crossing an end, spanning two abutting lines
    bed = [("chr1", 100000, 101000), ("chr1", 101000, 102000), ("chr2", 0, 1000)]
    recs = [deletion("chr1", 100000, 100060, "touch_lo"), deletion("chr1", 100940, 101000, "touch_hi"), deletion("chr1", 100970, 101030, "span_two"),
            deletion("chr1", 99990, 100050, "cross_lo"), deletion("chr1", 101950, 102010, "cross_hi"), deletion("chr1", 101400, 101460, "inside"),
            insertion("chr1", 101000, random_bases(rng, 60), "ins_on_the_seam"), insertion("chr1", 102000, random_bases(rng, 60), "ins_at_hi"),
            insertion("chr1", 102001, random_bases(rng, 60), "ins_past_hi"), deletion("chr2", 0, 60, "start_zero"), deletion("chr10", 500, 560, "other_contig")]
    cases["bed"] = dict(base=recs, comp=list(recs), bed=bed)
    # ---- a partition over a small --compare_max_partition: left unmatched, counted; the one beside it is matched
    crowd = [deletion("chr2", 70000 + 30 * k, 70060 + 30 * k, "b%d" % k) for k in range(4)]
    cases["over_cap"] = dict(base=crowd + [deletion("chr2", 90000, 90060, "b_far")],
                             comp=[deletion("chr2", 70000 + 30 * k, 70060 + 30 * k, "c%d" % k) for k in range(3)] + [deletion("chr2", 90000, 90060, "c_far")],
                             options=dict(compare_max_partition=6))
    cases["under_cap"] = dict(cases["over_cap"], options=dict(compare_max_partition=7))
    # ---- classes that are counted, not compared
    cases["not_compared"] = dict(base=[deletion("chr1", 5000, 5100, "b1"), "chr1\t300\tsnv\tA\tC\t.\tPASS\t.\tGT\t1/1", "chr1\t400\tinv\tN\t<INV>\t.\tPASS\tEND=900\tGT\t1/1",
                                       "chr1\t500\tsym\tN\t<INS>\t.\tPASS\tEND=500;SVLEN=80\tGT\t1/1", "chr1\t600\tmulti\tA\tAT,ATT\t.\tPASS\t.\tGT\t1/2",
                                       deletion("chr1", 7000, 7100, "absent", gt="0/0"), deletion("chr1", 8000, 8100, "lowq", flt="q5")],
                                 comp=[deletion("chr1", 5000, 5100, "c1"), deletion("chr1", 8000, 8100, "c_lowq")], options=dict(passonly=True))
    return cases


def crowded_case(n_ins=40, n_del=129, seed=3):
    """One partition of n_ins x n_ins insertions and one of n_del deletions a side: distance and match kernels at partition
    sizes the golden files do not have."""
    rng = np.random.default_rng(seed)
    core = random_bases(rng, 90)
    base = [insertion("chr1", 150000 + 3 * k, mutate(rng, core, int(rng.integers(0, 12))), "bi%d" % k, gt=("0/1", "1/1")[k % 2]) for k in range(n_ins)]
    comp = [insertion("chr1", 150001 + 3 * k, mutate(rng, core, int(rng.integers(0, 12))), "ci%d" % k) for k in range(n_ins)]
    # (one base apart: the haplotype strings of a pair stay under 400 bases, 16 641 pairs of them)
    base += [deletion("chr10", 100000 + k, 100060 + k + k % 3, "bd%d" % k) for k in range(n_del)]
    comp += [deletion("chr10", 100001 + k, 100061 + k + k % 2, "cd%d" % k) for k in range(n_del)]
    return dict(base=base, comp=comp)


def write(case, directory, gz=False):
    """(base path, comp path, bed path or None) of the case's files under `directory`."""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for side in ("base", "comp"):
        p = os.path.join(str(directory), side + ".vcf")
        with open(p, "w") as fh:
            fh.write(HEADER + "".join(l + "\n" for l in case[side]))
        if gz:
            from svim_asm_amd import bamio
            data = open(p, "rb").read()
            with open(p + ".gz", "wb") as fh:
                for at in range(0, len(data), 700):
                    fh.write(bamio._bgzf_member(memoryview(data)[at:at + 700], 6))
                fh.write(bamio._BGZF_EOF)
            p += ".gz"
        paths.append(p)
    bed = None
    if case.get("bed"):
        bed = os.path.join(str(directory), "regions.bed")
        with open(bed, "w") as fh:  # (out of order on purpose: the command sorts)
            fh.write("".join("%s\t%d\t%d\n" % line for line in reversed(case["bed"])))
    return paths[0], paths[1], bed


def options_of(case):
    o = dict(DEFAULTS)
    o.update(case.get("options", {}))
    return o


_RESTATED = {}


def restated(base_path, comp_path, case_options, bed=None, key=None, compiled_distance=None):
    """The restatement's answer for two files (cached per `key` for the session) with the distance matrices it matched."""
    if key is not None and key in _RESTATED:
        return _RESTATED[key]
    o = case_options
    record = []
    base = R.parse_vcf(base_path, LEN_OF, sample=o["base_sample"], passonly=o["passonly"])
    comp = R.parse_vcf(comp_path, LEN_OF, sample=o["comp_sample"], passonly=o["passonly"])
    res = R.compare(base, comp, SEQS, bed=bed, partition_max_distance=o["partition_max_distance"], max_edit_distance=o["max_edit_distance"],
                    max_relative_distance=o["max_relative_distance"], min_sv_size=o["min_sv_size"], comp_min_sv_size=o["comp_min_sv_size"],
                    compare_max_partition=o["compare_max_partition"], record=record,
                    compiled_distance=compiled_distance)
    out = (base, comp, res, record)
    if key is not None:
        _RESTATED[key] = out
    return out
