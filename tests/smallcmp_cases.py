"""Inputs and the common check of the svim-asm-small-compare tests (tests/test_smallcmp_host.py, tests/test_gpu_smallcmp.py,
tests/test_replay_restatement.py): the fixture pair — tests/golden/config1's small.vcf by tests/small_restatement.py, and
the same alignments after tests/shift_restatement.rewrite —, rewritten copies of it, made-up files on the fixture's genome,
and `check`: the command's six files byte for byte against tests/replay_restatement.compare_small."""
import functools
import os
import tempfile

from tests import merge_restatement as MR, replay_restatement as RR, shift_restatement as SH, small_restatement as SR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config1")
REF = os.path.join(GOLD, "ref.fa")
SEQS = MR.read_fasta(REF)
NAMES = list(SEQS)
FILES = ("summary.json", "tp-base.vcf", "fn.vcf", "tp-comp.vcf", "fp.vcf", "clusters.tsv")
HEADER = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"


@functools.lru_cache(maxsize=None)
def fixture_texts():
    """(base small.vcf, comp small.vcf) as text."""
    haps = [SR.alignments_of(os.path.join(GOLD, "hap1.bam")), SR.alignments_of(os.path.join(GOLD, "hap2.bam"))]
    out = []
    with tempfile.TemporaryDirectory() as d:
        for name, hs in (("base", haps), ("comp", [SH.rewrite(h, SEQS)[0] for h in haps])):
            SR.write(os.path.join(d, name), hs, SEQS, NAMES)
            out.append(open(os.path.join(d, name, "small.vcf")).read())
    return tuple(out)


def write(tmp_path, name, text):
    p = os.path.join(str(tmp_path), name)
    os.makedirs(str(tmp_path), exist_ok=True)
    with open(p, "w") as fh:
        fh.write(text)
    return p


def map_gt(text, fn):
    """The VCF text with fn applied to the last column of every data line."""
    out = []
    for line in text.splitlines():
        if line and not line.startswith("#"):
            f = line.split("\t")
            f[-1] = fn(f[-1])
            line = "\t".join(f)
        out.append(line)
    return "\n".join(out) + "\n"


def swap_haplotypes(gt):
    a, b = gt.split("|")
    return b + "|" + a


def line(contig, pos, ref, alt, gt="1|1", rid=".", flt="PASS"):
    return "%s\t%d\t%s\t%s\t%s\t.\t%s\t.\tGT\t%s\n" % (contig, pos, rid, ref, alt, flt, gt)


def ref_at(contig, pos, n=1):
    """The genome's n bases at 1-based pos, upper case."""
    return SEQS[contig][pos - 1:pos - 1 + n].upper()


def other(base):
    return {"A": "C", "C": "G", "G": "T", "T": "A"}.get(base.upper(), "A")


def read_bed(path):
    return [(f[0], int(f[1]), int(f[2])) for f in (l.rstrip("\n").split("\t") for l in open(path)) if len(f) >= 3]


def check(run, base, comp, tmp_path, **options):
    """run(out_dir, base, comp, options) is the command; holds its files to compare_small's.  Returns (summary, details)."""
    import json
    got_dir, want_dir = os.path.join(str(tmp_path), "got"), os.path.join(str(tmp_path), "want")
    run(got_dir, base, comp, options)
    kw = {k: v for k, v in options.items() if k in ("max_size", "cluster_distance", "max_cluster", "base_sample", "comp_sample", "passonly")}
    bed = read_bed(options["include_bed"]) if options.get("include_bed") else None
    summary, details = RR.compare_small(want_dir, base, comp, SEQS, NAMES, bed=bed, **kw)
    assert sorted(os.listdir(got_dir)) == sorted(FILES)
    for name in FILES:
        assert open(os.path.join(got_dir, name), "rb").read() == open(os.path.join(want_dir, name), "rb").read(), name
    assert json.load(open(os.path.join(got_dir, "summary.json"))) == summary
    return summary, details


def argv_of(out_dir, base, comp, options):
    argv = [out_dir, REF, base, comp]
    for k, v in options.items():
        if v is True:
            argv.append("--" + k)
        elif v not in (None, False):
            argv += ["--" + k, str(v)]
    return argv
