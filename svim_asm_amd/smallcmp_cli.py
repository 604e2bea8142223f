"""`svim-asm-small-compare`: score small-variant calls against a truth VCF by haplotype replay (SVIM_SMALLCMP.py;
DESIGN.md §3.20).

    svim-asm-small-compare OUT_DIR GENOME BASE.vcf[.gz] COMP.vcf[.gz] [options]

BASE is the truth, COMP the calls under test.  Records with the same position and alleles in both files match as they
are; the others are clustered, each file's alleles are applied to the reference window of their cluster, haplotype by
haplotype, on the device, and a record is a true positive when the haplotypes it is carried on come out the same in both
files.  OUT_DIR gets summary.json (TP-base, FN, TP-comp, FP, precision, recall, f1 — overall and per type —, exact and
replay matches, genotype concordance, clusters by mode and orientation, and the counts of everything that was not
compared), tp-base.vcf and fn.vcf (BASE's header and lines), tp-comp.vcf and fp.vcf (COMP's) and clusters.tsv (one line
per replayed cluster).  A .gz input has to be bgzip-compressed."""
import argparse
import logging
import os
import sys

from svim_asm_amd import SVIM_SMALLCMP, vcfin
from svim_asm_amd.fasta import BgzfFormatError, FastaFile, MissingGziError


def parse(argv):
    p = argparse.ArgumentParser(prog="svim-asm-small-compare", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("working_dir", metavar="OUT_DIR", type=os.path.abspath, help="Output directory (created if missing)")
    p.add_argument("genome", metavar="GENOME", help="Reference genome FASTA both call sets were made against (indexed with .fai)")
    p.add_argument("base", metavar="BASE.vcf[.gz]", help="The truth set")
    p.add_argument("comp", metavar="COMP.vcf[.gz]", help="The calls under test")
    p.add_argument("--max_size", type=int, default=50, help="Records whose longer allele (after trimming) has this many bases or more are left out")
    p.add_argument("--cluster_distance", type=int, default=50, help="A record this far or less behind the largest end so far joins the cluster")
    p.add_argument("--max_cluster", type=int, default=4096, help="Clusters of more records than this are not replayed (exact twins only)")
    p.add_argument("--include_bed", default=None, help="Compare only records that lie inside ONE line of this BED")
    p.add_argument("--base_sample", default=None, help="Sample column of BASE (default: the first)")
    p.add_argument("--comp_sample", default=None, help="Sample column of COMP (default: the first)")
    p.add_argument("--passonly", action="store_true", help="Leave out records whose FILTER is neither PASS nor .")
    p.add_argument("--batch_bases", type=int, default=SVIM_SMALLCMP.DEFAULT_BATCH_BASES, help="Most window and allele bytes of one device call")
    p.add_argument("--device", type=int, default=0, help="HIP device index of the GPU to use")
    p.add_argument("--verbose", action="store_true", help="Enable more verbose logging")
    return p.parse_args(argv)


def check(options):
    """Argument errors, before any work."""
    for name in ("max_size", "batch_bases", "max_cluster"):
        if getattr(options, name) < 1:
            raise ValueError("--%s %d: 1 or more" % (name, getattr(options, name)))
    if options.cluster_distance < 0:
        raise ValueError("--cluster_distance %d: 0 or more" % options.cluster_distance)
    for path in (options.base, options.comp, options.include_bed):
        if path is not None and not os.path.isfile(path):
            raise ValueError("no such file: %s" % path)


def main(argv=None):
    options = parse(list(sys.argv[1:] if argv is None else argv))
    try:
        check(options)
    except ValueError as e:
        print("svim-asm-small-compare: %s" % e, file=sys.stderr)
        return 2
    logging.getLogger().setLevel(logging.DEBUG if options.verbose else logging.INFO)
    if not logging.getLogger().handlers:
        logging.basicConfig(format="%(asctime)s [%(levelname)-7.7s]  %(message)s")
    try:
        reference = FastaFile(options.genome, device=options.device)
    except (MissingGziError, BgzfFormatError, ValueError, IOError) as e:
        logging.error("The given reference genome cannot be used (%s: %s).", options.genome, e)
        return 1
    try:
        summary = SVIM_SMALLCMP.compare(options.base, options.comp, reference, options, options.working_dir)
    except (vcfin.VcfFormatError, ValueError) as e:
        logging.error("%s", e)
        return 1
    logging.info("TP-base %d, FN %d, TP-comp %d, FP %d: %s", summary["TP-base"], summary["FN"], summary["TP-comp"], summary["FP"],
                 os.path.join(options.working_dir, "summary.json"))
    return 0


def entry():
    sys.exit(main())
