"""`svim-asm-compare`: score a call set against a truth VCF (SVIM_COMPARE.py).

    svim-asm-compare OUT_DIR GENOME BASE.vcf[.gz] COMP.vcf[.gz] [options]

BASE is the truth, COMP the calls under test.  The deletions and insertions of the two files are matched one to one
inside PAIR's partitions by the haplotype edit distance PAIR and svim-asm-merge use as "the same allele".  OUT_DIR gets
summary.json (TP-base, FN, TP-comp, FP, precision, recall, f1 — overall and per type —, genotype concordance, and the
counts of everything that was not compared), tp-base.vcf and fn.vcf (BASE's header and lines), tp-comp.vcf and fp.vcf
(COMP's) and matches.tsv (one line per matched pair).  A .gz input has to be bgzip-compressed."""
import argparse
import logging
import os
import sys

from svim_asm_amd import SVIM_COMPARE, vcfin
from svim_asm_amd.fasta import BgzfFormatError, FastaFile, MissingGziError


def parse(argv):
    p = argparse.ArgumentParser(prog="svim-asm-compare", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("working_dir", metavar="OUT_DIR", type=os.path.abspath, help="Output directory (created if missing)")
    p.add_argument("genome", metavar="GENOME", help="Reference genome FASTA both call sets were made against (indexed with .fai)")
    p.add_argument("base", metavar="BASE.vcf[.gz]", help="The truth set")
    p.add_argument("comp", metavar="COMP.vcf[.gz]", help="The calls under test")
    p.add_argument("--include_bed", default=None, help="Compare only records that lie inside ONE line of this BED")
    p.add_argument("--partition_max_distance", type=int, default=1000, help="Maximum distance in bp between SVs in a partition")
    p.add_argument("--max_edit_distance", type=int, default=200, help="Maximum haplotype edit distance of a matched pair")
    p.add_argument("--max_relative_distance", type=float, default=0.0,
                   help="A pair also matches up to this fraction of the larger SV's size (default: 0.0, off)")
    p.add_argument("--min_sv_size", type=int, default=50, help="Smallest BASE record that is compared")
    p.add_argument("--comp_min_sv_size", type=int, default=30, help="Smallest COMP record that is compared")
    p.add_argument("--compare_max_partition", type=int, default=SVIM_COMPARE.DEFAULT_MAX_PARTITION,
                   help="Partitions of more records than this are left unmatched (bounds the quadratic work)")
    p.add_argument("--base_sample", default=None, help="Sample column of BASE (default: the first)")
    p.add_argument("--comp_sample", default=None, help="Sample column of COMP (default: the first)")
    p.add_argument("--passonly", action="store_true", help="Leave out records whose FILTER is neither PASS nor .")
    p.add_argument("--device", type=int, default=0, help="HIP device index of the GPU to use")
    p.add_argument("--verbose", action="store_true", help="Enable more verbose logging")
    return p.parse_args(argv)


def check(options):
    """Argument errors, before any work."""
    for name in ("partition_max_distance", "max_edit_distance", "min_sv_size", "comp_min_sv_size"):
        if getattr(options, name) < 0:
            raise ValueError("--%s %d: 0 or more" % (name, getattr(options, name)))
    if options.compare_max_partition < 2:
        raise ValueError("--compare_max_partition %d: 2 or more" % options.compare_max_partition)
    if not 0.0 <= options.max_relative_distance <= 1.0:
        raise ValueError("--max_relative_distance %r: a fraction between 0 and 1" % options.max_relative_distance)
    for path in (options.base, options.comp, options.include_bed):
        if path is not None and not os.path.isfile(path):
            raise ValueError("no such file: %s" % path)


def main(argv=None):
    options = parse(list(sys.argv[1:] if argv is None else argv))
    try:
        check(options)
    except ValueError as e:
        print("svim-asm-compare: %s" % e, file=sys.stderr)
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
        summary = SVIM_COMPARE.compare(options.base, options.comp, reference, options, options.working_dir)
    except (vcfin.VcfFormatError, ValueError) as e:
        logging.error("%s", e)
        return 1
    logging.info("TP-base %d, FN %d, TP-comp %d, FP %d: %s", summary["TP-base"], summary["FN"], summary["TP-comp"], summary["FP"],
                 os.path.join(options.working_dir, "summary.json"))
    return 0


def entry():
    sys.exit(main())
