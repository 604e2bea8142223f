"""`svim-asm-genotype`: call known SVs in an assembly's alignments (SVIM_GENOTYPE.py).

    svim-asm-genotype OUT_DIR GENOME SITES.vcf[.gz] HAP1 [HAP2] [options]

SITES is any VCF whose deletions and insertions are the sites to genotype — a cohort's cohort.vcf, a truth set, another
caller's output; its genotype columns do not matter.  HAP1 and HAP2 are the alignments of the sample's haplotype
assemblies to GENOME (BAM, SAM, or PAF with --query1 / --query2).  Per site and haplotype the bases the spanning
alignment holds over the site's window are compared with the reference allele and with the alternative allele.  OUT_DIR
gets genotypes.vcf (SITES' header and records with one sample column GT:DR:DA, haplotype 1 first) and summary.json.  A
.gz input has to be bgzip-compressed."""
import argparse
import logging
import os
import sys

from svim_asm_amd import SVIM_GENOTYPE, vcfin
from svim_asm_amd.fasta import BgzfFormatError, FastaFile, MissingGziError


def parse(argv):
    p = argparse.ArgumentParser(prog="svim-asm-genotype", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("working_dir", metavar="OUT_DIR", type=os.path.abspath, help="Output directory (created if missing)")
    p.add_argument("genome", metavar="GENOME", help="Reference genome FASTA the sites and the alignments refer to (indexed with .fai)")
    p.add_argument("sites", metavar="SITES.vcf[.gz]", help="The sites to genotype")
    p.add_argument("hap1", metavar="HAP1", help="Alignments of the first haplotype's assembly (BAM, SAM, or PAF with --query1)")
    p.add_argument("hap2", metavar="HAP2", nargs="?", default=None, help="Alignments of the second haplotype's assembly")
    p.add_argument("--query1", default=None, help="Assembly FASTA of HAP1 when it is a PAF")
    p.add_argument("--query2", default=None, help="Assembly FASTA of HAP2 when it is a PAF")
    p.add_argument("--sample", default="Sample", help="Name of the sample column (default: %(default)s)")
    p.add_argument("--flank", type=int, default=100, help="Bases on either side of a site its window takes in (default: %(default)s)")
    p.add_argument("--max_edit_distance", type=int, default=200, help="Largest edit distance at which an allele counts as observed")
    p.add_argument("--max_relative_distance", type=float, default=0.0,
                   help="An allele is also observed up to this fraction of the SV's size (default: 0.0, off)")
    p.add_argument("--min_sv_size", type=int, default=50, help="Smallest record that is genotyped (default: %(default)s)")
    p.add_argument("--min_mapq", type=int, default=20, help="Alignments below this mapping quality are ignored (default: %(default)s)")
    p.add_argument("--passonly", action="store_true", help="Leave out records whose FILTER is neither PASS nor .")
    p.add_argument("--no_bgzf_crc", action="store_true", help="Do not check the CRC32 of the BGZF members of a BAM")
    p.add_argument("--device", type=int, default=0, help="HIP device index of the GPU to use")
    p.add_argument("--verbose", action="store_true", help="Enable more verbose logging")
    return p.parse_args(argv)


def check(options):
    """Argument errors, before any work."""
    for name in ("flank", "max_edit_distance", "min_sv_size", "min_mapq"):
        if getattr(options, name) < 0:
            raise ValueError("--%s %d: 0 or more" % (name, getattr(options, name)))
    if not 0.0 <= options.max_relative_distance <= 1.0:
        raise ValueError("--max_relative_distance %r: a fraction between 0 and 1" % options.max_relative_distance)
    for path in (options.sites, options.hap1, options.hap2, options.query1, options.query2):
        if path is not None and not os.path.isfile(path):
            raise ValueError("no such file: %s" % path)
    if options.query2 is not None and options.hap2 is None:
        raise ValueError("--query2 without HAP2")
    if "\t" in options.sample or "\n" in options.sample or not options.sample:
        raise ValueError("--sample %r: a name without tabs or line ends" % options.sample)


def main(argv=None):
    options = parse(list(sys.argv[1:] if argv is None else argv))
    try:
        check(options)
    except ValueError as e:
        print("svim-asm-genotype: %s" % e, file=sys.stderr)
        return 2
    logging.getLogger().setLevel(logging.DEBUG if options.verbose else logging.INFO)
    if not logging.getLogger().handlers:
        logging.basicConfig(format="%(asctime)s [%(levelname)-7.7s]  %(message)s")
    from svim_asm_amd import cli
    options.sub = "haploid" if options.hap2 is None else "diploid"  # (how cli sizes the readers' thread pools)
    try:
        reference = FastaFile(options.genome, device=options.device)
    except (MissingGziError, BgzfFormatError, ValueError, IOError) as e:
        logging.error("The given reference genome cannot be used (%s: %s).", options.genome, e)
        return 1
    try:
        if options.hap2 is None:
            files = [cli._open(options.hap1, "", options, query=options.query1)]
        else:
            second = cli._open_ahead(options.hap2, options, query=options.query2)
            files = [cli._open(options.hap1, "first", options, query=options.query1)]
            files.append(cli._open(options.hap2, "second", options, opened=second, query=options.query2) if files[0] is not None else None)
        if any(f is None for f in files):
            return 1
        summary = SVIM_GENOTYPE.genotype(options.sites, reference, files, options, options.working_dir)
    except (vcfin.VcfFormatError, ValueError, IOError) as e:
        logging.error("%s", e)
        return 1
    for h, counts in enumerate(summary["haplotypes"]):
        logging.info("Haplotype %d: %s", h + 1, ", ".join("%s %d" % kv for kv in counts.items()))
    logging.info("Genotyped %d of %d records: %s", summary["genotyped"], summary["records"], os.path.join(options.working_dir, "genotypes.vcf"))
    return 0


def entry():
    sys.exit(main())
