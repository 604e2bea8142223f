"""`svim-asm-merge`: the final tables of a cohort's samples (candidates.svxt, written with --keep_candidates) merged into
one VCF with a genotype column per sample (SVIM_MERGE.py).

    svim-asm-merge OUT_DIR GENOME SAMPLE_DIR [SAMPLE_DIR ...] [options]
    svim-asm-merge OUT_DIR GENOME --manifest MANIFEST [options]

MANIFEST: a cohort manifest (svim-asm-cohort); its first column names the sample directories.  A sample's column is
named after its directory; the records go to OUT_DIR/cohort.vcf (cohort.vcf.gz and its index with --bgzip_output).

With --genotype_non_carriers a sample without a call in a record is genotyped per haplotype from the coverage its run
kept (coverage.svxt, written with --keep_coverage): 0 where one alignment of the haplotype's assembly spans the record's
window, . where none does.

With --callable_bed the same files give OUT_DIR/cohort.callable.bed: contig, start, end and the number of samples whose
own callable set — the ranges exactly one alignment per haplotype lies over — contains the range."""
import argparse
import logging
import os
import sys

from svim_asm_amd import SVIM_CALLABLE, SVIM_MERGE
from svim_asm_amd.fasta import BgzfFormatError, FastaFile, MissingGziError

__version__ = "1.0.3"


def parse(argv):
    p = argparse.ArgumentParser(prog="svim-asm-merge", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("working_dir", metavar="OUT_DIR", type=os.path.abspath, help="Output directory (created if missing)")
    p.add_argument("genome", metavar="GENOME", help="Reference genome FASTA the samples were called against (indexed with .fai)")
    p.add_argument("sample_dirs", metavar="SAMPLE_DIR", nargs="*", help="Working directories of the samples, in column order")
    p.add_argument("--manifest", default=None, help="Cohort manifest: its first column gives the sample directories")
    p.add_argument("--partition_max_distance", type=int, default=1000, help="Maximum distance in bp between SVs in a partition")
    p.add_argument("--max_edit_distance", type=int, default=200, help="Maximum edit distance between alleles of one record")
    p.add_argument("--merge_max_partition", type=int, default=SVIM_MERGE.DEFAULT_MAX_PARTITION,
                   help="Partitions of more distinct alleles than this are left unclustered (bounds the quadratic work)")
    p.add_argument("--types", type=str, default="DEL,INS,INV,DUP:TANDEM,DUP:INT,BND", help="SV types to include, comma-separated")
    p.add_argument("--symbolic_alleles", action="store_true", help="Use symbolic alleles such as <DEL>")
    p.add_argument("--tandem_duplications_as_insertions", action="store_true", help="Represent tandem duplications as insertions")
    p.add_argument("--interspersed_duplications_as_insertions", action="store_true",
                   help="Represent interspersed duplications as insertions")
    p.add_argument("--genotype_non_carriers", action="store_true",
                   help="Genotype the samples without a call per haplotype (0 or .) from their coverage.svxt (--keep_coverage)")
    p.add_argument("--genotype_margin", type=int, default=None,
                   help="Bases on either side of a record an alignment has to span (default: --partition_max_distance)")
    p.add_argument("--callable_bed", action="store_true",
                   help="Also write cohort.callable.bed: the ranges exactly one alignment per haplotype lies over, with the number "
                        "of samples, from the samples' coverage.svxt (--keep_coverage)")
    p.add_argument("--callable_min_length", type=int, default=0,
                   help="Alignments with fewer reference bases than this are left out of --callable_bed (default: 0, none)")
    p.add_argument("--bgzip_output", action="store_true", help="Write cohort.vcf.gz and its tabix index instead of cohort.vcf")
    p.add_argument("--device", type=int, default=0, help="HIP device index of the GPU to use")
    p.add_argument("--verbose", action="store_true", help="Enable more verbose logging")
    return p.parse_args(argv)


def sample_dirs_of(options):
    dirs = [os.path.abspath(d) for d in options.sample_dirs]
    if options.manifest is not None:
        if dirs:
            raise ValueError("give the sample directories or --manifest, not both")
        for line in open(options.manifest):
            fields = line.split()
            if fields and not fields[0].startswith("#"):
                dirs.append(os.path.abspath(fields[0]))
    if not dirs:
        raise ValueError("no sample directory given")
    names = [os.path.basename(d.rstrip(os.sep)) for d in dirs]
    seen = {}
    for d, name in zip(dirs, names):
        if name in seen:
            raise ValueError("two samples would share the column name %s: %s and %s" % (name, seen[name], d))
        seen[name] = d
    return dirs, names


def main(argv=None):
    options = parse(list(sys.argv[1:] if argv is None else argv))
    try:
        dirs, names = sample_dirs_of(options)  # (before any work)
    except (ValueError, OSError) as e:
        print("svim-asm-merge: %s" % e, file=sys.stderr)
        return 2
    logging.getLogger().setLevel(logging.DEBUG if options.verbose else logging.INFO)
    if not logging.getLogger().handlers:
        logging.basicConfig(format="%(asctime)s [%(levelname)-7.7s]  %(message)s")
    os.makedirs(options.working_dir, exist_ok=True)
    try:
        tables = [SVIM_MERGE.read_candidates(d) for d in dirs]
        SVIM_MERGE.check_same_contigs(tables, names)
        coverages = [SVIM_MERGE.read_coverage(d) for d in dirs] if options.genotype_non_carriers or options.callable_bed else None
        SVIM_CALLABLE.check_min_length(options)
        if options.genotype_margin is not None and options.genotype_margin < 0:
            raise ValueError("--genotype_margin %d: a number of bases, 0 or more" % options.genotype_margin)
    except ValueError as e:
        logging.error("%s", e)
        return 1
    try:
        reference = FastaFile(options.genome, device=options.device)
    except (MissingGziError, BgzfFormatError, ValueError, IOError) as e:
        logging.error("The given reference genome cannot be used (%s: %s).", options.genome, e)
        return 1
    logging.info("****************** MERGE: %d samples, %d candidates ******************", len(tables), sum(len(t) for t in tables))
    options.query_names = False
    merged, genotypes = SVIM_MERGE.merge_tables(tables, names, reference, options)
    types_to_output = [entry.strip() for entry in options.types.split(",")]
    covered = None
    if options.genotype_non_carriers:
        try:
            covered = SVIM_MERGE.genotype_non_carriers(merged, coverages, options, sample_names=names)
        except ValueError as e:
            logging.error("%s", e)
            return 1
    if options.callable_bed:
        try:
            SVIM_MERGE.check_coverage_contigs(merged, coverages, names)
            bed = SVIM_CALLABLE.write_cohort_bed(merged.contigs, coverages, options, options.working_dir, sample_names=names)
        except ValueError as e:
            logging.error("%s", e)
            return 1
    path = SVIM_MERGE.write_cohort_vcf(merged, genotypes, names, __version__, types_to_output, reference, options, C=covered)
    logging.info("%d records of %d samples: %s", len(merged), len(names), path)
    if options.callable_bed:
        logging.info("callable ranges of %d samples: %s", len(names), bed)
    return 0


def entry():
    sys.exit(main())
