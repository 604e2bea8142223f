"""`svim-asm-small`: SNVs and small indels from an assembly's alignments (SVIM_SMALL.py).

    svim-asm-small OUT_DIR GENOME HAP1 [HAP2] [options]

HAP1 and HAP2 are the alignments of the sample's haplotype assemblies to GENOME (BAM, SAM, or PAF with --query1 /
--query2).  Every aligned column that differs from the reference and every inserted or deleted run shorter than
--min_sv_size becomes a record where exactly one alignment of its haplotype lies over it; the aligner's placement of an
indel stands unless --left_align is given, which shifts each one leftmost on the device, so that two assemblies that
place the same indel differently give one record.  OUT_DIR gets small.vcf (one sample column, GT phased: haplotype 1 | haplotype 2; small.vcf.gz and its index
with --bgzip_output) and summary.json."""
import argparse
import logging
import os
import sys

from svim_asm_amd import SVIM_SMALL
from svim_asm_amd.fasta import BgzfFormatError, FastaFile, MissingGziError


def parse(argv):
    p = argparse.ArgumentParser(prog="svim-asm-small", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("working_dir", metavar="OUT_DIR", type=os.path.abspath, help="Output directory (created if missing)")
    p.add_argument("genome", metavar="GENOME", help="Reference genome FASTA the alignments refer to (indexed with .fai)")
    p.add_argument("hap1", metavar="HAP1", help="Alignments of the first haplotype's assembly (BAM, SAM, or PAF with --query1)")
    p.add_argument("hap2", metavar="HAP2", nargs="?", default=None, help="Alignments of the second haplotype's assembly")
    p.add_argument("--query1", default=None, help="Assembly FASTA of HAP1 when it is a PAF")
    p.add_argument("--query2", default=None, help="Assembly FASTA of HAP2 when it is a PAF")
    p.add_argument("--sample", default="Sample", help="Name of the sample column (default: %(default)s)")
    p.add_argument("--min_mapq", type=int, default=20, help="Alignments below this mapping quality are ignored (default: %(default)s)")
    p.add_argument("--min_sv_size", type=int, default=40,
                   help="Insertions and deletions of this size or more are left to svim-asm (default: %(default)s)")
    p.add_argument("--batch_bases", type=int, default=1 << 28,
                   help="Most reference plus assembly bases compared in one device call (default: %(default)s)")
    p.add_argument("--left_align", action="store_true",
                   help="Move every insertion and deletion shorter than --min_sv_size as far to the left as its bases allow, "
                        "never past another gap of its alignment (default: the aligner's placement stands)")
    p.add_argument("--bgzip_output", action="store_true", help="Write small.vcf.gz and its tabix index instead of small.vcf")
    p.add_argument("--no_bgzf_crc", action="store_true", help="Do not check the CRC32 of the BGZF members of a BAM")
    p.add_argument("--device", type=int, default=0, help="HIP device index of the GPU to use")
    p.add_argument("--verbose", action="store_true", help="Enable more verbose logging")
    return p.parse_args(argv)


def check(options):
    """Argument errors, before any work."""
    if options.min_mapq < 0:
        raise ValueError("--min_mapq %d: 0 or more" % options.min_mapq)
    for name in ("min_sv_size", "batch_bases"):
        if getattr(options, name) < 1:
            raise ValueError("--%s %d: 1 or more" % (name, getattr(options, name)))
    for path in (options.hap1, options.hap2, options.query1, options.query2):
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
        print("svim-asm-small: %s" % e, file=sys.stderr)
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
        summary = SVIM_SMALL.small(reference, files, options, options.working_dir)
    except (ValueError, IOError) as e:
        logging.error("%s", e)
        return 1
    for h, counts in enumerate(summary["haplotypes"]):
        logging.info("Haplotype %d: %s", h + 1, ", ".join("%s %d" % kv for kv in counts.items()))
    logging.info("%d records (%s): %s", summary["records"], ", ".join("%s %d" % kv for kv in summary["by_type"].items()),
                 os.path.join(options.working_dir, "small.vcf.gz" if options.bgzip_output else "small.vcf"))
    return 0


def entry():
    sys.exit(main())
