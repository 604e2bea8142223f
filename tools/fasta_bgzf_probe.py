"""bgzip-compressed genomes on the full-size sample: what the host and the device path of svx_fasta_fetch_batch cost.

  python tools/fasta_bgzf_probe.py OUT_DIR [--work DIR] [--runs 3] [--cohort 16]

Generates the full-size sample (tests/golden/full_inputs.json, as tests/test_full_golden.py does), bgzips its genome
twice (zlib level 6; libdeflate level 6, what `bgzip` writes when htslib has libdeflate) with 16 threads, then:
  * one in-process `svim-asm diploid` per genome form and path (plain; zlib-6 / libdeflate-6 on the host threads and on
    the device): the reference's counters split at the VCF phase (members inflated, cache / resident hits — on the device
    path the VCF phase's resident hits are the members it shares with PAIR —, bytes staged) and the PAIR-window and VCF
    fetch stages' wall and CPU seconds (SVIM_COMBINE.LAST_TIMING);
  * the fresh command (bin/svim-asm, a new process each time) with `ref.fa` and each `ref.fa.gz` form and path,
    interleaved, `--runs` times each: wall and CPU seconds (children's rusage);
  * `svim-asm-cohort diploid` over `--cohort` samples (the same BAMs) per genome form and path: samples per second.
Every VCF is compared with the plain genome's.  Writes OUT_DIR/fasta_bgzf_probe.json.
  python tools/fasta_bgzf_probe.py --one GENOME WD BAM1 BAM2   (the in-process run; prints one JSON line)
"""
import json
import os
import resource
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def one(genome, wd, bam1, bam2):
    from svim_asm_amd import SVIM_COMBINE, cli, fasta
    opened, marks = [], {}
    real_init, real_body = fasta.FastaFile.__init__, SVIM_COMBINE.vcf_body

    def init(self, *a, **k):
        real_init(self, *a, **k)
        opened.append(self)

    def body(table, types, reference, *a, **k):
        marks["before_vcf"] = reference.stats()
        return real_body(table, types, reference, *a, **k)
    fasta.FastaFile.__init__ = init
    SVIM_COMBINE.vcf_body = body
    t0, c0 = time.perf_counter(), time.process_time()
    cli.main(["diploid", wd, bam1, bam2, genome])
    wall, cpu = time.perf_counter() - t0, time.process_time() - c0
    end = opened[0].stats()
    pre = marks.get("before_vcf", {k: 0 for k in end})
    timing = {k: v for k, v in SVIM_COMBINE.LAST_TIMING.items() if "fetch" in k}
    print(json.dumps({"wall_s": wall, "cpu_s": cpu, "pair": pre, "vcf": {k: end[k] - pre[k] for k in end},
                      "compressed": opened[0].compressed, "timing": timing}))


def vcf_body_of(path):
    return "".join(l for l in open(path) if not l.startswith("##fileDate="))


def fresh(argv, env):
    r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.perf_counter()
    res = subprocess.run(argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    wall = time.perf_counter() - t0
    r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    if res.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (argv, res.stdout[-3000:]))
    return wall, (r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime), res.stdout


def main(argv):
    if argv and argv[0] == "--one":
        return one(*argv[1:5])
    out_dir = argv[0]
    opt = dict(zip(argv[1::2], argv[2::2]))
    work = opt.get("--work", os.path.join(out_dir, "work"))
    runs, n_cohort = int(opt.get("--runs", 3)), int(opt.get("--cohort", 16))
    os.makedirs(work, exist_ok=True)
    from svim_asm_amd import bamio, fasta, synth_bam
    from tools import e2e_bench
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "full_inputs.json")))
    prm = meta["params"]
    t0 = time.perf_counter()
    plain, bams = synth_bam.write_dataset(work, **e2e_bench.dataset_args(prm["scale"], prm["sv_per_mbp"], prm["mean_m"], prm["seed"]))
    report = {"generate_s": time.perf_counter() - t0, "forms": {}}
    genomes = {"plain": plain}
    for name, level in (("zlib6", 6), ("libdeflate6", 106)):
        if level >= 100 and bamio._libdeflate_compress(b"ACGT" * 64, 6) is None:
            continue
        gz = os.path.join(work, "ref.%s.fa.gz" % name)
        t0 = time.perf_counter()
        fasta.bgzip_fasta(plain, gz, level=level, threads=16)
        _, uoff = fasta.read_gzi(gz + ".gzi")
        genomes[name] = gz
        report["forms"][name] = {"bgzip_s": time.perf_counter() - t0, "members": int(len(uoff)) + 1,
                                 "bytes": os.path.getsize(gz), "plain_bytes": os.path.getsize(plain)}
    env0 = dict(os.environ)
    cases = [("plain", None)] + [(g, p) for g in genomes if g != "plain" for p in ("host", "device")]

    def env_of(path):
        e = dict(env0)
        if path:
            e["SVX_FASTA_DEVICE"] = "1" if path == "device" else "0"
        return e
    # in process: counters and fetch stages
    expected = None
    report["in_process"] = {}
    for g, p in cases:
        wd = os.path.join(work, "one_%s_%s" % (g, p))
        w, c, text = fresh([sys.executable, os.path.abspath(__file__), "--one", genomes[g], wd] + list(bams), env_of(p))
        rec = json.loads([l for l in text.splitlines() if l.startswith("{")][-1])
        body = vcf_body_of(os.path.join(wd, "variants.vcf"))
        expected = expected if expected is not None else body
        rec["vcf_equals_plain"] = body == expected
        report["in_process"]["%s/%s" % (g, p)] = rec
        print(g, p, json.dumps(rec), flush=True)
    # the fresh command, interleaved
    report["fresh"] = {"%s/%s" % c: {"wall_s": [], "cpu_s": []} for c in cases}
    for k in range(runs):
        for g, p in cases:
            wd = os.path.join(work, "fresh_%s_%s_%d" % (g, p, k))
            w, c, _ = fresh([os.path.join(ROOT, "bin", "svim-asm"), "diploid", wd] + list(bams) + [genomes[g]], env_of(p))
            r = report["fresh"]["%s/%s" % (g, p)]
            r["wall_s"].append(w)
            r["cpu_s"].append(c)
            r["vcf_equals_plain"] = r.get("vcf_equals_plain", True) and vcf_body_of(os.path.join(wd, "variants.vcf")) == expected
            print("fresh", g, p, k, round(w, 3), round(c, 3), flush=True)
    # the cohort
    report["cohort"] = {}
    for g, p in cases:
        d = os.path.join(work, "cohort_%s_%s" % (g, p))
        os.makedirs(d, exist_ok=True)
        manifest = os.path.join(d, "manifest.tsv")
        with open(manifest, "w") as fh:
            for s in range(n_cohort):
                fh.write("%s %s %s\n" % (os.path.join(d, "s%d" % s), bams[0], bams[1]))
        w, c, _ = fresh([os.path.join(ROOT, "bin", "svim-asm-cohort"), "diploid", manifest, genomes[g]], env_of(p))
        ok = all(vcf_body_of(os.path.join(d, "s%d" % s, "variants.vcf")) == expected for s in range(n_cohort))
        report["cohort"]["%s/%s" % (g, p)] = {"samples": n_cohort, "wall_s": w, "cpu_s": c, "samples_per_s": n_cohort / w,
                                              "vcf_equals_plain": ok}
        print("cohort", g, p, round(n_cohort / w, 2), round(c, 2), ok, flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "fasta_bgzf_probe.json"), "w") as fh:
        json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
