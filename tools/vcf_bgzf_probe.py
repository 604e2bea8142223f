"""`--bgzip_output` on the full-size sample: what the device and the host BGZF path cost.

  python tools/vcf_bgzf_probe.py OUT_DIR [--work DIR] [--runs 3] [--cohort 16]

Generates the full-size sample (tests/golden/full_inputs.json, as tests/test_full_golden.py does), then:
  * the fresh command (bin/svim-asm diploid, a new process each time) plain, with --bgzip_output on the device
    (SVX_VCF_BGZF_DEVICE=1) and on the host threads (=0), interleaved, `--runs` times each: wall and CPU seconds
    (children's rusage), medians;
  * the encoder alone on the plain run's text: kernel milliseconds (svx_ctx_last_kernel_ms), upload / download and
    whole-call seconds, the host path's seconds, and the compressed sizes against zlib levels 1 and 6 over the same blocks;
  * `svim-asm-cohort diploid` over `--cohort` samples (the same BAMs) with and without the option: samples per second.
Every decompressed VCF is compared with the plain one (##fileDate masked).  Writes OUT_DIR/vcf_bgzf_probe.json.
"""
import gzip
import json
import os
import resource
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def masked(data):
    return b"".join(l for l in data.splitlines(keepends=True) if not l.startswith(b"##fileDate="))


def fresh(argv, env):
    r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.perf_counter()
    res = subprocess.run(argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    w = time.perf_counter() - t0
    r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    if res.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (argv, res.stdout[-3000:]))
    return w, (r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime)


def zlib_size(data, level):
    total = 0
    for k in range(0, len(data), 65280):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += 26 + len(c.compress(data[k:k + 65280]) + c.flush())
    return total + 28


def main(argv):
    out_dir = argv[0]
    opt = dict(zip(argv[1::2], argv[2::2]))
    runs, n_cohort = int(opt.get("--runs", 3)), int(opt.get("--cohort", 16))
    work = opt.get("--work") or os.path.join(out_dir, "work")
    os.makedirs(work, exist_ok=True)
    from svim_asm_amd import synth_bam
    from tools import e2e_bench
    prm = json.load(open(os.path.join(ROOT, "tests", "golden", "full_inputs.json")))["params"]
    fasta, bams = synth_bam.write_dataset(work, **e2e_bench.dataset_args(prm["scale"], prm["sv_per_mbp"], prm["mean_m"], prm["seed"]))
    cli = os.path.join(ROOT, "bin", "svim-asm")
    forms = {"plain": ([], None), "device": (["--bgzip_output"], "1"), "host": (["--bgzip_output"], "0")}

    def env_of(dev):
        env = dict(os.environ)
        env.pop("SVX_VCF_BGZF_DEVICE", None)
        if dev is not None:
            env["SVX_VCF_BGZF_DEVICE"] = dev
        return env
    report = {"runs": runs, "fresh": {f: {"wall_s": [], "cpu_s": []} for f in forms}}
    texts = {}
    for r in range(runs):
        for f, (extra, dev) in forms.items():
            wd = os.path.join(work, "fresh_%s" % f)
            w, c = fresh([cli, "diploid", wd, bams[0], bams[1], fasta] + extra, env_of(dev))
            report["fresh"][f]["wall_s"].append(w)
            report["fresh"][f]["cpu_s"].append(c)
            print("fresh", f, round(w, 3), round(c, 3), flush=True)
            if r == 0:
                path = os.path.join(wd, "variants.vcf" + (".gz" if extra else ""))
                data = open(path, "rb").read()
                texts[f] = masked(gzip.decompress(data) if extra else data)
                if extra:
                    report["fresh"][f]["compressed_bytes"] = len(data)
                    report["fresh"][f]["index_bytes"] = os.path.getsize(path + ".tbi")
    for f in forms:
        for k in ("wall_s", "cpu_s"):
            report["fresh"][f]["median_" + k] = statistics.median(report["fresh"][f][k])
    report["same_text"] = texts["device"] == texts["plain"] and texts["host"] == texts["plain"]
    for f in ("device", "host"):
        report["added_over_plain_" + f] = {k: report["fresh"][f]["median_" + k] - report["fresh"]["plain"]["median_" + k]
                                           for k in ("wall_s", "cpu_s")}
    # the encoder alone
    from svim_asm_amd import _lib, vcf_bgzf
    text = open(os.path.join(work, "fresh_plain", "variants.vcf"), "rb").read()
    ctx = _lib.Context(0)
    ctx.bgzf_deflate(text)  # (first call: workspace, code object)
    enc = {"text_bytes": len(text), "device_calls_s": [], "kernel_ms": [], "host_calls_s": [], "host_cpu_s": []}
    for _ in range(5):
        ctx.set_timing(True)
        t0 = time.perf_counter()
        blob, _ = ctx.bgzf_deflate(text)
        enc["device_calls_s"].append(time.perf_counter() - t0)
        enc["kernel_ms"].append(ctx.last_kernel_ms()[0])
        ctx.set_timing(False)
        c0, t0 = time.process_time(), time.perf_counter()
        hblob, _ = vcf_bgzf.compress(text)
        enc["host_calls_s"].append(time.perf_counter() - t0)
        enc["host_cpu_s"].append(time.process_time() - c0)
    d_in = ctx.dev_array(nbytes=len(text))
    t0 = time.perf_counter()
    lib = _lib.load()
    import numpy as np
    src = np.frombuffer(text, np.uint8)
    for _ in range(5):
        lib.svx_dev_upload(ctx.h, d_in.ptr, src.ctypes.data, len(text))
    ctx.sync()
    enc["upload_s"] = (time.perf_counter() - t0) / 5
    dst = np.empty(len(blob), np.uint8)
    t0 = time.perf_counter()
    for _ in range(5):
        lib.svx_dev_download(ctx.h, dst.ctypes.data, d_in.ptr, len(blob))
    enc["download_s"] = (time.perf_counter() - t0) / 5
    d_in.free()
    enc.update({"device_bytes": len(blob), "host_bytes": len(hblob), "zlib1_bytes": zlib_size(text, 1),
                "zlib6_bytes": zlib_size(text, 6)})
    enc["device_over_zlib6"] = len(blob) / enc["zlib6_bytes"]
    enc["device_over_zlib1"] = len(blob) / enc["zlib1_bytes"]
    enc["device_equals_text"] = gzip.decompress(blob) == text
    report["encoder"] = enc
    print("encoder", json.dumps({k: v for k, v in enc.items() if not isinstance(v, list)}), flush=True)
    # the cohort
    report["cohort"] = {}
    for f, (extra, dev) in (("plain", forms["plain"]), ("device", forms["device"])):
        d = os.path.join(work, "cohort_%s" % f)
        os.makedirs(d, exist_ok=True)
        manifest = os.path.join(d, "manifest.tsv")
        with open(manifest, "w") as fh:
            for s in range(n_cohort):
                fh.write("%s %s %s\n" % (os.path.join(d, "s%d" % s), bams[0], bams[1]))
        w, c = fresh([os.path.join(ROOT, "bin", "svim-asm-cohort"), "diploid", manifest, fasta] + extra, env_of(dev))
        name = "variants.vcf" + (".gz" if extra else "")
        ok = all(masked(gzip.decompress(open(os.path.join(d, "s%d" % s, name), "rb").read()) if extra else
                        open(os.path.join(d, "s%d" % s, name), "rb").read()) == texts["plain"] for s in range(n_cohort))
        report["cohort"][f] = {"samples": n_cohort, "wall_s": w, "cpu_s": c, "samples_per_s": n_cohort / w, "same_text": ok}
        print("cohort", f, round(n_cohort / w, 2), round(c, 2), ok, flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "vcf_bgzf_probe.json"), "w") as fh:
        json.dump(report, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
