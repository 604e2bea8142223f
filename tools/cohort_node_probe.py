#!/usr/bin/env python3
"""What `svim-asm-cohort --gpus N` costs and gains on ONE device: the plain single-process command of another tree (the
commit before the launcher: --baseline) against this tree's `--gpus 1`, `--gpus 2 --devices 0,0` and `--gpus 4 --devices
0,0,0,0` on N own copies of the full-size synthetic sample (tools/e2e_bench.py's, scale 1.0), the runs interleaved (their
order rotated from one repetition to the next), three repetitions each, medians and spreads reported.

    python tools/cohort_node_probe.py --baseline OTHER_TREE/bin/svim-asm-cohort [--samples 16] [--reps 3] [--out FILE]

Every run is a fresh process under a time limit of its own; the first run that fails, times out or writes a VCF that is
not the reference's ends the probe (nothing further is started on the device).  This process never touches the GPU.  Per
run: samples per second over the command's wall-clock, CPU-seconds per sample (the command and everything it started),
the time the cgroup was throttled meanwhile (cpu.stat), and beside them the threads the processes of that configuration
planned together (P x workers x readers x threads per reader, from the same functions the command uses).  One JSON line per
run and a summary line at the end; --out appends them to a file."""
import argparse
import hashlib
import json
import os
import resource
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def throttled_us():
    """Microseconds the cgroup has throttled this process's group so far (cpu.stat), None where that is not exposed."""
    for path, key, scale in (("/sys/fs/cgroup/cpu.stat", "throttled_usec", 1.0),
                             ("/sys/fs/cgroup/cpu/cpu.stat", "throttled_time", 1e-3)):
        try:
            with open(path) as fh:
                for line in fh:
                    parts = line.split()
                    if len(parts) == 2 and parts[0] == key:
                        return float(parts[1]) * scale
        except OSError:
            pass
    return None


def planned(processes, n_samples):
    """What `processes` cohort processes of this tree plan together for a diploid manifest of `n_samples`."""
    from svim_asm_amd import bamio, cohort
    cpus = bamio.process_cpus(processes)
    workers = max(1, min(cohort.default_workers(cpus), -(-n_samples // processes)))
    threads = cohort.default_reader_threads(workers, 2, cpus)
    return {"processes": processes, "cpus_per_process": cpus, "workers": workers, "threads_per_reader": threads,
            "lanes": cohort.default_lanes(workers, 2), "reader_threads_all_processes": processes * workers * 2 * threads,
            "device_leg_default_percent": bamio.default_device_inflate_percent(cpus)}


def run_limited(argv, env, limit):
    """(status, output) of a fresh process in a session of its own; past `limit` seconds SIGTERM — which the launcher passes
    on to its children —, ten seconds later SIGKILL for whatever the session still holds: status 124."""
    import signal
    p = subprocess.Popen(argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        text = p.communicate(timeout=limit)[0]
        return p.returncode, text
    except subprocess.TimeoutExpired:
        p.terminate()
        try:
            text = p.communicate(timeout=10)[0]
        except subprocess.TimeoutExpired:
            text = ""
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except (ProcessLookupError, PermissionError):
            pass
        p.wait()
        return 124, text or ""


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline", required=True, help="bin/svim-asm-cohort of the tree to compare with (built)")
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dataset", default=None, help="directory holding ref.fa / hap1.bam / hap2.bam of an earlier run")
    ap.add_argument("--timeout", type=int, default=120, help="seconds one run may take")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    from tools import e2e_bench
    from svim_asm_amd import bamio, synth_bam

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    work = tempfile.mkdtemp(prefix="svx_node_probe_")
    try:
        t0 = time.perf_counter()
        if args.dataset:
            fasta, bams = os.path.join(args.dataset, "ref.fa"), [os.path.join(args.dataset, "hap%d.bam" % k) for k in (1, 2)]
        else:
            fasta, bams = synth_bam.write_dataset(os.path.join(work, "sample"), level=1, **e2e_bench.dataset_args(args.scale))
        _, meta = e2e_bench.reference_meta(args.scale, 8.0, 2000)
        dirs = []
        for k in range(args.samples):  # own copies of the BAMs (no shared page-cache pages), the genome shared as in a real cohort
            d = os.path.join(work, "copy_%d" % k)
            os.makedirs(d)
            for src in list(bams) + [b + ".bai" for b in bams]:
                shutil.copyfile(src, os.path.join(d, os.path.basename(src)))
            dirs.append(d)
        manifest = os.path.join(work, "manifest.txt")
        with open(manifest, "w") as f:
            for d in dirs:
                f.write("%s %s %s\n" % (os.path.join(d, "wd"), os.path.join(d, "hap1.bam"), os.path.join(d, "hap2.bam")))
        emit({"what": "setup", "samples": args.samples, "scale": args.scale, "bam_bytes": [os.path.getsize(b) for b in bams],
              "setup_s": time.perf_counter() - t0, "cpu_quota_cpus": e2e_bench.cpu_quota(), "host_cpus": bamio.host_cpus(),
              "hardware_threads": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)),
              "vcf_checked_against": "the real reference's digest" if meta else "the first VCF of the first run"})
        this = os.path.join(ROOT, "bin", "svim-asm-cohort")
        configs = [("baseline", args.baseline, [], 1), ("gpus1", this, ["--gpus", "1"], 1),
                   ("gpus2", this, ["--gpus", "2", "--devices", "0,0"], 2),
                   ("gpus4", this, ["--gpus", "4", "--devices", "0,0,0,0"], 4)]
        env = dict(os.environ)
        for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "SVX_NODE_PROCESSES"):
            env.pop(name, None)
        runs, first_vcf = {name: [] for name, _, _, _ in configs}, [None]

        def vcf_ok(path):
            if not os.path.exists(path):
                return False
            text = e2e_bench.masked(path).encode()
            if meta:
                return hashlib.sha256(text).hexdigest() == meta["vcf_sha256"] and len(text) == meta["vcf_bytes"]
            first_vcf[0] = first_vcf[0] or text
            return text == first_vcf[0]

        for rep in range(args.reps):
            # interleaved — every configuration sees the same drift of the box — and rotated: none of them always runs
            # behind the same neighbour (the run behind the throttled four-process one was the slow one when it always was
            # the baseline)
            for name, script, extra, processes in configs[rep % len(configs):] + configs[:rep % len(configs)]:
                for d in dirs:
                    shutil.rmtree(os.path.join(d, "wd"), ignore_errors=True)
                ru0, thr0, t0 = resource.getrusage(resource.RUSAGE_CHILDREN), throttled_us(), time.perf_counter()
                rc, text = run_limited([sys.executable, script, "diploid", manifest, fasta] + extra, env, args.timeout)
                wall, thr1, ru1 = time.perf_counter() - t0, throttled_us(), resource.getrusage(resource.RUSAGE_CHILDREN)
                cpu = (ru1.ru_utime + ru1.ru_stime) - (ru0.ru_utime + ru0.ru_stime)
                oks = [vcf_ok(os.path.join(d, "wd", "variants.vcf")) for d in dirs]
                rec = {"what": "run", "config": name, "rep": rep, "rc": rc, "wall_s": wall, "samples_per_s": args.samples / wall,
                       "cpu_seconds_per_sample": cpu / args.samples,
                       "throttled_s": None if thr0 is None or thr1 is None else (thr1 - thr0) * 1e-6,
                       "vcfs_ok": sum(1 for o in oks if o), "planned": planned(processes, args.samples),
                       "budget_lines": [l.split("BUDGET: ", 1)[1] for l in text.split("\n") if "BUDGET: " in l]}
                if rc != 0 or not all(oks):
                    rec["output_tail"] = text[-3000:]
                emit(rec)
                if rc != 0 or not all(oks):
                    emit({"what": "stopped", "why": "%s failed in repetition %d: nothing further is started" % (name, rep)})
                    return 1
                runs[name].append(rec)
        summary = {"what": "summary", "samples": args.samples, "reps": args.reps, "date": time.strftime("%Y-%m-%d")}
        for name, _, _, _ in configs:
            summary[name] = {k: {"median": statistics.median(r[k] for r in runs[name]), "min": min(r[k] for r in runs[name]),
                                 "max": max(r[k] for r in runs[name])}
                             for k in ("samples_per_s", "cpu_seconds_per_sample", "throttled_s") if runs[name][0][k] is not None}
            summary[name]["planned"] = runs[name][0]["planned"]
        base = summary["baseline"]["samples_per_s"]
        summary["baseline_spread_samples_per_s"] = base["max"] - base["min"]
        summary["gpus1_median_minus_baseline_median"] = summary["gpus1"]["samples_per_s"]["median"] - base["median"]
        summary["gpus1_within_baseline_spread"] = \
            summary["gpus1"]["samples_per_s"]["median"] >= base["median"] - summary["baseline_spread_samples_per_s"]
        emit(summary)
        return 0
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
