"""What PAF input costs next to SAM input on the same records, and what the oriented gather costs next to the plain one
(DESIGN.md §3.12).

    python tools/paf_probe.py [--ops 2500000] [--reps 3] [--out DIR] [--rocprof]

Two steps, each a child process under its own `timeout`; a step that fails ends the script:
  load     a haplotype's worth of CIGAR operations (svim_asm_amd.synth.synth_cigar_batch, the workload of
           tools/sam_probe.py) written once as a SAM (SEQ `*`) and once as a PAF with cg:Z:; bamio's load() +
           device_pool(wait=True) on a fresh handle each time, SAM and PAF, SVX_SAM_DEVICE=1 and =0, interleaved
  gather   a bgzip-compressed assembly, `--windows` windows of a few hundred bases: svx_fasta_fetch_batch (k_fasta_gather)
           and svx_fasta_fetch_oriented with no and with every window reversed (k_fasta_gather_oriented), members
           resident; wall time of the calls here, kernel time from `rocprofv3 --kernel-trace --stats` with --rocprof
Needs a GPU."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child_load(a):
    from svim_asm_amd import bamio, synth
    b = synth.synth_cigar_batch(seed=1, ops_target=a.ops)
    words, off = b["cigar"], b["aln_off"].astype(np.int64)
    letters = np.frombuffer(b"MIDNSHP=X", np.uint8)
    n = len(off) - 1
    d = tempfile.mkdtemp(prefix="paf_probe_")
    names = ["c%d" % k for k in range(len(b["contig_lengths"]))]
    lengths = [min(int(l), 2 ** 31 - 1) for l in b["contig_lengths"]]
    ref_span = np.add.reduceat(np.where(np.isin(words & 15, (0, 2, 3, 7, 8)), words >> 4, 0).astype(np.int64), off[:-1])
    for i in range(n):  # (the synthetic records may run past their contig's nominal end: a PAF row must not)
        lengths[int(b["tid"][i])] = max(lengths[int(b["tid"][i])], int(b["ref_start"][i]) + int(ref_span[i]))
    assert max(lengths) < 2 ** 31
    order = np.random.default_rng(1).permutation(n)
    sam, paf, ref, qfa = (os.path.join(d, x) for x in ("probe.sam", "probe.paf", "ref.fa", "q.fa"))
    with open(ref + ".fai", "w") as f:
        f.write("".join("%s\t%d\t0\t60\t61\n" % (nm, l) for nm, l in zip(names, lengths)))
    with open(qfa, "w") as f:
        f.write(">none\nA\n")
    with open(qfa + ".fai", "w") as f:
        f.write("none\t1\t6\t1\t2\n")
    with open(sam, "w") as fs, open(paf, "w") as fp:
        fs.write("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, l) for nm, l in zip(names, lengths)))
        for i in order.tolist():
            w = words[off[i]:off[i + 1]]
            ln, op = (w >> 4).astype(np.int64), w & 15
            text = "".join("%d%s" % (l, chr(o)) for l, o in zip(ln.tolist(), letters[op].tolist()))
            q = int(ln[np.isin(op, (0, 1, 4, 7, 8))].sum())
            t = int(ln[np.isin(op, (0, 2, 3, 7, 8))].sum())
            tid, ts = int(b["tid"][i]), int(b["ref_start"][i])
            assert ts + t <= lengths[tid]
            fs.write("q%d\t0\t%s\t%d\t60\t%s\t*\t0\t0\t*\t*\n" % (i, names[tid], ts + 1, text))
            fp.write("q%d\t%d\t0\t%d\t+\t%s\t%d\t%d\t%d\t%d\t%d\t60\ttp:A:P\tcg:Z:%s\n"
                     % (i, q, q, names[tid], lengths[tid], ts, ts + t, min(q, t), max(q, t), text))

    def load(path, device_parse):
        os.environ["SVX_SAM_DEVICE"] = "1" if device_parse else "0"
        kw = {"query": qfa, "reference": ref} if path is paf else {}
        f = bamio.AlignmentFile(path, device=0, threads=a.threads, **kw)
        t0 = time.perf_counter()
        f.load()
        f.device_pool(wait=True)
        ms = (time.perf_counter() - t0) * 1e3
        assert f.parsed_on_device == bool(device_parse) and len(f._cigar) == len(words)
        got = (f._cigar.copy(), f._cols["pos"].copy(), f._cols["ref_len"].copy())
        f.close()
        return ms, got

    cases = [("sam_device", sam, 1), ("sam_threads", sam, 0), ("paf_device", paf, 1), ("paf_threads", paf, 0)]
    first = {k: load(p, dp)[1] for k, p, dp in cases}  # (first touches: pages, streams, code objects)
    for k in first:
        assert all(np.array_equal(x, y) for x, y in zip(first[k], first["sam_threads"])), k  # PAF against SAM, same records
    res = {k: [] for k, _, _ in cases}
    for _ in range(a.reps):
        for k, p, dp in cases:
            res[k].append(load(p, dp)[0])
    table = {"step": "load", "ops": int(len(words)), "records": int(n), "sam_bytes": os.path.getsize(sam), "paf_bytes": os.path.getsize(paf),
             "threads": a.threads, "median_ms": {k: round(statistics.median(v), 3) for k, v in res.items()},
             "all_ms": {k: [round(x, 3) for x in v] for k, v in res.items()}}
    print(json.dumps(table), flush=True)
    shutil.rmtree(d)


def child_gather(a):
    from svim_asm_amd import fasta
    rng = np.random.default_rng(2)
    d = tempfile.mkdtemp(prefix="paf_probe_")
    n_ctg, ctg_len = 16, a.assembly_mb * (1 << 20) // 16
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ctg_len)] for _ in range(n_ctg)]
    names = ["ctg%d" % k for k in range(n_ctg)]
    path = fasta.write_bgzf_fasta(os.path.join(d, "asm.fa.gz"), names, seqs, level=1, threads=16)
    os.environ["SVX_FASTA_DEVICE"] = "1"
    f = fasta.FastaFile(path, device=0)
    n = a.windows
    ctg = [names[k] for k in rng.integers(0, n_ctg, n).tolist()]
    start = rng.integers(0, ctg_len - 2000, n)
    end = start + rng.integers(50, 1000, n)
    none, every = np.zeros(n, bool), np.ones(n, bool)
    calls = {"plain_gather": lambda: f.fetch_batch(ctg, start, end, upper=True),
             "oriented_forward": lambda: f.fetch_oriented(ctg, start, end, none),
             "oriented_reversed": lambda: f.fetch_oriented(ctg, start, end, every)}
    out = {k: fn()[0] for k, fn in calls.items()}  # (the first call inflates every member under the windows: resident from here on)
    assert np.array_equal(out["plain_gather"], out["oriented_forward"]) and f.stats()["device_calls"] == 3
    res = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            res[k].append((time.perf_counter() - t0) * 1e3)
    table = {"step": "gather", "windows": n, "bases": int(len(out["plain_gather"])), "assembly_bytes": n_ctg * ctg_len,
             "calls_per_kind": a.reps + 1, "stats": f.stats(),
             "median_call_ms": {k: round(statistics.median(v), 3) for k, v in res.items()},
             "all_call_ms": {k: [round(x, 3) for x in v] for k, v in res.items()}}
    print(json.dumps(table), flush=True)
    f.close()
    shutil.rmtree(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=2_500_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--windows", type=int, default=60000)
    ap.add_argument("--assembly_mb", type=int, default=128)
    ap.add_argument("--out", help="directory for the two tables (and rocprofv3's files)")
    ap.add_argument("--rocprof", action="store_true", help="run the gather step under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--child", choices=["load", "gather"])
    ap.add_argument("--step_timeout", type=int, default=420)
    a = ap.parse_args()
    if a.child:
        return {"load": child_load, "gather": child_gather}[a.child](a)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    common = ["--ops", str(a.ops), "--reps", str(a.reps), "--threads", str(a.threads), "--windows", str(a.windows),
              "--assembly_mb", str(a.assembly_mb)]
    for step in ("load", "gather"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step] + common
        if step == "gather" and a.rocprof:
            trace = os.path.join(a.out or tempfile.mkdtemp(prefix="paf_probe_trace_"), "rocprof")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--"] + cmd
        res = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:  # nothing more is started on the device behind a step that failed
            sys.exit("paf_probe: step %s ended with status %d" % (step, res.returncode))
        if a.out:
            lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
            if lines:
                open(os.path.join(a.out, "paf_probe_%s.json" % step), "w").write(lines[-1] + "\n")


if __name__ == "__main__":
    main()
