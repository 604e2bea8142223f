#!/usr/bin/env python3
"""What the lift-over of svim-asm-genotype costs (svx_cigar_lift), and where one genotyping run spends
its time.

    python tools/lift_probe.py [--ops 5000000] [--queries 250000] [--sites 60000] [--reps 5] [--out profiles/lift_probe.json]

Synthetic and seeded.  The lift: a pool of `--ops` CIGAR ops in alignments of 1000 ops (matches, small indels, a clip
at either end) and `--queries` positions spread over them, a few in front of and behind their alignment.  Timed:
Context.cigar_lift — the uploads, four kernels, the read-back, a host clock around a call that ends in a synchronise —
as the median of `--reps` calls after one untimed call; beside it the kernels' milliseconds from HIP events, and the same
batch on the host with numpy (cumsum + searchsorted per alignment), timed the same way.  The two answers must be equal.
The run: SVIM_GENOTYPE.genotype over `--sites` made-up deletions and insertions on the contigs of tests/golden/config1
against its two haplotype BAMs, once, seconds by phase.  No real cohort or truth set is genotyped here.  No target: the
numbers are what they are."""
import argparse
import datetime
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svim_asm_amd import _lib  # noqa: E402

M, I, D, S = 0, 1, 2, 4
REF_OPS = np.array([1, 0, 1, 1, 0, 0, 0, 1, 1] + [0] * 7, dtype=np.int64)
QRY_OPS = np.array([1, 1, 0, 0, 1, 0, 0, 1, 1] + [0] * 7, dtype=np.int64)


def synthetic_batch(n_ops, n_queries, per_alignment=1000, seed=21):
    rng = np.random.default_rng(seed)
    n_aln = max(1, n_ops // per_alignment)
    n_ops = n_aln * per_alignment
    op = np.where(np.arange(n_ops) % 2 == 0, M, rng.choice([I, D], n_ops)).astype(np.uint32)
    length = np.where(op == M, rng.integers(20, 400, n_ops), rng.integers(1, 60, n_ops)).astype(np.uint32)
    first, last = np.arange(n_aln) * per_alignment, np.arange(n_aln) * per_alignment + per_alignment - 1
    op[first], op[last] = S, S
    cigar = (length << np.uint32(4)) | op
    aln_off = (np.arange(n_aln + 1, dtype=np.uint64) * np.uint64(per_alignment))
    ref_start = rng.integers(0, 1 << 27, n_aln).astype(np.int32)
    ref_len = np.add.reduceat(length.astype(np.int64) * REF_OPS[op], first)
    q_aln = rng.integers(0, n_aln, n_queries).astype(np.uint32)
    q_ref = ref_start[q_aln].astype(np.int64) + (rng.random(n_queries) * (ref_len[q_aln] + 40)).astype(np.int64) - 20
    return cigar, aln_off, ref_start, q_aln, q_ref


def on_host(cigar, aln_off, ref_start, q_aln, q_ref):
    query, state = np.zeros(len(q_aln), np.uint32), np.zeros(len(q_aln), np.uint8)
    order = np.argsort(q_aln, kind="stable")
    cut = np.searchsorted(q_aln[order], np.arange(len(aln_off)))
    for a in range(len(aln_off) - 1):
        qs = order[cut[a]:cut[a + 1]]
        if not len(qs):
            continue
        w = cigar[int(aln_off[a]):int(aln_off[a + 1])]
        op, n = (w & 15).astype(np.int64), (w >> 4).astype(np.int64)
        p_ref, p_qry = np.cumsum(n * REF_OPS[op]), np.cumsum(n * QRY_OPS[op])
        if not len(w) or p_ref[-1] == 0:
            continue
        t = q_ref[qs] - int(ref_start[a])
        inside = (t >= 0) & (t < p_ref[-1])
        k = np.minimum(np.searchsorted(p_ref, t, side="right"), len(w) - 1)
        ref_before = np.where(k > 0, p_ref[np.maximum(k, 1) - 1], 0)
        qry_before = np.where(k > 0, p_qry[np.maximum(k, 1) - 1], 0)
        aligned = QRY_OPS[op[k]] > 0
        at_end = t == p_ref[-1]
        last = p_qry[np.searchsorted(p_ref, p_ref[-1], side="left")]
        query[qs] = np.where(inside, np.where(aligned, qry_before + t - ref_before, qry_before), np.where(at_end, last, 0))
        state[qs] = np.where(inside, np.where(aligned, _lib.LIFT_ALIGNED, _lib.LIFT_DELETED), np.where(at_end, _lib.LIFT_END, _lib.LIFT_OUTSIDE))
    return query, state


def timed(fn, reps):
    fn()  # warm-up: code objects, the regions' growth, the host's caches
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append(time.perf_counter() - t0)
    return out, wall


def made_up_sites(path, fasta, n_sites, seed=22):
    """A VCF of n_sites deletions and insertions of 50 to 300 bases at random places of `fasta`'s contigs."""
    from svim_asm_amd.fasta import FastaFile
    ref = FastaFile(fasta)
    rng = np.random.default_rng(seed)
    names, lengths = list(ref.references), list(ref.lengths)
    seqs = [ref.fetch(n) for n in names]
    rows = []
    for k in range(n_sites):
        c = int(rng.integers(0, len(names)))
        size = int(rng.integers(50, 300))
        pos = int(rng.integers(1, lengths[c] - size - 1))
        if k % 2:
            rows.append((c, pos, seqs[c][pos - 1:pos + size], seqs[c][pos - 1]))
        else:
            rows.append((c, pos, seqs[c][pos - 1], seqs[c][pos - 1] + "".join("ACGT"[b] for b in rng.integers(0, 4, size))))
    rows.sort(key=lambda r: r[:2])
    with open(path, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for k, (c, pos, r, alt) in enumerate(rows):
            fh.write("%s\t%d\tsite%d\t%s\t%s\t.\tPASS\t.\n" % (names[c], pos, k, r, alt))
    return ref


def genotype_run(n_sites, ctx):
    from svim_asm_amd import SVIM_GENOTYPE, bamio
    gold = os.path.join(ROOT, "tests", "golden", "config1")
    options = argparse.Namespace(flank=100, max_edit_distance=200, max_relative_distance=0.0, min_sv_size=50, min_mapq=20, passonly=False,
                                 sample="Sample", device=0)
    with tempfile.TemporaryDirectory() as tmp:
        reference = made_up_sites(os.path.join(tmp, "sites.vcf"), os.path.join(gold, "ref.fa"), n_sites)
        files = [bamio.AlignmentFile(os.path.join(gold, name), device=0) for name in ("hap1.bam", "hap2.bam")]
        timing = {}
        t0 = time.perf_counter()
        summary = SVIM_GENOTYPE.genotype(os.path.join(tmp, "sites.vcf"), reference, files, options, os.path.join(tmp, "out"), ctx=ctx, timing=timing)
        total = time.perf_counter() - t0
    return {"sites": n_sites, "genotyped": summary["genotyped"], "haplotypes": summary["haplotypes"], "total_s": total,
            "phase_s": {k: timing.get(k, 0.0) for k in SVIM_GENOTYPE.STAGES}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=5000000)
    ap.add_argument("--queries", type=int, default=250000)
    ap.add_argument("--sites", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "lift_probe.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 repetitions")
    batch = synthetic_batch(a.ops, a.queries)
    ctx = _lib.Context(0)  # (raises without a device: a measurement path does not fall back)
    ctx.set_timing(True)
    kernel_ms = []

    def device():
        out = ctx.cigar_lift(*batch)
        kernel_ms.append(ctx.last_kernel_ms())
        return out
    got, dev_wall = timed(device, a.reps)
    exp, host_wall = timed(lambda: on_host(*batch), a.reps)
    ctx.set_timing(False)
    equal = bool(np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]))
    ms = lambda xs: 1e3 * float(np.median(xs))
    result = {
        "date": datetime.date.today().isoformat(), "note": "one box, synthetic; no real cohort or truth set has been genotyped",
        "ops": int(len(batch[0])), "alignments": int(len(batch[1]) - 1), "queries": int(len(batch[3])),
        "states": {name: int((got[1] == code).sum()) for code, name in enumerate(("outside", "aligned", "deleted", "end"))},
        "answers_equal": equal, "reps": a.reps,
        "device_call_ms_median": ms(dev_wall), "device_call_ms_min": 1e3 * min(dev_wall), "device_call_ms_max": 1e3 * max(dev_wall),
        "device_kernels_ms_median": float(np.median([k[0] for k in kernel_ms[1:]])),
        "device_scan_kernels_ms_median": float(np.median([k[1] for k in kernel_ms[1:]])),
        "host_numpy_ms_median": ms(host_wall), "host_numpy_ms_min": 1e3 * min(host_wall), "host_numpy_ms_max": 1e3 * max(host_wall),
        "method": "median of `reps` calls after one untimed call; device: host clock around Context.cigar_lift (uploads, four "
                  "kernels, read-back, synchronise), kernels from HIP events; host: numpy cumsum + searchsorted per alignment, one thread",
    }
    if a.sites:
        result["genotype_run"] = genotype_run(a.sites, ctx)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not equal:
        sys.exit("the device's answers differ from the host's")


if __name__ == "__main__":
    main()
