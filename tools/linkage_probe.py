#!/usr/bin/env python3
"""Lane path against workgroup path of the complete linkage at the partition sizes of a cohort merge, and the wall-clock
of one synthetic merge.

    python tools/linkage_probe.py [--reps 7] [--parts 2000] [--out profiles/linkage_group_probe.json] [--no-cohort]

Kernel part: batches of `--parts` partitions of n in {16, 32, 64, 128, 300} members, integer distances in 0..49, through
svx_linkage_cut_batch_dev with the device buffers resident; svx_ctx_set_timing / svx_ctx_last_kernel_ms give the kernel
milliseconds.  The two settings — group_min = 0xFFFFFFFF (every partition one lane: all there was before the group
kernel) and group_min = 2 (every partition one workgroup) — alternate inside every repetition, after one untimed call of
each; the table holds the medians and the extremes.  The labels of the two settings are compared once per size.

Cohort part ("measured once, one box"): 64 synthetic samples at the size of a human sample (svim_asm_amd/synth.py's
config-2 contigs, ~20 000 calls per sample, a fiftieth of the loci with a different allele in almost every carrier) merged
by SVIM_MERGE.merge_tables against a procedural reference; wall-clock seconds per stage, no target."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svim_asm_amd import _lib, synth  # noqa: E402

SIZES = (16, 32, 64, 128, 300)
LANES, GROUPS = _lib.LINKAGE_LANES_ONLY, 2


def kernel_table(ctx, parts, reps):
    rows = []
    ctx.set_timing(True)
    for n in SIZES:
        rng = np.random.default_rng(n)
        m = n * (n - 1) // 2
        dist = rng.integers(0, 50, parts * m).astype(np.float64)
        counts = np.full(parts, n, np.uint32)
        d_dist, d_n, d_lab = ctx.dev_array(host=dist), ctx.dev_array(host=counts), ctx.dev_array(nbytes=4 * parts * n)

        def run(setting):
            ctx.set_linkage_group_min(setting)
            ctx._check(ctx.lib.svx_linkage_cut_batch_dev(ctx.h, d_dist.ptr, counts.ctypes.data, d_n.ptr, parts, 10.0, d_lab.ptr))
            ctx.sync()
            total, dominant = C.c_float(), C.c_float()
            ctx._check(ctx.lib.svx_ctx_last_kernel_ms(ctx.h, C.byref(total), C.byref(dominant)))
            return float(dominant.value)
        labels = {}
        for setting in (LANES, GROUPS):  # warm-up: code objects, workspace growth
            run(setting)
            labels[setting] = d_lab.download(np.uint32)
        ms = {LANES: [], GROUPS: []}
        for r in range(reps):
            for setting in ((LANES, GROUPS) if r % 2 == 0 else (GROUPS, LANES)):
                ms[setting].append(run(setting))
        row = {"n": n, "partitions": parts, "labels_equal": bool(np.array_equal(labels[LANES], labels[GROUPS]))}
        for name, setting in (("lanes", LANES), ("group", GROUPS)):
            row[name + "_ms_median"] = float(np.median(ms[setting]))
            row[name + "_ms_min"], row[name + "_ms_max"] = float(min(ms[setting])), float(max(ms[setting]))
        row["lanes_over_group"] = row["lanes_ms_median"] / row["group_ms_median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        for d in (d_dist, d_n, d_lab):
            d.free()
    ctx.set_linkage_group_min(0)
    ctx.set_timing(False)
    return rows


class ProceduralReference(object):
    """A genome of config-2's contigs whose bases are one seeded megabase repeated: fetch() without a 3-GB file."""

    def __init__(self, names, lengths):
        self.references, self.lengths = list(names), [int(x) for x in lengths]
        self._len = dict(zip(self.references, self.lengths))
        self._block = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(7).integers(0, 4, 1 << 20)]

    def get_reference_length(self, name):
        return self._len[name]

    def fetch(self, name, start, end):
        end = min(end, self._len[name])
        if start >= end:
            return ""
        return self._block[np.arange(start, end) & ((1 << 20) - 1)].tobytes().decode()

    def close(self):
        pass


def synthetic_cohort(n_samples, n_loci, seed=11):
    """One CandidateTable per sample: deletions and insertions at `n_loci` shared loci; at a fiftieth of them (VNTR-like)
    every carrier has an allele of its own length."""
    from svim_asm_amd.table import CandidateTable, T_DEL, T_INS
    rng = np.random.default_rng(seed)
    names, lengths = synth.GRCH38_NAMES, synth.GRCH38_LENGTHS
    contig = rng.choice(len(names), n_loci, p=lengths / lengths.sum())
    pos = (rng.random(n_loci) * (lengths[contig] - 20000)).astype(np.int64) + 10000
    is_ins = rng.random(n_loci) < 0.5
    size = np.clip(np.exp(rng.uniform(np.log(40), np.log(2000), n_loci)).astype(np.int64), 40, 2000)
    vntr = rng.random(n_loci) < 0.02
    freq = rng.beta(0.5, 0.5, n_loci)
    ins_pool = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 4096)]
    tables = []
    for s in range(n_samples):
        carried = np.flatnonzero(rng.random(n_loci) < freq)
        n = len(carried)
        t = CandidateTable(names, lengths, n)
        mine = size[carried] + np.where(vntr[carried], rng.integers(0, 120, n) * 3, 0)
        ins = is_ins[carried]
        t.type[:] = np.where(ins, T_INS, T_DEL)
        t.sc[:] = np.where(ins, -1, contig[carried]); t.ss[:] = np.where(ins, 0, pos[carried]); t.se[:] = np.where(ins, 0, pos[carried] + mine)
        t.dc[:] = np.where(ins, contig[carried], -1); t.ds[:] = np.where(ins, pos[carried], 0); t.de[:] = np.where(ins, pos[carried] + mine, 0)
        t.gt[:] = rng.integers(0, 3, n)
        t.q_len[:] = np.where(ins, mine, 0)
        t.q_off[:] = np.cumsum(t.q_len) - t.q_len
        # the inserted bytes of a locus are the same for everybody (a prefix of one pool: length decides the allele)
        idx = np.concatenate([(np.arange(l) + 13 * c) % 4096 for l, c in zip(t.q_len[ins].tolist(), carried[ins].tolist())]) \
            if bool(ins.any()) else np.zeros(0, np.int64)
        t.seqs = ins_pool[idx]
        tables.append(t)
    return tables, ProceduralReference(names, lengths)


def cohort_wall_clock(ctx, n_samples=64, n_loci=40000):
    from svim_asm_amd import SVIM_COMBINE, SVIM_MERGE
    t0 = time.perf_counter()
    tables, reference = synthetic_cohort(n_samples, n_loci)
    t_build = time.perf_counter() - t0
    options = argparse.Namespace(partition_max_distance=1000, max_edit_distance=200, merge_max_partition=1024, device=0)
    t0 = time.perf_counter()
    merged, G = SVIM_MERGE.merge_tables(tables, ["s%d" % k for k in range(n_samples)], reference, options, ctx=ctx)
    wall = time.perf_counter() - t0
    out = {"samples": n_samples, "rows_in": int(sum(len(t) for t in tables)), "records_out": int(len(merged)),
           "build_inputs_s": t_build, "merge_tables_s": wall, "note": "measured once, one box",
           "stages_s": {k: v for k, v in SVIM_COMBINE.LAST_TIMING.items() if k.startswith("pair_") and k.endswith("_s") and "cpu" not in k}}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parts", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join("profiles", "linkage_group_probe.json"))
    ap.add_argument("--no-cohort", action="store_true")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 repetitions")
    ctx = _lib.Context(0)
    result = {"kernel": kernel_table(ctx, a.parts, a.reps), "reps": a.reps,
              "method": "settings alternate inside every repetition after one untimed call of each; kernel ms from HIP events"}
    if not a.no_cohort:
        result["cohort_merge"] = cohort_wall_clock(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
