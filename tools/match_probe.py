#!/usr/bin/env python3
"""Lane form against workgroup form of the greedy matching (svx_match_greedy_batch): where the default of
svx_ctx_set_match_group_min comes from.

    python tools/match_probe.py [--reps 9] [--out profiles/match_probe.json]

Three tables, every figure the kernel milliseconds between the HIP events around the matching launches
(svx_ctx_set_timing / svx_ctx_last_kernel_ms; the offsets launch and the copies are outside):
  call     one call of 60 000 partitions as a comparison of two call sets hands them over: mostly 1 x 1, one in six 1 x 2
           or 2 x 1, and a seeded tail of squares up to 64 x 64 — at the default threshold, lanes only, groups only and at a
           sweep of thresholds;
  single   ONE partition of n x n, n = 1 ... 512, values from {0..3} with one cell in eight ineligible (edit distances
           tie), lanes only against groups only;
  batch    2 000 partitions of n x n, n = 1 ... 64, the same two settings: what the threshold costs when the device is full.
The settings alternate inside every repetition after one untimed call of each; the tables hold medians and extremes, and
the outputs of the settings are compared once per row.  The baseline of the group form is the lane form of the same build
on the same case; the default threshold is the smallest size from which the group form wins in `single` AND in `batch`.

End to end ("measured once, one box", --no-compare leaves it out): svim-asm-compare's SVIM_COMPARE.compare on two
synthetic call sets of 60 000 records each at the contig sizes of a human genome (svim_asm_amd/synth.py) — symbolic
deletions and sequence-resolved insertions; the second file has 95 % of the first one's loci, moved by up to ten bases and
with a few substitutions, and 3 000 calls of its own — against a procedural reference; wall-clock seconds split into
read / partition / distances / match / write.  No target; a real truth set has not been compared."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svim_asm_amd import _lib  # noqa: E402

NONE = _lib.MATCH_NONE
LANES, GROUPS, DEFAULT = _lib.MATCH_LANES_ONLY, 1, 0
SINGLE = (1, 2, 3, 4, 8, 12, 16, 24, 32, 64, 128, 256, 512)
BATCH = (1, 2, 3, 4, 8, 12, 16, 24, 32, 64)
THRESHOLDS = (2, 4, 8, 16, 32, 64, 256)  # `call` once more at each of these values of group_min
LANE_REPS_CAP = {512: 3}  # a lane at 512 x 512 reads the matrix hundreds of times: seconds a call


def square(rng, n):
    m = rng.integers(0, 4, n * n, dtype=np.uint32)
    m[rng.integers(0, 8, n * n) == 0] = NONE
    return m


def call_of_60000(seed=5, n_parts=60000):
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 6, n_parts)
    n_base = np.where(kind == 4, 2, 1).astype(np.uint32)
    n_comp = np.where(kind == 5, 2, 1).astype(np.uint32)
    tail = rng.choice(n_parts, 600, replace=False)
    side = np.clip(np.exp(rng.uniform(np.log(2), np.log(64), len(tail))).astype(np.int64), 2, 64)
    n_base[tail] = side
    n_comp[tail] = side
    n = int((n_base.astype(np.int64) * n_comp).sum())
    dist = rng.integers(0, 200, n, dtype=np.uint32)
    dist[rng.integers(0, 8, n) == 0] = NONE
    return dist, n_base, n_comp


def timed(ctx, dist, n_base, n_comp, setting):
    ctx.set_match_group_min(setting)
    out = ctx.match_greedy_batch(dist, n_base, n_comp)
    total, dominant = C.c_float(), C.c_float()
    ctx._check(ctx.lib.svx_ctx_last_kernel_ms(ctx.h, C.byref(total), C.byref(dominant)))
    return float(dominant.value), out


def compare(ctx, dist, n_base, n_comp, settings, reps, reps_cap=None):
    """{name: [ms...]} with the settings alternating, and whether all of them gave the same outputs."""
    outs, ms = {}, {name: [] for name, _ in settings}
    for name, setting in settings:  # warm-up: code objects, scratch growth
        outs[name] = timed(ctx, dist, n_base, n_comp, setting)[1]
    first = outs[settings[0][0]]
    same = all(np.array_equal(o[0], first[0]) and np.array_equal(o[1], first[1]) for o in outs.values())
    for r in range(reps):
        for name, setting in (settings if r % 2 == 0 else settings[::-1]):
            if reps_cap and name in reps_cap and len(ms[name]) >= reps_cap[name]:
                continue
            ms[name].append(timed(ctx, dist, n_base, n_comp, setting)[0])
    row = {"outputs_equal": bool(same)}
    for name, _ in settings:
        row[name + "_ms_median"] = float(np.median(ms[name]))
        row[name + "_ms_min"], row[name + "_ms_max"], row[name + "_reps"] = float(min(ms[name])), float(max(ms[name])), len(ms[name])
    return row


def write_call_sets(directory, n=60000, seed=9):
    """(base.vcf, comp.vcf, names, lengths): two synthetic call sets, written without a reference (symbolic deletions,
    insertions as N + bytes)."""
    from svim_asm_amd import synth
    rng = np.random.default_rng(seed)
    names, lengths = list(synth.GRCH38_NAMES), np.asarray(synth.GRCH38_LENGTHS, np.int64)
    contig = rng.choice(len(names), n, p=lengths / lengths.sum())
    pos = (rng.random(n) * (lengths[contig] - 40000)).astype(np.int64) + 20000
    size = np.clip(np.exp(rng.uniform(np.log(50), np.log(3000), n)).astype(np.int64), 50, 3000)
    is_ins = rng.random(n) < 0.5
    pool = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1 << 16)]
    order = np.lexsort((pos, contig))
    header = "##fileformat=VCFv4.2\n" + "".join("##contig=<ID=%s,length=%d>\n" % (a, b) for a, b in zip(names, lengths.tolist())) + \
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"

    def line(k, shift, subs, tag):
        c, p, l = names[contig[k]], int(pos[k]) + shift, int(size[k])
        gt = ("0/1", "1/0", "1/1")[k % 3]
        if not is_ins[k]:
            return "%s\t%d\t%s%d\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=%d;SVLEN=%d\tGT\t%s\n" % (c, p, tag, k, p + l, -l, gt)
        seq = pool[(np.arange(l) + 31 * k) & 0xFFFF].copy()
        if subs:
            seq[rng.integers(0, l, subs)] = ord("A")
        return "%s\t%d\t%s%d\tN\tN%s\t.\tPASS\tSVTYPE=INS\tGT\t%s\n" % (c, p, tag, k, seq.tobytes().decode(), gt)
    base, comp = os.path.join(directory, "base.vcf"), os.path.join(directory, "comp.vcf")
    with open(base, "w") as fh:
        fh.write(header + "".join(line(int(k), 0, 0, "b") for k in order))
    kept = order[rng.random(n) < 0.95]
    with open(comp, "w") as fh:
        fh.write(header + "".join(line(int(k), int(rng.integers(0, 11)), int(rng.integers(0, 4)), "c") for k in kept))
        extra = rng.choice(n, min(3000, n), replace=False)
        fh.write("".join(line(int(k), 5000, 0, "x") for k in extra[np.lexsort((pos[extra], contig[extra]))]))
    return base, comp, names, lengths


def end_to_end(ctx):
    import tempfile
    import time
    from linkage_probe import ProceduralReference
    from svim_asm_amd import SVIM_COMPARE
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        base, comp, names, lengths = write_call_sets(d)
        t_build = time.perf_counter() - t0
        reference = ProceduralReference(names, lengths)
        options = argparse.Namespace(include_bed=None, partition_max_distance=1000, max_edit_distance=200, max_relative_distance=0.0,
                                     min_sv_size=50, comp_min_sv_size=30, compare_max_partition=1024, base_sample=None, comp_sample=None,
                                     passonly=False, device=0)
        t0 = time.perf_counter()
        stages = {}
        summary = SVIM_COMPARE.compare(base, comp, reference, options, os.path.join(d, "out"), ctx=ctx, timing=stages)
        wall = time.perf_counter() - t0
    out = {"records": [summary["base"]["records"], summary["comp"]["records"]], "build_inputs_s": t_build, "compare_s": wall,
           "stages_s": stages, "note": "measured once, one box",
           "summary": {k: summary[k] for k in ("TP-base", "FN", "TP-comp", "FP", "precision", "recall", "gt_concordance")}}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-compare", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join("profiles", "match_probe.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 repetitions")
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    two = (("lanes", LANES), ("group", GROUPS))
    result = {"reps": a.reps, "single": [], "batch": [],
              "method": "settings alternate inside every repetition after one untimed call of each; kernel ms from HIP events "
                        "around the matching launches"}
    dist, n_base, n_comp = call_of_60000()
    sweep = tuple(("min_%d" % t, t) for t in THRESHOLDS)
    row = compare(ctx, dist, n_base, n_comp, (("default", DEFAULT),) + two + sweep, a.reps)
    row.update(partitions=len(n_base), pairs=len(dist), largest=int(n_base.max()))
    result["call"] = row
    print(json.dumps(row), flush=True)
    for n in SINGLE:
        cap = {"lanes": LANE_REPS_CAP[n]} if n in LANE_REPS_CAP else None
        row = compare(ctx, square(np.random.default_rng(n), n), [n], [n], two, a.reps, cap)
        row.update(n=n, pairs=n * n, lanes_over_group=row["lanes_ms_median"] / row["group_ms_median"])
        result["single"].append(row)
        print(json.dumps(row), flush=True)
    for n in BATCH:
        parts = 2000
        dist = np.concatenate([square(np.random.default_rng(1000 * n + k), n) for k in range(parts)])
        row = compare(ctx, dist, np.full(parts, n, np.uint32), np.full(parts, n, np.uint32), two, a.reps)
        row.update(n=n, pairs=n * n, partitions=parts, lanes_over_group=row["lanes_ms_median"] / row["group_ms_median"])
        result["batch"].append(row)
        print(json.dumps(row), flush=True)
    ctx.set_match_group_min(0)
    ctx.set_timing(False)
    if not a.no_compare:
        result["compare_60000"] = end_to_end(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
