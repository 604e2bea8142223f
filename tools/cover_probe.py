#!/usr/bin/env python3
"""What the coverage query of a cohort merge costs (svx_cover_query) at the size of a 64-sample cohort.

    python tools/cover_probe.py [--samples 64] [--intervals 20000] [--records 40000] [--reps 5] [--out profiles/cover_probe.json]

Synthetic and seeded: `--samples` x 2 lists of `--intervals` alignments each over the contigs of svim_asm_amd/synth.py
(tiling the genome with gaps and overlaps, a tenth of them nested inside their neighbour), and the windows of
`--records` records (2 kb, a margin of 1000 on either side of a point).  Timed: Context.cover_query — the uploads, the
two kernels, the read-back, a host clock around a call that ends in a synchronise — as the median of `--reps` calls after
one untimed call; beside it the kernels' share from HIP events, and the same batch on the host with numpy
(searchsorted + maximum.accumulate per list), timed the same way.  The two answers must be equal.  No target: the
number is what it is."""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svim_asm_amd import _lib, synth  # noqa: E402


def synthetic_batch(n_lists, n_intervals, n_records, seed=14):
    rng = np.random.default_rng(seed)
    lengths = np.asarray(synth.GRCH38_LENGTHS, dtype=np.int64)
    p = lengths / lengths.sum()
    starts, ends = [], []
    for _ in range(n_lists):
        contig = np.sort(rng.choice(len(lengths), n_intervals, p=p))
        pos = (rng.random(n_intervals) * (lengths[contig] - 1)).astype(np.int64)
        key = np.sort((contig.astype(np.uint64) << np.uint64(32)) | pos.astype(np.uint64))
        contig, pos = (key >> np.uint64(32)).astype(np.int64), (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        # an alignment reaches about as far as the next one starts, give or take; a tenth stop well inside it
        nxt = np.concatenate([pos[1:], lengths[contig[-1:]]])
        same = np.concatenate([contig[1:] == contig[:-1], [False]])
        reach = np.where(same, nxt - pos, lengths[contig] - pos)
        length = np.maximum(1, (reach * rng.uniform(0.7, 1.3, n_intervals)).astype(np.int64))
        length = np.where(rng.random(n_intervals) < 0.1, np.maximum(1, length // 20), length)
        end = np.minimum(lengths[contig], pos + length)
        starts.append(key)
        ends.append((contig.astype(np.uint64) << np.uint64(32)) | end.astype(np.uint64))
    list_off = (np.arange(n_lists + 1, dtype=np.uint64) * np.uint64(n_intervals))
    contig = rng.choice(len(lengths), n_records, p=p)
    mid = (rng.random(n_records) * lengths[contig]).astype(np.int64)
    lo, hi = np.maximum(mid - 1000, 0), np.minimum(mid + 1000, lengths[contig])
    c64 = contig.astype(np.uint64) << np.uint64(32)
    return np.concatenate(starts), np.concatenate(ends), list_off, c64 | lo.astype(np.uint64), c64 | hi.astype(np.uint64)


def on_host(start, end, list_off, q_lo, q_hi):
    out = np.zeros((len(list_off) - 1, len(q_lo)), np.uint8)
    for l in range(len(list_off) - 1):
        a, b = int(list_off[l]), int(list_off[l + 1])
        if a == b:
            continue
        k = np.searchsorted(start[a:b], q_lo, side="right")
        reach = np.maximum.accumulate(end[a:b])
        out[l] = (k > 0) & (reach[np.maximum(k, 1) - 1] >= q_hi)
    return out


def timed(fn, reps):
    fn()  # warm-up: code objects, the regions' growth, the host's caches
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append(time.perf_counter() - t0)
    return out, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--intervals", type=int, default=20000)
    ap.add_argument("--records", type=int, default=40000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "cover_probe.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 repetitions")
    batch = synthetic_batch(2 * a.samples, a.intervals, a.records)
    ctx = _lib.Context(0)  # (raises without a device: a measurement path does not fall back)
    ctx.set_timing(True)
    kernel_ms = []

    def device():
        out = ctx.cover_query(*batch)
        kernel_ms.append(ctx.last_kernel_ms())
        return out
    got, dev_wall = timed(device, a.reps)
    exp, host_wall = timed(lambda: on_host(*batch), a.reps)
    equal = bool(np.array_equal(got, exp))
    ms = lambda xs: 1e3 * float(np.median(xs))
    result = {
        "date": datetime.date.today().isoformat(), "note": "one box, synthetic",
        "lists": 2 * a.samples, "intervals_per_list": a.intervals, "queries": a.records, "answers": int(got.size),
        "share_of_ones": float(got.mean()), "answers_equal": equal, "reps": a.reps,
        "device_call_ms_median": ms(dev_wall), "device_call_ms_min": 1e3 * min(dev_wall), "device_call_ms_max": 1e3 * max(dev_wall),
        "device_kernels_ms_median": float(np.median([k[0] for k in kernel_ms[1:]])),
        "device_search_kernel_ms_median": float(np.median([k[1] for k in kernel_ms[1:]])),
        "host_numpy_ms_median": ms(host_wall), "host_numpy_ms_min": 1e3 * min(host_wall), "host_numpy_ms_max": 1e3 * max(host_wall),
        "method": "median of `reps` calls after one untimed call; device: host clock around Context.cover_query (uploads, "
                  "two kernels, read-back, synchronise), kernels from HIP events; host: numpy searchsorted + maximum.accumulate "
                  "per list, one thread",
    }
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not equal:
        sys.exit("the device's answers differ from the host's")


if __name__ == "__main__":
    main()
