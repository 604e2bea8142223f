#!/usr/bin/env python3
"""What the single-coverage sweep of a cohort costs (svx_cover_single) at the size of a 64-sample cohort.

    python tools/callable_probe.py [--samples 64] [--intervals 20000] [--reps 5] [--out profiles/callable_probe.json]

The synthetic, seeded batch of tools/cover_probe.py: `--samples` x 2 lists of `--intervals` alignments each (tiling the
genome with gaps and overlaps, a tenth of them nested inside their neighbour).  Timed: Context.cover_single — the uploads,
the three kernels, the read-backs, a host clock around a call that ends in a synchronise — as the median of `--reps`
calls after one untimed call; beside it the kernels' share from HIP events, and the same batch on the host with numpy
(per list: the +1 / -1 events sorted, a running sum, the pieces of depth 1), one thread, timed the same way.  The two
answers must be equal.  No target: the number is what it is."""
import argparse
import datetime
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svim_asm_amd import _lib  # noqa: E402
from tools.cover_probe import synthetic_batch, timed  # noqa: E402


def on_host(start, end, list_off):
    """(seg_lo, seg_hi, seg_off).  Between two neighbouring distinct keys of a list no entry begins or ends; where the
    depth is 1 on both sides of a key, one entry ended there and another began (no entry is empty): every piece of depth
    1 is a segment of its own."""
    los, his, seg_off = [], [], np.zeros(len(list_off), np.uint64)
    for l in range(len(list_off) - 1):
        a, b = int(list_off[l]), int(list_off[l + 1])
        if a < b:
            key = np.concatenate([start[a:b], end[a:b]])
            step = np.concatenate([np.ones(b - a, np.int64), -np.ones(b - a, np.int64)])
            order = np.argsort(key, kind="stable")
            key, step = key[order], step[order]
            at = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
            depth = np.cumsum(np.add.reduceat(step, at))
            key = key[at]
            one = np.flatnonzero(depth[:-1] == 1)
            los.append(key[one])
            his.append(key[one + 1])
        seg_off[l + 1] = seg_off[l] + np.uint64(len(los[-1]) if a < b else 0)
    empty = np.zeros(0, np.uint64)
    return (np.concatenate(los) if los else empty), (np.concatenate(his) if his else empty), seg_off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--intervals", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "callable_probe.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 repetitions")
    start, end, list_off = synthetic_batch(2 * a.samples, a.intervals, 1)[:3]
    ctx = _lib.Context(0)  # (raises without a device: a measurement path does not fall back)
    ctx.set_timing(True)
    kernel_ms = []

    def device():
        out = ctx.cover_single(start, end, list_off)
        kernel_ms.append(ctx.last_kernel_ms())
        return out
    got, dev_wall = timed(device, a.reps)
    exp, host_wall = timed(lambda: on_host(start, end, list_off), a.reps)
    equal = all(bool(np.array_equal(g, e)) for g, e in zip(got, exp))
    ms = lambda xs: 1e3 * float(np.median(xs))
    result = {
        "date": datetime.date.today().isoformat(), "note": "one box, synthetic",
        "lists": 2 * a.samples, "intervals_per_list": a.intervals, "segments": int(len(got[0])),
        "share_of_slots_with_a_segment": float(len(got[0])) / float(len(start)), "answers_equal": equal, "reps": a.reps,
        "device_call_ms_median": ms(dev_wall), "device_call_ms_min": 1e3 * min(dev_wall), "device_call_ms_max": 1e3 * max(dev_wall),
        "device_kernels_ms_median": float(np.median([k[0] for k in kernel_ms[1:]])),
        "device_scan_kernel_ms_median": float(np.median([k[1] for k in kernel_ms[1:]])),
        "host_numpy_ms_median": ms(host_wall), "host_numpy_ms_min": 1e3 * min(host_wall), "host_numpy_ms_max": 1e3 * max(host_wall),
        "method": "median of `reps` calls after one untimed call; device: host clock around Context.cover_single (uploads, "
                  "three kernels, read-backs, synchronise), kernels from HIP events; host: numpy sorted +1/-1 events and cumsum "
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
