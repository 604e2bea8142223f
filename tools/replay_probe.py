#!/usr/bin/env python3
"""What one batch of svim-asm-small-compare costs on the device (svx_variant_replay).

    python tools/replay_probe.py [--clusters 1000000] [--long 1000] [--reps 5] [--out profiles/replay_probe.json]

Synthetic and seeded: `--clusters` phased clusters with the cluster-size histogram of tests/golden/config1's pair of call
sets (733 of 2 records, 81 of 4, 10 of 6, 1 of 8 in 825), half of a cluster's records on either side, windows of 30 + 12
bases per record; one cluster in `--long` has a window of 10^4 to 10^5 bases and 100 to 300 records per side.  A record is an
SNV, a deletion of 1 to 3 or an insertion of 1 to 3 bases on one haplotype; comp repeats base's records, one in a hundred
with another inserted or substituted base, so that not every pair is equal.  Four jobs and four pairs per cluster, as the
command lays them out (the four jobs share their window's bytes).  Timed, each as the median of `--reps` calls after one
untimed call: Context.variant_replay on a host clock (the host's checks, uploads from pageable memory, up to twelve
launches, the read-backs), its kernels by HIP events (all of them, and the emit and compare launches alone), the uploads
alone (the same arrays into buffers that exist), and the same batch on the host by a plain splice in numpy, one thread, in
slices of 20 000 clusters.  Every answer must equal the host's.  No target: nobody has measured this before."""
import argparse
import datetime
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svim_asm_amd import _lib  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
FIXTURE_SIZES = np.repeat([1, 2, 3, 4], [733, 81, 10, 1])  # records per side


def flat(pool, start, length):
    total = int(length.sum())
    if not total:
        return np.zeros(0, np.uint8)
    col = np.arange(total) - np.repeat(np.cumsum(length) - length, length)
    return pool[np.repeat(start, length) + col]


def synthetic_batch(n_cl, long_every, seed=20):
    rng = np.random.default_rng(seed)
    per_side = FIXTURE_SIZES[rng.integers(0, len(FIXTURE_SIZES), n_cl)].astype(np.int64)
    win_len = 30 + 12 * per_side
    long_at = rng.choice(n_cl, max(1, n_cl // long_every), replace=False) if long_every else np.zeros(0, np.int64)
    per_side[long_at] = rng.integers(100, 301, len(long_at))
    win_len[long_at] = rng.integers(10_000, 100_001, len(long_at))
    win_off = np.cumsum(win_len) - win_len
    windows = ACGT[rng.integers(0, 4, int(win_len.sum()))]
    # base's records: record i of a cluster begins at 5 + i * spacing (spacing >= 12: in order and inside)
    n_rec = int(per_side.sum())
    cl = np.repeat(np.arange(n_cl), per_side)
    i = np.arange(n_rec) - np.repeat(np.cumsum(per_side) - per_side, per_side)
    start = 5 + i * ((win_len - 10) // per_side)[cl]
    kind = rng.integers(0, 3, n_rec)  # SNV, DEL, INS
    size = rng.integers(1, 4, n_rec)
    ref_len = np.where(kind == 0, 1, np.where(kind == 1, size, 0))
    alt_len = np.where(kind == 0, 1, np.where(kind == 1, 0, size))
    hap = rng.integers(0, 2, n_rec)
    alt_off = np.cumsum(alt_len) - alt_len
    alts = ACGT[rng.integers(0, 4, int(alt_len.sum()))]
    # an SNV's base differs from the reference's
    snv = np.flatnonzero(kind == 0)
    alts[alt_off[snv]] = ACGT[(np.searchsorted(ACGT, windows[win_off[cl[snv]] + start[snv]]) + 1 + rng.integers(0, 3, len(snv))) % 4]
    comp_alts = alts.copy()
    changed = rng.choice(len(alts), max(1, len(alts) // 100), replace=False)
    comp_alts[changed] = ACGT[(np.searchsorted(ACGT, alts[changed]) + 1) % 4]
    pool = np.concatenate((windows, alts, comp_alts))
    # edits: base's records in jobs 4c + h, comp's in 4c + 2 + h; inside a job in start order (the records are)
    job = np.concatenate((4 * cl + hap, 4 * cl + 2 + hap))
    o = np.argsort(job, kind="stable")
    two = lambda x: np.concatenate((x, x))[o]
    ed_first = np.zeros(4 * n_cl + 1, np.int64)
    np.cumsum(np.bincount(job, minlength=4 * n_cl), out=ed_first[1:])
    ed_alt_off = np.concatenate((len(windows) + alt_off, len(windows) + len(alts) + alt_off))[o]
    k = np.arange(n_cl) * 4
    pair_a = (k[:, None] + np.array([0, 1, 0, 1])).reshape(-1)
    pair_b = (k[:, None] + np.array([2, 3, 3, 2])).reshape(-1)
    return (pool, np.repeat(win_off, 4).astype(np.uint64), np.repeat(win_len, 4).astype(np.uint32), ed_first.astype(np.uint32),
            two(start).astype(np.uint32), two(ref_len).astype(np.uint32), ed_alt_off.astype(np.uint64), two(alt_len).astype(np.uint32),
            pair_a.astype(np.uint32), pair_b.astype(np.uint32)), {"records_per_side": n_rec, "long_clusters": int(len(long_at))}


def on_host(pool, win_off, win_len, ed_first, ed_start, ed_ref_len, ed_alt_off, ed_alt_len, pair_a, pair_b, jobs_per_slice=80_000):
    """The plain splice for jobs whose edits are in order and inside (the batch's are): per job the runs window, allele,
    window, ... gathered one behind the other; a pair is equal when lengths and bytes are.  Pairs name jobs of their own
    slice (a cluster's four jobs and four pairs lie together)."""
    n_jobs = len(win_off)
    out_len, equal = np.zeros(n_jobs, np.uint32), np.zeros(len(pair_a), np.uint8)
    first = ed_first.astype(np.int64)
    for j0 in range(0, n_jobs, jobs_per_slice):
        j1 = min(n_jobs, j0 + jobs_per_slice)
        e0, e1 = first[j0], first[j1]
        n_ed = first[j0 + 1:j1 + 1] - first[j0:j1]
        s, r = ed_start[e0:e1].astype(np.int64), ed_ref_len[e0:e1].astype(np.int64)
        a_off, a_len = ed_alt_off[e0:e1].astype(np.int64), ed_alt_len[e0:e1].astype(np.int64)
        job = np.repeat(np.arange(j1 - j0), n_ed)
        w0, wl = win_off[j0:j1].astype(np.int64), win_len[j0:j1].astype(np.int64)
        is_first = np.ones(e1 - e0, bool)
        is_first[1:] = job[1:] != job[:-1]
        prev_end = np.zeros(e1 - e0, np.int64)
        prev_end[1:] = (s + r)[:-1]
        prev_end[is_first] = 0
        # runs in output order: per edit (window in front of it, its allele), per job the window behind its last edit
        last_end = np.zeros(j1 - j0, np.int64)
        has = n_ed > 0
        last_end[has] = (s + r)[(first[j0 + 1:j1 + 1] - e0 - 1)[has]]
        run_src = np.concatenate((w0[job] + prev_end, a_off, w0 + last_end))
        run_len = np.concatenate((s - prev_end, a_len, wl - last_end))
        run_key = np.concatenate((2 * (np.arange(e1 - e0) + job), 2 * (np.arange(e1 - e0) + job) + 1, 2 * (first[j0 + 1:j1 + 1] - e0 + np.arange(j1 - j0))))
        o = np.argsort(run_key, kind="stable")
        run_src, run_len = run_src[o], run_len[o]
        run_job = np.concatenate((job, job, np.arange(j1 - j0)))[o]
        length = np.bincount(run_job, weights=run_len, minlength=j1 - j0).astype(np.int64)
        out_len[j0:j1] = length
        text = flat(pool, run_src, run_len)
        off = np.cumsum(length) - length
        p0, p1 = j0, j1  # (as many pairs as jobs, cluster by cluster)
        a, b = pair_a[p0:p1].astype(np.int64) - j0, pair_b[p0:p1].astype(np.int64) - j0
        same_len = length[a] == length[b]
        n = np.where(same_len, length[a], 0)
        diff = flat(text, off[a], n) != flat(text, off[b], n)
        bad = np.concatenate(([0], np.cumsum(diff)))
        ends = np.cumsum(n)
        equal[p0:p1] = same_len & (bad[ends] == bad[ends - n])
    return out_len, equal


def timed(fn, reps):
    fn()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append(time.perf_counter() - t0)
    return out, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=1000000)
    ap.add_argument("--long", type=int, default=1000, help="one cluster in this many has a window of 10^4 to 10^5 bases (0: none)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "replay_probe.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 repetitions")
    batch, facts = synthetic_batch(a.clusters, a.long)
    t0 = time.perf_counter()
    exp_len, exp_equal = on_host(*batch)
    host_s = [time.perf_counter() - t0]  # (tens of seconds: once, not `reps` times)
    ctx = _lib.Context(0)  # (raises without a device: a measurement path does not fall back)
    ctx.set_timing(True)
    ms = lambda xs: 1e3 * float(np.median(xs))
    host_arrays = [np.ascontiguousarray(x) for x in batch]
    buffers = [ctx.dev_array(nbytes=max(1, x.nbytes)) for x in host_arrays]

    def upload():
        for x, d in zip(host_arrays, buffers):
            ctx._check(ctx.lib.svx_dev_upload(ctx.h, d.ptr, x.ctypes.data, x.nbytes))
        ctx.sync()
    _, up_wall = timed(upload, a.reps)
    kernel_ms = []

    def device():
        out = ctx.variant_replay(*batch)
        kernel_ms.append(ctx.last_kernel_ms())
        return out
    got, wall = timed(device, a.reps)
    ctx.set_timing(False)
    equal = bool(np.array_equal(got["out_len"], exp_len) and np.array_equal(got["equal"], exp_equal) and not got["status"].any())
    result = {
        "date": datetime.date.today().isoformat(), "box": socket.gethostname(), "note": "one box, synthetic; no real call set has been scored",
        "clusters": a.clusters, "jobs": int(len(batch[1])), "edits": int(len(batch[4])), "pairs": int(len(batch[8])),
        "pool_bytes": int(len(batch[0])), "column_bytes": int(sum(x.nbytes for x in batch[1:])), "string_bytes": int(got["total"]),
        "equal_pairs": int(exp_equal.sum()), "reps": a.reps, "answers_equal": equal, "tile": _lib.REPLAY_TILE,
        "call_ms_median": ms(wall), "call_ms_min": 1e3 * min(wall), "call_ms_max": 1e3 * max(wall),
        "kernels_ms_median": float(np.median([k[0] for k in kernel_ms[1:]])), "kernels_ms_min": float(min(k[0] for k in kernel_ms[1:])),
        "kernels_ms_max": float(max(k[0] for k in kernel_ms[1:])),
        "emit_and_compare_ms_median": float(np.median([k[1] for k in kernel_ms[1:]])),
        "upload_ms_median": ms(up_wall), "upload_ms_min": 1e3 * min(up_wall), "upload_ms_max": 1e3 * max(up_wall),
        "upload_share_of_the_call": ms(up_wall) / ms(wall),
        "host_numpy_ms": 1e3 * host_s[0],
        "method": "median of `reps` calls after one untimed call; call: host clock around Context.variant_replay without strings (the "
                  "host's checks, uploads from pageable memory, the launches, the read-backs, synchronise); kernels: HIP events behind "
                  "the uploads; emit_and_compare: from k_replay_emit to the last launch; upload: svx_dev_upload of the same arrays "
                  "into existing buffers, then a synchronise; host: the plain splice in numpy, one thread, ONE run",
    }
    result.update(facts)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not equal:
        sys.exit("the device's answers differ from the host's")


if __name__ == "__main__":
    main()
