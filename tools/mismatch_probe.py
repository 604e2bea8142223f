#!/usr/bin/env python3
"""What one batch of svim-asm-small's column comparison costs (svx_cigar_mismatch).

    python tools/mismatch_probe.py [--columns 268435456] [--alignments 64] [--reps 5] [--out profiles/mismatch_probe.json]

Synthetic and seeded: `--alignments` alignments of equal length, M runs of 200 to 2000 columns with an insertion or a
deletion of 1 to 10 bases between them, a soft clip at either end; `--columns` aligned columns in all, about one in a
thousand of them a mismatch.  The pool holds every alignment's reference window and SEQ as ASCII, two bytes per column.
Timed: Context.cigar_mismatch — the upload of the pool, six kernels, the read-back, a host clock around a call that ends in
a synchronise — as the median of `--reps` calls after one untimed call; beside it the kernels' milliseconds from HIP events
(all six, and the three behind the prefix scan), and the same batch on the host with numpy (per alignment the columns' index
vectors from the ops, two gathers, one compare), timed the same way.  The two answers must be equal.  No target: nobody has
measured this before, and a full-size sample's time will be set by the host's supply of the bases, which is not measured here."""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svim_asm_amd import _lib  # noqa: E402

M, I, D, S = 0, 1, 2, 4
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def one_alignment(rng, columns):
    """(ops, lengths, reference window, SEQ) of one alignment with `columns` aligned columns, equal in every column."""
    runs = []
    left = columns
    while left > 0:
        n = min(left, int(rng.integers(200, 2000)))
        runs.append(n)
        left -= n
    k = len(runs)
    op = np.empty(2 * k + 1, np.uint32)
    length = np.empty(2 * k + 1, np.uint32)
    op[0], length[0] = S, 50
    op[1::2], length[1::2] = M, runs
    op[2::2], length[2::2] = rng.choice([I, D], k), rng.integers(1, 10, k)
    op[-1], length[-1] = S, 30
    n64 = length.astype(np.int64)
    uses_ref, uses_qry = (op == M) | (op == D), (op == M) | (op == I) | (op == S)
    ref = ACGT[rng.integers(0, 4, int(n64[uses_ref].sum()))]
    qry = ACGT[rng.integers(0, 4, int(n64[uses_qry].sum()))]
    r0 = np.cumsum(np.where(uses_ref, n64, 0)) - np.where(uses_ref, n64, 0)
    q0 = np.cumsum(np.where(uses_qry, n64, 0)) - np.where(uses_qry, n64, 0)
    for a, b, n in zip(r0[op == M].tolist(), q0[op == M].tolist(), n64[op == M].tolist()):
        qry[b:b + n] = ref[a:a + n]
    return op, length, ref, qry


def synthetic_batch(columns, n_aln, seed=31):
    rng = np.random.default_rng(seed)
    op, length, ref, qry = one_alignment(rng, columns // n_aln)
    cigar = np.tile((length << np.uint32(4)) | op, n_aln)
    aln_off = np.arange(n_aln + 1, dtype=np.uint64) * np.uint64(len(op))
    ref_start = (np.arange(n_aln, dtype=np.int64) * 1000).astype(np.int32)
    bases = np.concatenate((np.tile(ref, n_aln), np.tile(qry, n_aln)))
    # one base in a thousand of the SEQ half becomes another one
    at = len(ref) * n_aln + rng.integers(0, len(qry) * n_aln, (len(qry) * n_aln) // 1000)
    bases[at] = ACGT[(np.searchsorted(ACGT, bases[at]) + rng.integers(1, 4, len(at))) % 4]
    ref_off = np.arange(n_aln, dtype=np.uint64) * np.uint64(len(ref))
    qry_off = np.uint64(len(ref) * n_aln) + np.arange(n_aln, dtype=np.uint64) * np.uint64(len(qry))
    return (cigar, aln_off, ref_start, bases, ref_off, np.full(n_aln, len(ref), np.uint32), qry_off, np.full(n_aln, len(qry), np.uint32))


def on_host(cigar, aln_off, ref_start, bases, ref_off, ref_len, qry_off, qry_len):
    out = {k: [] for k in ("aln", "ref_pos", "qry_pos", "ref_base", "qry_base")}
    for a in range(len(aln_off) - 1):
        w = cigar[int(aln_off[a]):int(aln_off[a + 1])]
        op, n = (w & 15).astype(np.int64), (w >> 4).astype(np.int64)
        uses_ref, uses_qry = np.isin(op, (0, 2, 3, 7, 8)), np.isin(op, (0, 1, 4, 7, 8))
        r0 = np.cumsum(np.where(uses_ref, n, 0)) - np.where(uses_ref, n, 0)
        q0 = np.cumsum(np.where(uses_qry, n, 0)) - np.where(uses_qry, n, 0)
        col = np.isin(op, (0, 7, 8))
        m = n[col]
        within = np.arange(int(m.sum())) - np.repeat(np.cumsum(m) - m, m)
        r, q = np.repeat(r0[col], m) + within, np.repeat(q0[col], m) + within
        keep = (r < int(ref_len[a])) & (q < int(qry_len[a]))
        r, q = r[keep], q[keep]
        R, Q = bases[int(ref_off[a]) + r] & 0xDF, bases[int(qry_off[a]) + q] & 0xDF
        hit = np.flatnonzero((R != Q) & np.isin(R, ACGT) & np.isin(Q, ACGT))
        out["aln"].append(np.full(len(hit), a, np.uint32))
        out["ref_pos"].append((int(ref_start[a]) + r[hit]).astype(np.uint32))
        out["qry_pos"].append(q[hit].astype(np.uint32))
        out["ref_base"].append(R[hit])
        out["qry_base"].append(Q[hit])
    return {k: np.concatenate(v) for k, v in out.items()}


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
    ap.add_argument("--columns", type=int, default=1 << 28)
    ap.add_argument("--alignments", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "mismatch_probe.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 repetitions")
    batch = synthetic_batch(a.columns, a.alignments)
    ctx = _lib.Context(0)  # (raises without a device: a measurement path does not fall back)
    ctx.set_timing(True)
    kernel_ms = []

    def device():
        out = ctx.cigar_mismatch(*batch, cap=len(batch[3]) // 1000)
        kernel_ms.append(ctx.last_kernel_ms())
        return out
    got, dev_wall = timed(device, a.reps)
    exp, host_wall = timed(lambda: on_host(*batch), a.reps)
    ctx.set_timing(False)
    equal = all(np.array_equal(got[k], exp[k]) for k in exp)
    columns = int((((batch[0] & 15) == 0) * (batch[0] >> 4).astype(np.int64)).sum())
    ms = lambda xs: 1e3 * float(np.median(xs))
    kernels = float(np.median([k[0] for k in kernel_ms[1:]]))
    result = {
        "date": datetime.date.today().isoformat(), "note": "one box, synthetic; no real assembly has been compared",
        "columns": columns, "alignments": a.alignments, "ops": int(len(batch[0])), "pool_bytes": int(len(batch[3])),
        "mismatches": int(len(got["aln"])), "answers_equal": bool(equal), "reps": a.reps,
        "device_call_ms_median": ms(dev_wall), "device_call_ms_min": 1e3 * min(dev_wall), "device_call_ms_max": 1e3 * max(dev_wall),
        "device_kernels_ms_median": kernels,
        "device_tile_kernels_ms_median": float(np.median([k[1] for k in kernel_ms[1:]])),
        "kernels_gb_per_s_at_two_bytes_per_column": 2.0 * columns / (kernels * 1e-3) / 1e9,
        "host_numpy_ms_median": ms(host_wall), "host_numpy_ms_min": 1e3 * min(host_wall), "host_numpy_ms_max": 1e3 * max(host_wall),
        "method": "median of `reps` calls after one untimed call; device: host clock around Context.cigar_mismatch (upload of the "
                  "pool from pageable memory, six kernels, read-back, synchronise), kernels from HIP events; host: numpy, per alignment "
                  "the columns' index vectors, two gathers and one compare, one thread",
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
