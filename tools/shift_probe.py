#!/usr/bin/env python3
"""What one batch of svim-asm-small --left_align costs, and where the lane form should hand over to the wave form
(svx_indel_shift).

    python tools/shift_probe.py [--events 1000000] [--long 1000] [--reps 7] [--out profiles/shift_probe.json]

Synthetic and seeded: `--events` gaps of one base at the right end of a homopolymer run, half deletions and half
insertions, 20 random bases between one run and the next, in 64 alignments.  The true shift of an event is the length of
its run: drawn from the shifts of tests/golden/config1's 394 small indels (0: 298, 1: 71, 2: 21, 3: 3, 5: 1), but one event
in `--long` gets a shift of 100 to 5000, uniform — the microsatellite and homopolymer tail a real genome has and the fixture
lacks.  Limits as the command computes them (the column behind the gap in front).  Timed, each as the median of `--reps`
calls after one untimed call: Context.indel_shift on a host clock (uploads from pageable memory, three or four launches,
one read-back of the list's length, the read-back of the shifts), its kernels by HIP events (all of them, and the wave
form's launch alone), the uploads alone (the pool and the event columns into buffers that exist), and the same batch on the
host with numpy (all events in lockstep, one step per pass over the events still walking) — for lane_steps 0 (wave form
only), 2, 4, 8, 16, 32, 64, INT32_MAX (lane form only) and the built default.  Every answer must equal numpy's.  No target:
nobody has measured this before."""
import argparse
import ctypes as C
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
FIXTURE_SHIFTS = np.repeat([0, 1, 2, 3, 5], [298, 71, 21, 3, 1])
FILLER = 20
INS, DEL = 0, 1


def synthetic_batch(n_ev, long_every, n_aln=64, seed=19):
    rng = np.random.default_rng(seed)
    shift = FIXTURE_SHIFTS[rng.integers(0, len(FIXTURE_SHIFTS), n_ev)].astype(np.int64)
    long_at = rng.choice(n_ev, max(1, n_ev // long_every), replace=False) if long_every else np.zeros(0, np.int64)
    shift[long_at] = rng.integers(100, 5001, len(long_at))
    kind = rng.integers(0, 2, n_ev).astype(np.uint8)
    base = rng.integers(0, 4, n_ev)

    def strand(extra):
        """Per event FILLER random bases and a run of shift + extra bases; the filler's last base and the next filler's
        first one differ from the run's base."""
        run = shift + extra
        seg_len = np.stack((np.full(n_ev, FILLER, np.int64), run), axis=1).reshape(-1)
        seg_off = np.cumsum(seg_len) - seg_len
        total = int(seg_len.sum())
        seg = np.repeat(np.arange(2 * n_ev), seg_len)
        out = np.where(seg & 1, base[seg >> 1], rng.integers(0, 4, total))
        out[seg_off[0::2] + FILLER - 1] = (base + 1) % 4
        out[seg_off[2::2]] = (base[:-1] + 2) % 4
        return ACGT[out], seg_off[0::2], int(total)
    ref, ref_at, ref_total = strand((kind == DEL).astype(np.int64))
    qry, qry_at, qry_total = strand((kind == INS).astype(np.int64))
    first = np.arange(n_aln) * (n_ev // n_aln)  # the first event of every alignment
    aln = (np.searchsorted(first, np.arange(n_ev), side="right") - 1).astype(np.uint32)
    ref_off, qry_off = ref_at[first].astype(np.uint64), (ref_total + qry_at[first]).astype(np.uint64)
    ref_len = np.diff(np.append(ref_at[first], ref_total)).astype(np.uint32)
    qry_len = np.diff(np.append(qry_at[first], qry_total)).astype(np.uint32)
    ref_start = np.full(n_aln, 1000, np.int32)
    r = ref_at + FILLER + shift - ref_at[first][aln]
    q = qry_at + FILLER + shift - qry_at[first][aln]
    prev_end = np.zeros(n_ev, np.int64)
    prev_end[1:] = np.where(aln[1:] == aln[:-1], (r + (kind == DEL))[:-1], 0)
    limit = np.maximum(0, r - prev_end - 1)
    bases = np.concatenate((ref, qry))
    return (bases, ref_off, ref_len, qry_off, qry_len, ref_start, aln, (r + 1000).astype(np.uint32), q.astype(np.uint32),
            np.ones(n_ev, np.uint32), kind, limit.astype(np.uint32)), shift


def on_host(bases, ref_off, ref_len, qry_off, qry_len, ref_start, aln, ref_pos, qry_pos, length, kind, limit):
    """include/svx.h's loop for all events in lockstep."""
    a = aln.astype(np.int64)
    r, q, n = ref_pos.astype(np.int64) - ref_start[a], qry_pos.astype(np.int64), length.astype(np.int64)
    ro, qo, rl, ql = ref_off[a].astype(np.int64), qry_off[a].astype(np.int64), ref_len[a].astype(np.int64), qry_len[a].astype(np.int64)
    ins = kind == INS
    x0 = np.where(ins, qo + q + n, ro + r + n)
    x_ok0 = np.where(ins, q + n, r + n)
    x_len = np.where(ins, ql, rl)
    k = np.zeros(len(a), np.int64)
    live = np.flatnonzero(limit > 0)
    i = 0
    while len(live):
        i += 1
        e = live
        ok = (i <= r[e]) & (i <= q[e]) & (r[e] - i < rl[e]) & (q[e] - i < ql[e]) & (x_ok0[e] - i < x_len[e])
        e = e[ok]
        R, Q, X = bases[ro[e] + r[e] - i] & 0xDF, bases[qo[e] + q[e] - i] & 0xDF, bases[x0[e] - i] & 0xDF
        e = e[np.isin(R, ACGT) & (R == Q) & (X == R)]
        k[e] = i
        live = e[limit[e] > i]
    return k.astype(np.uint32)


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
    ap.add_argument("--events", type=int, default=1000000)
    ap.add_argument("--long", type=int, default=1000, help="one event in this many gets a shift of 100 to 5000 (0: none)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "shift_probe.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 repetitions")
    batch, shift = synthetic_batch(a.events, a.long)
    exp, host_wall = timed(lambda: on_host(*batch), a.reps)
    if not np.array_equal(exp, shift):
        sys.exit("the numpy walk does not find the shifts the batch was built with")
    ctx = _lib.Context(0)  # (raises without a device: a measurement path does not fall back)
    ctx.set_timing(True)
    ms = lambda xs: 1e3 * float(np.median(xs))
    # the uploads alone: the pool and the event columns into buffers that exist
    host_arrays = [np.ascontiguousarray(x) for x in batch]
    buffers = [ctx.dev_array(nbytes=max(1, x.nbytes)) for x in host_arrays]

    def upload():
        for x, d in zip(host_arrays, buffers):
            ctx._check(ctx.lib.svx_dev_upload(ctx.h, d.ptr, x.ctypes.data, x.nbytes))
        ctx.sync()
    _, up_wall = timed(upload, a.reps)
    settings = []
    equal = True
    for name, steps in (("wave_only", 0), ("2", 2), ("4", 4), ("8", 8), ("16", 16), ("32", 32), ("64", 64),
                        ("lane_only", _lib.SHIFT_LANES_ONLY), ("default", -1)):
        ctx.set_shift_lane_steps(steps)
        kernel_ms = []

        def device():
            out = ctx.indel_shift(*batch)
            kernel_ms.append(ctx.last_kernel_ms())
            return out
        got, wall = timed(device, a.reps)
        same = bool(np.array_equal(got, exp))
        equal = equal and same
        eff = _lib.SHIFT_LANE_STEPS if steps < 0 else steps  # (still matching behind `eff` steps with steps left: handed over)
        handed = 0 if steps == _lib.SHIFT_LANES_ONLY else int(((shift >= eff) & (batch[11] > eff)).sum())
        settings.append({"lane_steps": name if steps in (0, -1, _lib.SHIFT_LANES_ONLY) else steps,
                         "events_handed_to_the_wave_form": handed, "answers_equal": same,
                         "call_ms_median": ms(wall), "call_ms_min": 1e3 * min(wall), "call_ms_max": 1e3 * max(wall),
                         "kernels_ms_median": float(np.median([k[0] for k in kernel_ms[1:]])),
                         "kernels_ms_min": float(min(k[0] for k in kernel_ms[1:])), "kernels_ms_max": float(max(k[0] for k in kernel_ms[1:])),
                         "wave_launch_ms_median": float(np.median([k[1] for k in kernel_ms[1:]]))})
        print(json.dumps(settings[-1]), flush=True)
    ctx.set_shift_lane_steps(-1)
    ctx.set_timing(False)
    default = settings[-1]
    result = {
        "date": datetime.date.today().isoformat(), "box": socket.gethostname(), "note": "one box, synthetic; no real assembly has been shifted",
        "events": a.events, "alignments": 64, "pool_bytes": int(len(batch[0])), "column_bytes": int(sum(x.nbytes for x in batch[1:])),
        "long_events": int((shift >= 100).sum()), "shifted_events": int((shift > 0).sum()), "shifted_bases": int(shift.sum()),
        "built_default_lane_steps": _lib.SHIFT_LANE_STEPS, "wave_cols": _lib.SHIFT_WAVE_COLS, "reps": a.reps, "answers_equal": bool(equal),
        "settings": settings,
        "upload_ms_median": ms(up_wall), "upload_ms_min": 1e3 * min(up_wall), "upload_ms_max": 1e3 * max(up_wall),
        "upload_share_of_the_default_call": ms(up_wall) / default["call_ms_median"],
        "host_numpy_ms_median": ms(host_wall), "host_numpy_ms_min": 1e3 * min(host_wall), "host_numpy_ms_max": 1e3 * max(host_wall),
        "method": "median of `reps` calls after one untimed call; call: host clock around Context.indel_shift (uploads from pageable "
                  "memory, the launches, the read-backs, synchronise); kernels: HIP events behind the uploads, the host's wait for "
                  "the list's length included; upload: svx_dev_upload of the same arrays into existing buffers, then a "
                  "synchronise; host: numpy, all events in lockstep, one thread",
    }
    print(json.dumps({k: v for k, v in result.items() if k != "settings"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not equal:
        sys.exit("the device's answers differ from the host's")


if __name__ == "__main__":
    main()
