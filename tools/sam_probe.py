"""Who should turn a SAM's CIGAR strings into words: the reader's threads or the device.

    python tools/sam_probe.py [--ops 2500000] [--reps 3] [--out table.json]

A haplotype's worth of CIGAR operations (svim_asm_amd.synth.synth_cigar_batch: the full-size sample's record and
operation counts) is rendered as text and as a SAM file whose SEQ fields are `*` (the bases are the same bytes for both
paths: they are hopped over).  Measured, medians of `--reps` interleaved repetitions:
  host parse     svx_cigar_text_parse on 1 and on 16 threads
  kernels        svx_cigar_text_parse_dev, device time of its launches (svx_ctx_last_kernel_ms)
  load()         bamio.AlignmentFile(sam, device=0).load() + device_pool(wait=True) with SVX_SAM_DEVICE=0 and =1,
                 a fresh handle each time, the two settings in turn
Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=2_500_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    from svim_asm_amd import _lib, bamio, synth
    b = synth.synth_cigar_batch(seed=1, ops_target=a.ops)
    words, off = b["cigar"], b["aln_off"].astype(np.int64)
    ops = np.frombuffer(b"MIDNSHP=X", np.uint8)
    strings = []
    for i in range(len(off) - 1):
        w = words[off[i]:off[i + 1]]
        strings.append("".join("%d%s" % (l, chr(o)) for l, o in zip((w >> 4).tolist(), ops[w & 15].tolist())))
    text = np.frombuffer("".join(strings).encode(), np.uint8)
    rec_off = np.zeros(len(strings) + 1, np.uint64)
    np.cumsum([len(s) for s in strings], out=rec_off[1:])
    n, cap = len(strings), len(text) // 2 + 1
    lib = _lib.load()
    o_words, o_off = np.empty(cap, np.uint32), np.zeros(n + 1, np.uint64)
    o_rl, o_st = np.zeros(n, np.int32), np.zeros(n, np.uint32)

    def host(threads):
        t0 = time.perf_counter()
        rc = lib.svx_cigar_text_parse(text.ctypes.data, len(text), rec_off.ctypes.data, n, o_words.ctypes.data, cap, o_off.ctypes.data,
                                      o_rl.ctypes.data, o_st.ctypes.data, threads)
        assert rc == 0 and not o_st.any() and np.array_equal(o_words[:len(words)], words)
        return (time.perf_counter() - t0) * 1e3

    ctx = _lib.Context(0)
    ctx.set_timing(True)

    def kernels():
        out = ctx.cigar_text_parse(text, rec_off)
        assert np.array_equal(out["words"], words)
        return ctx.last_kernel_ms()[0]

    d = tempfile.mkdtemp(prefix="sam_probe_")
    sam = os.path.join(d, "probe.sam")
    names = ["c%d" % k for k in range(len(b["contig_lengths"]))]
    order = np.random.default_rng(1).permutation(n)
    with open(sam, "w") as f:
        f.write("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, min(int(l), 2 ** 31 - 1)) for nm, l in zip(names, b["contig_lengths"])))
        for i in order.tolist():
            f.write("q%d\t0\t%s\t%d\t60\t%s\t*\t0\t0\t*\t*\n" % (i, names[int(b["tid"][i])], int(b["ref_start"][i]) + 1, strings[i]))

    def load(device_parse):
        os.environ["SVX_SAM_DEVICE"] = "1" if device_parse else "0"
        f = bamio.AlignmentFile(sam, device=0, threads=a.threads)
        t0 = time.perf_counter()
        f.load()
        f.device_pool(wait=True)
        ms = (time.perf_counter() - t0) * 1e3
        assert f.parsed_on_device == bool(device_parse) and len(f._cigar) == len(words)
        f.close()
        return ms

    load(0), load(1), kernels(), host(1)  # (first touches: pages, streams, code objects)
    res = {k: [] for k in ("host_1_thread_ms", "host_%d_threads_ms" % a.threads, "kernels_ms", "load_host_ms", "load_device_ms")}
    for _ in range(a.reps):
        res["host_1_thread_ms"].append(host(1))
        res["host_%d_threads_ms" % a.threads].append(host(a.threads))
        res["kernels_ms"].append(kernels())
        res["load_host_ms"].append(load(0))
        res["load_device_ms"].append(load(1))
    table = {"ops": int(len(words)), "records": n, "text_bytes": int(len(text)), "reps": a.reps,
             "median": {k: round(statistics.median(v), 3) for k, v in res.items()}, "all": {k: [round(x, 3) for x in v] for k, v in res.items()}}
    print(json.dumps(table))
    if a.out:
        json.dump(table, open(a.out, "w"), indent=1)
    os.remove(sam)
    os.rmdir(d)


if __name__ == "__main__":
    main()
