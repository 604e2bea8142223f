"""bench.py --dump-outputs: what the last timed step computed, as the caller of svx_collect_batch receives it, written as
float64 .npy files under 64 MB with a fixed row sample where an output is larger.  CPU only: host arrays stand in for
the step's device buffers."""
import os
import types

import numpy as np
import pytest

from tests.test_bench_rank_record import _bench


class _Buf(object):
    """DeviceArray.download over a host array."""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a)

    def download(self, dtype, count=None):
        b = self.a.view(np.uint8).view(dtype)
        return (b if count is None else b[:int(count)]).copy()


def _resident(seed, n_sig=5000, n_reads=300, cap=8000):
    rng = np.random.default_rng(seed)
    slots = rng.integers(2, 5, n_reads)
    post_off = np.concatenate(([0], np.cumsum(slots * (slots + 3) // 2))).astype(np.uint64)
    n_segs = int(slots.sum())
    sig = [rng.integers(0, 2 ** 32, cap, dtype=np.uint32) for _ in range(4)] + [rng.integers(0, 6, cap, dtype=np.uint8)]
    raw = rng.integers(-2 ** 31, 2 ** 31, (n_segs, 8), dtype=np.int32)
    post = rng.integers(-2 ** 31, 2 ** 31, (int(post_off[-1]), 8), dtype=np.int32)
    cnt = rng.integers(0, slots * (slots + 3) // 2 + 1).astype(np.uint32)
    rc = types.SimpleNamespace(ctx=types.SimpleNamespace(sync=lambda: None), cap=cap,
                               case=dict(n_segs=n_segs, n_reads=n_reads, post_off=post_off),
                               o=[_Buf(s) for s in sig] + [_Buf(np.array([n_sig], np.uint64))],
                               d_raw=_Buf(raw), d_post=_Buf(post), d_cnt=_Buf(cnt))
    rc.n_sig = lambda: int(rc.o[5].a[0])
    return rc, sig, raw, post, post_off, cnt


def test_collect_outputs_are_what_the_caller_receives():
    bench = _bench()
    rc, sig, raw, post, post_off, cnt = _resident(1)
    out = bench.collect_outputs(rc)
    assert int(out["n_sig"][0]) == 5000
    for col, key in zip(sig, bench.SIG_KEYS):
        assert np.array_equal(out["sig_" + key], col[:5000])
    assert np.array_equal(out["raw"], raw[:, :7])
    packed = [post[int(post_off[r]):int(post_off[r]) + int(cnt[r]), :7] for r in range(len(cnt))]
    assert np.array_equal(out["post"], np.concatenate(packed))
    assert np.array_equal(out["post_first"], np.concatenate(([0], np.cumsum(cnt))))


def test_collect_outputs_refuse_a_count_beyond_the_capacity():
    bench = _bench()
    rc = _resident(2, n_sig=9000, cap=8000)[0]
    with pytest.raises(SystemExit):
        bench.collect_outputs(rc)


def test_split_outputs_are_what_the_callers_receive():
    import torch
    bench = _bench()
    rng = np.random.default_rng(4)
    cols = [rng.integers(-2 ** 31, 2 ** 31, 3000, dtype=np.int32) for _ in range(4)] + [rng.integers(0, 6, 3000, dtype=np.uint8)]
    raw = rng.integers(-2 ** 31, 2 ** 31, (700, 8), dtype=np.int32)
    o = [torch.from_numpy(c) for c in cols] + [torch.tensor([2500], dtype=torch.int64)]
    out = bench.split_outputs(o, torch.from_numpy(raw), 3000)
    assert int(out["n_sig"][0]) == 2500
    for col, key in zip(cols, bench.SIG_KEYS):
        assert np.array_equal(out["sig_" + key], col[:2500].view(np.uint32) if col.dtype == np.int32 else col[:2500])
    assert np.array_equal(out["raw"], raw[:, :7])
    with pytest.raises(SystemExit):
        bench.split_outputs(o, torch.from_numpy(raw), 2000)


def test_dump_is_float64_sampled_alike_and_repeatable(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_ROW_CAP", dict(bench.DUMP_ROW_CAP, sig=1000))
    rc, sig = _resident(3)[:2]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, bench.collect_outputs(rc))
    bench.dump_outputs(b, bench.collect_outputs(rc))
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert "sig_rows.npy" in names and "raw_rows.npy" not in names
    got = {n[:-4]: np.load(os.path.join(a, n)) for n in names}
    assert all(v.dtype == np.float64 for v in got.values())
    assert all(np.array_equal(v, np.load(os.path.join(b, n + ".npy"))) for n, v in got.items())
    rows = got["sig_rows"].astype(np.int64)
    assert len(rows) == 1000 and np.all(np.diff(rows) > 0) and rows[-1] < 5000
    for col, key in zip(sig, bench.SIG_KEYS):
        assert np.array_equal(got["sig_" + key], col[rows].astype(np.float64))


def test_an_empty_output_is_not_written(tmp_path):
    """The bench workload's reads yield no derived records: `post` is empty and is left out (a stale post.npy of an
    earlier dump into the same directory goes too); the per-read first index is still written."""
    bench = _bench()
    rc = _resident(5)[0]
    rc.d_cnt = _Buf(np.zeros(rc.case["n_reads"], np.uint32))
    out = bench.collect_outputs(rc)
    assert out["post"].shape == (0, 7)
    d = str(tmp_path)
    np.save(os.path.join(d, "post.npy"), np.ones(3))
    bench.dump_outputs(d, out)
    names = sorted(n[:-4] for n in os.listdir(d))
    assert "post" not in names
    assert names == sorted(n for n in out if n != "post")
    assert np.array_equal(np.load(os.path.join(d, "post_first.npy")), np.zeros(rc.case["n_reads"] + 1))


def test_dump_stays_under_64_mb_at_every_cap(tmp_path):
    bench = _bench()
    widths = {"sig_" + k: 1 for k in bench.SIG_KEYS}
    widths.update(raw=7, post=7, post_first=1)
    out = {"n_sig": np.array([1])}
    for name, w in widths.items():  # every group one row over its cap
        rows = bench.DUMP_ROW_CAP["sig" if name.startswith("sig_") else name] + 1
        out[name] = np.zeros((rows, w) if w > 1 else rows, np.uint8)
    bench.dump_outputs(str(tmp_path), out)
    assert sum(os.path.getsize(os.path.join(str(tmp_path), n)) for n in os.listdir(str(tmp_path))) <= 64 << 20
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(9 << 20, np.uint8)})
