"""`svim-asm-cohort --gpus N` without a GPU: the CPU budget one cohort process of several plans with
(bamio.process_cpus), what the four defaults make of it, how the manifest is dealt out, and the launcher — with a stub in
the place of the child (cohort._child_command), so nothing here loads the library or needs a device."""
import builtins
import io
import json
import os
import signal
import subprocess
import sys
import time

import pytest

from svim_asm_amd import bamio, cohort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(monkeypatch, hw, quota=None, mask=None):
    """A host of `hw` hardware threads, a cgroup quota of `quota` CPUs (None: cpu.max says "max") and an affinity mask of
    `mask` CPUs (None: all of them) — through the three things process_cpus / host_cpus read."""
    real_open = builtins.open

    def fake_open(path, *a, **kw):
        if path == "/sys/fs/cgroup/cpu.max":
            return io.StringIO("max 100000\n" if quota is None else "%d 100000\n" % (quota * 100000))
        if isinstance(path, str) and path.startswith("/sys/fs/cgroup/cpu/"):
            raise OSError(path)
        return real_open(path, *a, **kw)
    monkeypatch.setattr(os, "cpu_count", lambda: hw)
    monkeypatch.setattr(builtins, "open", fake_open)
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(hw if mask is None else mask)))
    monkeypatch.delenv("SVX_NODE_PROCESSES", raising=False)


# (hardware threads, quota, mask, siblings) -> min(host_cpus(), mask) / siblings, at least 2; host_cpus() alone at 1 sibling
BUDGETS = [
    (16, None, None, 1, 16.0), (16, None, None, 8, 2.0), (16, 16, None, 1, 16.0), (16, 16, None, 8, 2.0),
    (96, None, None, 1, 96.0), (96, None, None, 8, 12.0), (96, 16, None, 1, 16.0), (96, 16, None, 8, 2.0),
    (256, None, None, 1, 256.0), (256, None, None, 8, 32.0), (256, 16, None, 1, 16.0), (256, 16, None, 8, 2.0),
    (256, None, 32, 8, 4.0), (256, 16, 32, 8, 2.0),
    (256, None, 32, 1, 256.0), (256, 16, 32, 1, 16.0),  # alone: host_cpus(), whatever the mask says
    (256, None, None, 2, 128.0), (256, 16, None, 2, 8.0), (256, 16, None, 4, 4.0), (256, 16, 8, 2, 4.0),
]


@pytest.mark.parametrize("hw,quota,mask,siblings,expected", BUDGETS)
def test_budget_arithmetic(monkeypatch, hw, quota, mask, siblings, expected):
    _host(monkeypatch, hw, quota, mask)
    assert bamio.host_cpus() == float(min(hw, quota or hw))
    assert bamio.process_cpus(siblings) == expected
    assert bamio.process_cpus(1) == bamio.host_cpus()
    # the same through the environment, which is how a child of the launcher (or a process started by hand) learns it
    monkeypatch.setenv("SVX_NODE_PROCESSES", str(siblings))
    assert bamio.process_cpus() == expected
    assert bamio.process_cpus(1) == bamio.host_cpus()  # (the argument wins)


def test_budget_ignores_what_is_not_a_positive_integer(monkeypatch):
    _host(monkeypatch, 256, None, 32)
    for bad in ("0", "-3", "eight", "2.5"):
        monkeypatch.setenv("SVX_NODE_PROCESSES", bad)
        bamio._ENV_WARNED.clear()
        with pytest.warns(UserWarning):
            assert bamio.process_cpus() == 256.0
    monkeypatch.setenv("SVX_NODE_PROCESSES", "")
    assert bamio.process_cpus() == 256.0
    monkeypatch.setenv("SVX_NODE_PROCESSES", "8")
    for bad in (0, -1, 2.5, "x"):
        bamio._ENV_WARNED.clear()
        with pytest.warns(UserWarning):
            assert bamio.process_cpus(bad) == 4.0  # (a refused argument: the environment's figure)
    assert bamio.process_cpus() == 4.0


def test_device_leg_default_judges_cpus_per_process(monkeypatch):
    """On at 12 CPUs per process, off at 32 — 8 processes on a 96- and on a 256-thread host —; SVX_BAM_DEVICE_INFLATE wins."""
    monkeypatch.delenv("SVX_BAM_DEVICE_INFLATE", raising=False)
    _host(monkeypatch, 96)
    monkeypatch.setenv("SVX_NODE_PROCESSES", "8")
    assert bamio.process_cpus() == 12.0 and bamio.default_device_inflate_percent() == 100
    _host(monkeypatch, 256)
    monkeypatch.setenv("SVX_NODE_PROCESSES", "8")
    assert bamio.process_cpus() == 32.0 and bamio.default_device_inflate_percent() == 0
    assert bamio.default_device_inflate_percent(12.0) == 100 and bamio.default_device_inflate_percent(32.0) == 0
    assert bamio.default_device_inflate_percent(24.0) == 100 and bamio.default_device_inflate_percent(24.5) == 0
    monkeypatch.delenv("SVX_NODE_PROCESSES")
    assert bamio.default_device_inflate_percent() == 0  # (alone on 256 threads: as before)
    monkeypatch.setenv("SVX_BAM_DEVICE_INFLATE", "35")
    assert bamio.default_device_inflate_percent() == 35 and bamio.default_device_inflate_percent(12.0) == 35
    monkeypatch.setenv("SVX_NODE_PROCESSES", "8")
    assert bamio.default_device_inflate_percent() == 35


def _plan(n_bams=2):
    cpus = bamio.process_cpus()
    workers = cohort.default_workers(cpus)
    threads = cohort.default_reader_threads(workers, n_bams, cpus)
    return cpus, workers, threads, cohort.default_lanes(workers, n_bams)


def test_sizing_of_the_defaults_under_the_budget(monkeypatch):
    """Diploid cohorts (two readers per worker).  The threads of all processes together stay within 1.5 x the CPUs, except
    where the floor of two threads per reader binds — pinned as what it is."""
    # 8 processes on 256 threads without a quota: 32 CPUs each
    _host(monkeypatch, 256)
    monkeypatch.setenv("SVX_NODE_PROCESSES", "8")
    assert _plan() == (32.0, 4, 6, 3)
    assert 8 * 4 * 2 * 6 == 384 == 1.5 * 256
    # 2 processes under the 16-CPU quota: 8 CPUs each
    _host(monkeypatch, 256, 16)
    monkeypatch.setenv("SVX_NODE_PROCESSES", "2")
    assert _plan() == (8.0, 2, 3, 2)
    assert 2 * 2 * 2 * 3 == 24 == 1.5 * 16
    # 4 processes under the 16-CPU quota: 4 CPUs each, 1.5 x 4 / 4 readers = 1.5 -> the floor of 2: 32 threads on 16 CPUs
    monkeypatch.setenv("SVX_NODE_PROCESSES", "4")
    assert _plan() == (4.0, 2, 2, 2)
    assert 4 * 2 * 2 * 2 == 32 > 1.5 * 16
    # what the same hosts computed per process before there was a budget (and still do alone): 48 threads per reader, leg off
    _host(monkeypatch, 256)
    assert _plan() == (256.0, 4, 48, 3)
    _host(monkeypatch, 256, 16)
    assert _plan() == (16.0, 4, 3, 3)
    # without the argument the functions ask for the budget themselves
    monkeypatch.setenv("SVX_NODE_PROCESSES", "2")
    assert cohort.default_workers() == 2 and cohort.default_reader_threads(2, 2) == 3


def _samples(n, n_bams=2):
    return [("/wd/%d" % k, ["s%d_h%d.bam" % (k, h) for h in range(n_bams)]) for k in range(n)]


def test_dealing_is_round_robin():
    samples = _samples(7)
    shares = cohort.deal(samples, 3)
    assert [len(s) for s in shares] == [3, 2, 2]
    assert shares[0] == [samples[0], samples[3], samples[6]] and shares[1] == [samples[1], samples[4]] and \
        shares[2] == [samples[2], samples[5]]
    assert sorted(s for share in shares for s in share) == sorted(samples)
    assert [len(s) for s in cohort.deal(_samples(2), 4)] == [1, 1, 0, 0]


STUB = r"""
import json, os, sys, time
share, device = sys.argv[2], int(sys.argv[sys.argv.index("--device") + 1])
plan = json.load(open(os.environ["STUB_PLAN"]))
with open(os.path.join(plan["out"], "child_%d_%d.json" % (device, os.getpid())), "w") as f:
    json.dump({"argv": sys.argv[1:], "siblings": os.environ.get("SVX_NODE_PROCESSES"), "share": open(share).read()}, f)
time.sleep(plan.get("sleep", {}).get(str(device), 0))
with open(os.path.join(plan["out"], "done_%d_%d" % (device, os.getpid())), "w") as f:
    f.write("done")
sys.exit(plan.get("status", {}).get(str(device), 0))
"""


@pytest.fixture
def stub(tmp_path, monkeypatch):
    """Puts a stub in the place of the child; returns (set_plan, records): what the children wrote when they ran."""
    out = tmp_path / "stub_out"
    out.mkdir()
    plan_path = tmp_path / "stub_plan.json"

    def set_plan(**plan):
        plan_path.write_text(json.dumps(dict(plan, out=str(out))))
    set_plan()
    monkeypatch.setenv("STUB_PLAN", str(plan_path))
    monkeypatch.setattr(cohort, "_child_command", lambda mode, share, genome, device, rest:
                        [sys.executable, "-c", STUB, mode, share, genome, "--device", str(device)] + list(rest))

    def records():
        recs = [json.load(open(out / n)) for n in sorted(os.listdir(out)) if n.startswith("child_")]
        return recs, len([n for n in os.listdir(out) if n.startswith("done_")])
    return set_plan, records


def _manifest(tmp_path, n, n_bams=2):
    path = tmp_path / "cohort.tsv"
    path.write_text("# a cohort\n" + "".join("%s %s\n" % (tmp_path / ("wd%d" % k), " ".join("s%d_h%d.bam" % (k, h) for h in range(n_bams)))
                                              for k in range(n)))
    return str(path)


def _device_of(rec):
    return int(rec["argv"][rec["argv"].index("--device") + 1])


def test_launcher_starts_one_child_per_device(tmp_path, stub):
    set_plan, records = stub
    manifest = _manifest(tmp_path, 7)
    assert cohort.main(["diploid", manifest, "ref.fa", "--gpus", "3", "--devices=2,0,1", "--min_sv_size", "50",
                        "--cohort_workers", "2"]) == 0
    recs, done = records()
    assert len(recs) == 3 and done == 3
    lines = [l for l in open(manifest) if not l.startswith("#")]
    seen = []
    for rec in recs:
        a = rec["argv"]
        k = [2, 0, 1].index(_device_of(rec))  # the child's place in the deal
        # today's single-process command on its own share: --device d_k, the other options as given, no --gpus / --devices
        assert a[0] == "diploid" and a[2] == "ref.fa" and a[3:] == ["--device", str([2, 0, 1][k]), "--min_sv_size", "50", "--cohort_workers", "2"]
        assert not [x for x in a if x.startswith(("--gpus", "--devices"))]
        assert rec["siblings"] == "3"
        mine = [tuple(l.split()) for l in rec["share"].splitlines()]
        assert mine == [tuple(l.split()) for l in lines[k::3]]
        assert not os.path.exists(a[1])  # the shares' directory is gone
        seen += mine
    assert sorted(seen) == sorted(tuple(l.split()) for l in lines)  # every sample exactly once


def test_launcher_does_not_start_a_child_without_samples(tmp_path, stub):
    set_plan, records = stub
    assert cohort.main(["haploid", _manifest(tmp_path, 2, 1), "ref.fa", "--gpus", "4"]) == 0
    recs, done = records()
    assert sorted(_device_of(r) for r in recs) == [0, 1] and done == 2
    assert [r["siblings"] for r in recs] == ["2", "2"]
    assert all(len(r["share"].splitlines()) == 1 for r in recs)


def test_one_gpu_goes_through_the_same_launcher(tmp_path, stub):
    set_plan, records = stub
    assert cohort.main(["diploid", _manifest(tmp_path, 3), "ref.fa", "--gpus=1"]) == 0
    recs, done = records()
    assert len(recs) == 1 and done == 1 and recs[0]["siblings"] == "1" and _device_of(recs[0]) == 0
    assert len(recs[0]["share"].splitlines()) == 3
    # two processes on one device
    assert cohort.main(["diploid", _manifest(tmp_path, 3), "ref.fa", "--gpus", "2", "--devices", "0,0"]) == 0
    recs, done = records()
    assert len(recs) == 3 and done == 3 and [_device_of(r) for r in recs] == [0, 0, 0]


def test_a_failed_child_does_not_stop_the_others(tmp_path, stub):
    set_plan, records = stub
    set_plan(status={"1": 3}, sleep={"0": 0.5, "2": 0.5})  # child 1 fails at once; the others are still at work then
    assert cohort.main(["diploid", _manifest(tmp_path, 6), "ref.fa", "--gpus", "3"]) == 3
    recs, done = records()
    assert len(recs) == 3 and done == 3


def test_a_child_killed_by_a_signal_counts_as_failure(tmp_path, monkeypatch, stub):
    set_plan, records = stub
    monkeypatch.setattr(cohort, "_child_command", lambda mode, share, genome, device, rest:
                        [sys.executable, "-c", "import os, signal; os.kill(os.getpid(), signal.SIGKILL)" if device == 1 else "pass"])
    assert cohort.main(["diploid", _manifest(tmp_path, 2), "ref.fa", "--gpus", "2"]) != 0


@pytest.mark.parametrize("extra", [["--gpus", "0"], ["--gpus", "17"], ["--gpus", "2", "--devices", "0"],
                                   ["--gpus", "2", "--devices", "0,1,2"], ["--gpus", "2", "--device", "1"],
                                   ["--gpus", "2", "--device=1"], ["--gpus", "two"], ["--devices", "0,1"], ["--gpus"],
                                   ["--gpus", "2", "--devices", "0,-1"]])
def test_refused_requests_return_2_and_start_nothing(tmp_path, stub, capsys, extra):
    set_plan, records = stub
    assert cohort.main(["diploid", _manifest(tmp_path, 4), "ref.fa"] + extra) == 2
    assert records() == ([], 0)
    assert "svim-asm-cohort: " in capsys.readouterr().err


def test_a_malformed_manifest_fails_in_the_parent(tmp_path, stub):
    set_plan, records = stub
    bad = tmp_path / "bad.tsv"
    bad.write_text("%s a.bam b.bam\n%s only_one.bam\n" % (tmp_path / "w0", tmp_path / "w1"))
    with pytest.raises(ValueError):
        cohort.main(["diploid", str(bad), "ref.fa", "--gpus", "2"])
    assert records() == ([], 0)


def test_sixteen_children_is_the_limit_that_runs(tmp_path, stub):
    set_plan, records = stub
    assert cohort.main(["haploid", _manifest(tmp_path, 16, 1), "ref.fa", "--gpus", "16"]) == 0
    recs, done = records()
    assert sorted(_device_of(r) for r in recs) == list(range(16)) and done == 16 and {r["siblings"] for r in recs} == {"16"}


PARENT = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
from svim_asm_amd import cohort
STUB = %(stub)r
cohort._child_command = lambda mode, share, genome, device, rest: \
    [sys.executable, "-c", STUB, mode, share, genome, "--device", str(device)] + list(rest)
rc = cohort.main(sys.argv[1:])
maps = open("/proc/self/maps").read()
print(json.dumps({"rc": rc, "libsvx": "libsvx" in maps, "hip": "libamdhip64" in maps or "libhsa-runtime" in maps,
                  "visible": os.environ.get("HIP_VISIBLE_DEVICES")}))
sys.exit(rc)
"""


def _parent_script(tmp_path):
    path = tmp_path / "parent.py"
    path.write_text(PARENT % {"root": ROOT, "stub": STUB})
    return str(path)


def test_the_parent_maps_no_device_library(tmp_path, stub, monkeypatch):
    """In a process of its own (other tests of this session load the library): after main() the launcher has mapped neither
    libsvx nor the HIP runtime, and has not narrowed the visible devices."""
    monkeypatch.delenv("HIP_VISIBLE_DEVICES", raising=False)
    r = subprocess.run([sys.executable, _parent_script(tmp_path), "diploid", _manifest(tmp_path, 4), "ref.fa", "--gpus", "2",
                        "--devices", "1,1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"rc": 0, "libsvx": False, "hip": False, "visible": None}
    recs, done = stub[1]()
    assert len(recs) == 2 and done == 2
    # one log line per child: its device, its samples, its status
    assert len([l for l in r.stderr.splitlines() if "CHILD: device 1, 2 sample(s), status 0" in l]) == 2


@pytest.mark.parametrize("signo,status", [(signal.SIGTERM, 143), (signal.SIGINT, 130)])
def test_a_signal_to_the_parent_ends_the_children(tmp_path, stub, signo, status):
    set_plan, records = stub
    set_plan(sleep={"0": 60, "1": 60})
    parent = subprocess.Popen([sys.executable, _parent_script(tmp_path), "diploid", _manifest(tmp_path, 4), "ref.fa", "--gpus", "2"],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        deadline = time.time() + 60
        while len(records()[0]) < 2 and time.time() < deadline:  # both children are up (and asleep)
            time.sleep(0.05)
        recs, done = records()
        assert len(recs) == 2 and done == 0
        pids = [int(n.split("_")[2].split(".")[0]) for n in os.listdir(tmp_path / "stub_out") if n.startswith("child_")]
        t0 = time.time()
        parent.send_signal(signo)  # (to the parent alone: a session of its own, nothing is sent to the group)
        parent.communicate(timeout=20)
        assert parent.returncode == status
        assert time.time() - t0 < 8
        for pid in pids:  # the children are gone (reaped by the parent: the pid names no process)
            with pytest.raises(ProcessLookupError):
                os.kill(pid, 0)
        assert records()[1] == 0  # neither of them ran to its end
        assert not os.path.exists(os.path.dirname(recs[0]["argv"][1]))
    finally:
        if parent.poll() is None:
            parent.kill()
        try:
            os.killpg(parent.pid, signal.SIGKILL)  # whatever the session still holds, should the test have failed
        except (ProcessLookupError, PermissionError):
            pass
