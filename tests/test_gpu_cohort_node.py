"""`svim-asm-cohort --gpus N` on the device: the real command as a parent with one child per `--devices` entry — two of
them sharing device 0, which is how a one-GPU machine runs the node's configuration — against the real reference's VCFs of
the config-1 sample.  Every command is a fresh process with a time limit of its own; this process only waits."""
import os
import re
import signal
import subprocess
import sys

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.spawns_gpu_children]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "config1")
BAMS = {"diploid": ["hap1.bam", "hap2.bam"], "haploid": ["hap1.bam"]}


def _manifest(tmp_path, mode, n=4, name="cohort.tsv", broken=()):
    """`n` samples on the config-1 BAMs, a working directory each; `broken`: samples whose first BAM does not exist."""
    dirs = [tmp_path / ("%s_%s_%d" % (name.split(".")[0], mode, k)) for k in range(n)]
    lines = []
    for k, wd in enumerate(dirs):
        bams = [os.path.join(GOLD, b) for b in BAMS[mode]]
        if k in broken:
            bams[0] = str(tmp_path / "no_such_file.bam")
        lines.append("%s %s\n" % (wd, " ".join(bams)))
    path = tmp_path / ("%s_%s" % (mode, name))
    path.write_text("".join(lines))
    return str(path), dirs


def _cohort(mode, manifest, extra, timeout=300):
    env = dict(os.environ)
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SVX_NODE_PROCESSES"):
        env.pop(name, None)
    # a session of its own: past the limit the command AND the children it started are ended, and the test fails
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "bin", "svim-asm-cohort"), mode, manifest, os.path.join(GOLD, "ref.fa")]
                         + list(extra), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        out = p.communicate(timeout=timeout)[0]
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except (ProcessLookupError, PermissionError):
            pass
        out = p.communicate()[0]
        pytest.fail("svim-asm-cohort %s took more than %d s:\n%s" % (" ".join(extra), timeout, out[-3000:]))
    return subprocess.CompletedProcess(p.args, p.returncode, out)


def _masked(path):
    return "".join(l for l in open(path) if not l.startswith("##fileDate="))


@pytest.mark.parametrize("mode", ["diploid", "haploid"])
def test_two_processes_sharing_one_device_write_the_reference_vcfs(tmp_path, mode):
    golden = open(os.path.join(GOLD, "%s_default.vcf" % mode)).read()
    manifest, dirs = _manifest(tmp_path, mode)
    r = _cohort(mode, manifest, ["--gpus", "2", "--devices", "0,0"])
    assert r.returncode == 0, r.stdout
    for wd in dirs:
        assert _masked(wd / "variants.vcf") == golden
    assert len(re.findall(r"CHILD: device 0, 2 sample\(s\), status 0", r.stdout)) == 2
    # --gpus 1: the same launcher, one child, the same files
    manifest, dirs = _manifest(tmp_path, mode, name="one.tsv")
    r = _cohort(mode, manifest, ["--gpus", "1"])
    assert r.returncode == 0, r.stdout
    for wd in dirs:
        assert _masked(wd / "variants.vcf") == golden
    assert len(re.findall(r"CHILD: device 0, 4 sample\(s\), status 0", r.stdout)) == 1


def test_a_refused_input_does_not_stop_the_other_child(tmp_path):
    """Sample 1 goes to the second child (1 mod 2) and names a BAM that does not exist: the parent's status says so, the
    first child's samples (0 and 2) are complete and the reference's."""
    manifest, dirs = _manifest(tmp_path, "diploid", broken=(1,))
    r = _cohort("diploid", manifest, ["--gpus", "2", "--devices", "0,0"])
    assert r.returncode != 0, r.stdout
    golden = open(os.path.join(GOLD, "diploid_default.vcf")).read()
    for k in (0, 2):
        assert _masked(dirs[k] / "variants.vcf") == golden
    assert not os.path.exists(dirs[1] / "variants.vcf")
    assert len(re.findall(r"CHILD: device 0, 2 sample\(s\), status 0", r.stdout)) == 1
    assert len(re.findall(r"CHILD: device 0, 2 sample\(s\), (status [1-9]|killed)", r.stdout)) == 1


def test_every_child_logs_the_budget_it_planned_with(tmp_path):
    """Once per child, at its start: the figure is bamio.process_cpus(2) as this process computes it (same host, same
    cgroup, same affinity mask) and the workers and reader threads are what the defaults make of it."""
    from svim_asm_amd import bamio, cohort
    manifest, dirs = _manifest(tmp_path, "diploid")
    r = _cohort("diploid", manifest, ["--gpus", "2", "--devices", "0,0"])
    assert r.returncode == 0, r.stdout
    found = re.findall(r"BUDGET: ([0-9.]+) CPUs for this process \((\d+) cohort process\(es\) on the node\): (\d+) worker\(s\), "
                       r"(\d+) thread\(s\) per reader", r.stdout)
    print(found)
    assert len(found) == 2
    cpus = bamio.process_cpus(2)
    workers = min(cohort.default_workers(cpus), 2)  # (two samples per child: no more workers than groups)
    for got_cpus, siblings, got_workers, got_threads in found:
        assert float(got_cpus) == pytest.approx(cpus, abs=0.005) and int(siblings) == 2
        assert int(got_workers) == workers and int(got_threads) == cohort.default_reader_threads(workers, 2, cpus)
