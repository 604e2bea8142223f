"""`svim-asm-cohort`: many samples in one process — what the reference does one invocation per sample
(svim-asm:74-141) — as a STREAM: the manifest is cut into groups of G samples (default 1); a group is opened, its COLLECT
goes out as one device submission (svx_collect_batch over every BAM of the group: at G = the whole manifest the batch size
at which the CIGAR walk runs at HBM speed, bench.py's headline workload), then PAIR and the VCF per sample exactly as
`svim-asm haploid|diploid` produces them.  K workers (threads, each with a device context and stream of its own) take
the groups in manifest order, so the ingest of one group — the BAM readers' own threads, the device's share of the
inflate work on by default here — runs while another group is in PAIR or writing its VCF; at most K groups are in memory
whatever the manifest's length.  The process pays interpreter start and HIP bring-up once.

    svim-asm-cohort diploid MANIFEST GENOME [--cohort_workers K] [--cohort_group G] [--cohort_threads T] [--cohort_lanes L] [the options of svim-asm diploid]
    svim-asm-cohort haploid MANIFEST GENOME [--cohort_workers K] [--cohort_group G] [--cohort_threads T] [--cohort_lanes L] [the options of svim-asm haploid]

MANIFEST: one sample per line, whitespace-separated — working_dir bam (haploid) or working_dir bam1 bam2 (diploid), each a
sorted, indexed BAM or an uncompressed SAM in any record order (PAF input is not taken here: a manifest line has no place
for the query assembly a PAF needs, and the --query* options of `svim-asm haploid|diploid` are ignored by this command);
lines starting with # are skipped.  Every sample gets its own working_dir/variants.vcf, byte-identical to the one
the single-sample command writes.  K defaults to 4 (2 below 12 CPUs' worth of time), G to 1; `--cohort_group 0` = the whole
manifest in one submission (the round-5 behaviour); T threads per BAM reader (default: the process's CPUs shared out among
the readers in flight, default_reader_threads); L inflate lanes on the device (default_lanes: one per three readers in flight).  The reference has no such mode; this is an addition on top of the
drop-in command, which is unchanged.

    svim-asm-cohort haploid|diploid MANIFEST GENOME --gpus N [--devices d0,d1,...] [all other options]

The command for a node: a parent that never touches the GPU deals the manifest out round-robin (sample i to child i mod N)
and starts one fresh child per device — each of them the single-process command above on its own share with `--device d_k`.
`--devices` names the device of each child (default 0..N-1, N of them, 1 <= N <= 16; an index may repeat: two processes then
share that device); `--device` together with `--gpus` is an error.  Every child runs with SVX_NODE_PROCESSES=<children
started>, from which it takes its share of the node's CPUs (bamio.process_cpus: workers, reader threads and the device's
share of the inflate work follow the CPUs per PROCESS).  A failed child does not stop the others; the parent's status is the
worst of theirs; SIGINT / SIGTERM are passed on as SIGTERM and answered with 130 / 143 once every child is gone.  Processes
started by hand set SVX_NODE_PROCESSES themselves.

    svim-asm-cohort haploid|diploid MANIFEST GENOME --merge OUT_DIR [all other options]

`--keep_candidates` leaves every sample's final table beside its VCF (working_dir/candidates.svxt); `--merge OUT_DIR` implies
it and, once every sample has returned 0, merges the tables into OUT_DIR/cohort.vcf with one genotype column per sample
(svim-asm-merge, SVIM_MERGE.py): in this process on its default context, or — with `--gpus N` — in one more fresh child on the
first listed device, started when all children have exited with 0; its status counts towards the parent's.  If a sample
failed, no merge is attempted.

`--keep_coverage` leaves every sample's coverage.svxt beside its VCF; `--merge OUT_DIR --genotype_non_carriers` implies it and
passes the option (and `--genotype_margin N`) on to the merge, in the single process and to the merge child of `--gpus N`: the
samples without a call in a record are then genotyped per haplotype from their assemblies' coverage.

`--callable_bed` (with `--callable_min_length N`) leaves every sample's callable.bed beside its VCF — the ranges exactly one
alignment per haplotype lies over —, also under `--gpus N`; with `--merge OUT_DIR` it implies `--keep_coverage` and is passed on
to the merge, which writes OUT_DIR/cohort.callable.bed with the number of samples per range."""
import gc
import logging
import os
import sys

from svim_asm_amd import SVIM_COLLECT, _timeline, cli, shard
from svim_asm_amd.fasta import BgzfFormatError, FastaFile, MissingGziError
from svim_asm_amd.SVIM_COMBINE import write_vcf_table
from svim_asm_amd.SVIM_input_parsing import parse_arguments


def read_manifest(path, n_bams):
    samples = []
    for no, line in enumerate(open(path), 1):
        fields = line.split()
        if not fields or fields[0].startswith("#"):
            continue
        if len(fields) != 1 + n_bams:
            raise ValueError("%s:%d: expected a working directory and %d BAM path(s)" % (path, no, n_bams))
        samples.append((os.path.abspath(fields[0]), fields[1:]))
    if not samples:
        raise ValueError("%s names no sample" % path)
    return samples


def _take_option(rest, name, default, convert=int):
    """Removes `name VALUE` (or name=VALUE) from the argument list of the reference's parser; returns int(VALUE)
    (convert(VALUE) where the value is not a number: --devices)."""
    out, value, k = [], default, 0
    while k < len(rest):
        a = rest[k]
        if a == name and k + 1 < len(rest):
            value = convert(rest[k + 1])
            k += 2
            continue
        if a.startswith(name + "="):
            value = convert(a.split("=", 1)[1])
            k += 1
            continue
        out.append(a)
        k += 1
    return out, value


COHORT_DEVICE_INFLATE_PERCENT = 100
COHORT_DEVICE_INFLATE_WAIT_MS = int(os.environ.get("SVX_COHORT_INFLATE_WAIT_MS") or 3000)  # (the variable: tools/r06_cohort_ab.py)


def device_numa_cpus(device):
    """(PCI address, NUMA node, CPUs of that node) of a visible HIP device, from svx_device_pci_bus_id and sysfs; node and
    CPUs are None where the platform does not say (a single-node host, a container without the sysfs entries)."""
    import ctypes as C
    from svim_asm_amd import _lib
    buf = C.create_string_buffer(32)
    if _lib.load().svx_device_pci_bus_id(int(device), buf, 32) != 0:
        return None, None, None
    addr = buf.value.decode().lower()
    try:
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % addr).read())
        if node < 0:
            return addr, None, None
        cpus = set()
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
        allowed = os.sched_getaffinity(0)
        cpus &= allowed
        return addr, node, (sorted(cpus) or None)
    except (OSError, ValueError):
        return addr, None, None


def bind_to_device_node(device):
    """Keeps the calling thread — and every thread it starts from now on: a reader's pool, the writers — on the CPUs of
    the NUMA node the device hangs on: with one cohort process per GPU of a node the processes then neither share cores
    nor read their page-locked pools across sockets.  Returns what was done, for the log."""
    addr, node, cpus = device_numa_cpus(device)
    if cpus:
        try:
            os.sched_setaffinity(0, cpus)
            return "device %d (%s): NUMA node %d, threads bound to its %d CPUs" % (device, addr, node, len(cpus))
        except OSError as e:
            return "device %d (%s): NUMA node %d, binding refused (%s)" % (device, addr, node, e)
    return "device %d (%s): no NUMA node reported, threads not bound" % (device, addr or "address unknown")


def default_workers(cpus=None):
    """`cpus`: the process's budget (bamio.process_cpus, computed once by main before it binds its threads); None: asked now."""
    from svim_asm_amd import bamio
    return 4 if (bamio.process_cpus() if cpus is None else cpus) >= 12 else 2


def default_lanes(workers, n_bams):
    """Inflate lanes for `workers` workers of `n_bams` readers each (the workers are what the process's CPU budget gave it:
    default_workers): one per three readers in flight, at least the library's two.  A lane is held for a call's 50-70 ms and
    the workers are elsewhere most of the time, so a few lanes serve them;
    every further lane that is busy at the same time shares the same host link and costs CPU-seconds (N = 16 full-size
    samples, 4 workers, one box, twice: 2 lanes 8.4-8.9 samples/s at 0.79 CPU-seconds per sample, 3 lanes 8.6-9.0 at 0.85,
    8 lanes 7.7-8.6 at 1.0; another box at N = 24 with a 400 ms wait: 6.2 on 2 lanes — calls that found no lane in time
    decoded on the threads —, 9.2 on 4, 10.0 on 8: profiles/r06_cohort_lanes.txt).  What a call must not do is give up on the
    lane: COHORT_DEVICE_INFLATE_WAIT_MS."""
    return max(2, min(16, (workers * n_bams + 1) // 3))


def default_reader_threads(workers, n_bams, cpus=None):
    """Threads per BAM reader: the CPUs' worth of time the process gets (hardware threads or the cgroup's quota, divided by
    the cohort processes on the node: bamio.process_cpus — `cpus` when the caller has computed it, which main does once, before
    its workers narrow the affinity mask) shared out among the readers of the groups in flight.  Under a quota (cpu.max) a
    process that runs more threads than it has CPUs
    spends a period's budget in a fraction of the period and then stands still for the rest of it: the single-sample command
    may do that once (its record walk is 1.3 CPU-seconds: inside one 100-ms budget of 16 CPUs), a process that works
    continuously must not."""
    from svim_asm_amd import bamio
    # (one and a half times the CPUs: a reader's threads also wait — for pages, for the device's share of the inflate work)
    cpus = bamio.process_cpus() if cpus is None else cpus
    return max(2, int(round(1.5 * cpus / float(max(1, workers * n_bams)))))


def run_group(mode, group, genome, get_ctx, first_no, n_total, workers=1, reader_threads=None):
    """One group of samples from the BAMs to the VCFs on the calling thread's device context (`get_ctx()`: asked for
    behind the record walks, which do not need it — a fresh process's first groups walk their BAMs while the HIP runtime
    comes up): (opts, working dir, BAM paths) per sample.  Returns 0, or 1 after logging why an input was refused (as the
    command does)."""
    from svim_asm_amd import bamio
    from svim_asm_amd.SVIM_COMBINE import pair_tables
    n_bams = 2 if mode == "diploid" else 1
    files = []
    _timeline.mark("group starts", sample=first_no)
    for o, wd, bams in group:
        os.makedirs(wd, exist_ok=True)
        # the files of a sample side by side, each reader with its share of the host's threads among the `workers` groups in
        # flight.  The device's share of the inflate work (the one-shot command opens its files without one: cli._open_file):
        # here the process's wall-clock is its CPU-seconds over the CPUs it may use and nobody waits for ONE sample, so
        # the device takes the WHOLE sequence-slice call of every reader (unless SVX_BAM_DEVICE_INFLATE says otherwise) and a
        # call that finds both of the device's inflate lanes taken sleeps for one instead of spending the CPU seconds
        opened = [cli._open_ahead(path, o, one_shot=False, reader_threads=reader_threads or default_reader_threads(workers, n_bams))
                  for path in bams]
        for k, path in enumerate(bams):
            f = cli._open(path, ("first", "second")[k] if n_bams == 2 else "", o, opened=opened[k])
            if f is None:
                return 1
            if bamio.env_device_inflate_percent() is None:
                f.device_inflate_percent = COHORT_DEVICE_INFLATE_PERCENT
            f.device_inflate_wait_ms = COHORT_DEVICE_INFLATE_WAIT_MS
            files.append(f)
    _timeline.mark("files open", sample=first_no)
    SVIM_COLLECT._load_together(files)  # (collect_tables would do it: here, in front of the first use of the context)
    ctx = get_ctx()
    tables = SVIM_COLLECT.collect_tables(files, group[0][0], ctx=ctx)
    _timeline.mark("COLLECT done", sample=first_no)
    for k, (o, wd, bams) in enumerate(group):
        try:  # (write_final_vcf closes its FastaFile, SVIM_COMBINE.py:466-467: one per sample)
            reference = FastaFile(genome, device=getattr(o, "device", 0) or 0)
        except MissingGziError:
            logging.error("The given reference genome is bgzip-compressed and is missing its index file ({0}.gzi). Sequence "
                          "alleles cannot be retrieved.".format(genome))
            return 1
        except BgzfFormatError as e:
            logging.error("The given reference genome cannot be read ({0}). Sequence alleles cannot be retrieved.".format(e))
            return 1
        mine, mine_files = tables[k * n_bams:(k + 1) * n_bams], files[k * n_bams:(k + 1) * n_bams]
        candidates = pair_tables(mine[0], mine[1], reference, mine_files[0], o, ctx=ctx) if mode == "diploid" else mine[0]
        # as cli._run_steps: a damaged BGZF member among the inserted-sequence bytes must fail the run before a VCF is
        # written, also when nobody reads them (--symbolic_alleles)
        _ = candidates.seqs, [t.seqs for t in mine]
        _timeline.mark("PAIR done", sample=first_no + k)
        write_vcf_table(candidates, cli.__version__, mine_files[0].references, mine_files[0].lengths,
                        [entry.strip() for entry in o.types.split(",")], reference, o, ctx=ctx)
        if getattr(o, "keep_candidates", False):
            from svim_asm_amd import SVIM_MERGE
            SVIM_MERGE.keep_candidates(candidates, wd)
        if getattr(o, "keep_coverage", False):
            from svim_asm_amd import SVIM_MERGE
            SVIM_MERGE.keep_coverage(mine_files[0].references, mine_files[0].lengths, [t.coverage for t in mine], wd)
        if getattr(o, "callable_bed", False):
            from svim_asm_amd import SVIM_CALLABLE
            SVIM_CALLABLE.write_sample_bed(mine_files[0].references, [t.coverage for t in mine], o, wd, ctx=ctx)
        _timeline.mark("VCF written", sample=first_no + k)
        logging.info("sample %d of %d: %s/variants.vcf%s", first_no + k + 1, n_total, wd, ".gz" if getattr(o, "bgzip_output", False) else "")
    for f in files:
        f.close()
    del tables, files
    _timeline.mark("files closed", sample=first_no)
    gc.collect()  # (the collector is off while the workers run — the command's 10-15 % —: what a group leaves in cycles goes here)
    return 0


MAX_NODE_PROCESSES = 16  # (children with the GPU open at the same time; the parent is not one of them)


def deal(samples, n):
    """Sample i to child i mod n: the shares in child order, the empty ones of a short manifest included."""
    return [samples[k::n] for k in range(n)]


def _entry_script():
    """The script the children run: the one this process was started as, else bin/svim-asm-cohort beside the package."""
    if os.path.basename(sys.argv[0]) == "svim-asm-cohort" and os.path.isfile(sys.argv[0]):
        return os.path.abspath(sys.argv[0])
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "svim-asm-cohort")


def _child_command(mode, share, genome, device, rest):
    """argv of one child: today's single-process command on its share of the manifest (the seam a test replaces)."""
    return [sys.executable, _entry_script(), mode, share, genome, "--device", str(device)] + list(rest)


def _take_merge(rest):
    """(rest with --keep_candidates once and without --merge, OUT_DIR or None)."""
    rest, out_dir = _take_option(rest, "--merge", None, convert=str)
    if out_dir is not None and "--keep_candidates" not in rest:
        rest = list(rest) + ["--keep_candidates"]
    return rest, out_dir


def _take_genotype(rest):
    """(rest without --genotype_non_carriers / --genotype_margin and, where the first was given, with --keep_coverage
    once; the two as arguments of svim-asm-merge)."""
    try:
        rest, margin = _take_option(rest, "--genotype_margin", None)
    except ValueError:
        raise ValueError("--genotype_margin takes a number of bases")
    wanted = "--genotype_non_carriers" in rest
    rest = [a for a in rest if a != "--genotype_non_carriers"]
    if wanted and "--keep_coverage" not in rest:
        rest = rest + ["--keep_coverage"]
    extra = (["--genotype_non_carriers"] if wanted else []) + (["--genotype_margin", str(margin)] if margin is not None else [])
    return rest, extra


def _take_callable(rest, merging):
    """--callable_bed and --callable_min_length stay in `rest`: every sample writes its callable.bed.  With a merge and the
    first of them, (rest with --keep_coverage once, the two as arguments of svim-asm-merge); else (rest, [])."""
    rest = list(rest)
    if not merging or "--callable_bed" not in rest:
        return rest, []
    try:
        _, min_length = _take_option(rest, "--callable_min_length", None)
    except ValueError:
        raise ValueError("--callable_min_length takes a number of bases")
    if "--keep_coverage" not in rest:
        rest = rest + ["--keep_coverage"]
    return rest, ["--callable_bed"] + (["--callable_min_length", str(min_length)] if min_length is not None else [])


def _merge_command(mode, out_dir, genome, sample_dirs, device, rest, extra=()):
    """argv of the merge child of `--gpus N --merge OUT_DIR`: svim-asm-merge with the options of `rest` it shares with
    the samples' command (a seam like _child_command) and `extra`, its own (_take_genotype)."""
    for name in ("--cohort_workers", "--cohort_group", "--cohort_threads", "--cohort_lanes"):  # (this command's own)
        rest, _ = _take_option(rest, name, 0)
    o = parse_arguments(cli.__version__, [mode, out_dir] + ["-"] * (2 if mode == "diploid" else 1) + [genome] + list(rest))
    script = os.path.join(os.path.dirname(_entry_script()), "svim-asm-merge")
    return [sys.executable, script, out_dir, genome] + list(sample_dirs) + ["--device", str(device)] + _merge_options(o) + list(extra)


def _merge_options(o):
    """The options svim-asm-merge shares with the samples' command, as its argument list."""
    if getattr(o, "query_names", False):
        logging.info("MERGE: --query_names is ignored, read names are not carried into the merged file")
    out = ["--types", o.types]
    for name in ("partition_max_distance", "max_edit_distance"):
        if getattr(o, name, None) is not None:
            out += ["--" + name, str(getattr(o, name))]
    for flag in ("symbolic_alleles", "tandem_duplications_as_insertions", "interspersed_duplications_as_insertions", "bgzip_output",
                 "verbose"):
        if getattr(o, flag, False):
            out.append("--" + flag)
    return out


def _names_device(rest):
    """Does the argument list give --device (in any spelling the reference's parser accepts)?"""
    import argparse
    sniff = argparse.ArgumentParser(add_help=False)
    sniff.add_argument("--device", default=None)
    try:
        return sniff.parse_known_args(list(rest))[0].device is not None
    except (SystemExit, Exception):  # noqa: BLE001 — `--device` without a value: named all the same
        return True


def _launch_plan(rest):
    """(rest without --gpus / --devices, the device of each child) — or a message why the request is refused."""
    try:
        rest, gpus = _take_option(rest, "--gpus", None)
        rest, devices = _take_option(rest, "--devices", None, convert=lambda v: [int(d) for d in v.split(",")])
    except ValueError:
        return None, "--gpus takes a number and --devices a comma-separated list of device indices"
    if any(a in ("--gpus", "--devices") for a in rest):
        return None, "--gpus and --devices each take a value"
    if gpus is None:
        return None, "--devices needs --gpus N"
    if not 1 <= gpus <= MAX_NODE_PROCESSES:
        return None, "--gpus %d: one child per device, 1 to %d of them" % (gpus, MAX_NODE_PROCESSES)
    devices = list(range(gpus)) if devices is None else devices
    if len(devices) != gpus or min(devices) < 0:
        return None, "--devices names %d device(s) (none below 0) for --gpus %d" % (len(devices), gpus)
    if _names_device(rest):
        return None, "--device cannot be given together with --gpus: the parent gives each child its device (--devices)"
    return rest, devices


def launch(mode, manifest, genome, rest):
    """`--gpus N`: the manifest dealt out to one fresh child process per device under one CPU budget (the module's
    docstring).  This process creates no device context and does not load the library."""
    import shutil
    import signal
    import subprocess
    import tempfile
    import threading
    import time
    rest, devices = _launch_plan(rest)
    if rest is None:
        print("svim-asm-cohort: " + devices, file=sys.stderr)
        return 2
    rest, merge_dir = _take_merge(rest)  # (the children keep their tables; the merge is one more child, below)
    try:
        rest, genotype = _take_genotype(rest)
        if genotype and merge_dir is None:
            raise ValueError("--genotype_non_carriers and --genotype_margin are options of the merge: give --merge OUT_DIR")
        rest, callable_bed = _take_callable(rest, merge_dir is not None)
        genotype = genotype + callable_bed  # (the merge's own options, one list)
    except ValueError as e:
        print("svim-asm-cohort: %s" % e, file=sys.stderr)
        return 2
    samples = read_manifest(manifest, 2 if mode == "diploid" else 1)  # (a malformed manifest fails here, before any child exists)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)-7.7s]  %(message)s")
    shares = [(devices[k], share) for k, share in enumerate(deal(samples, len(devices))) if share]
    env = dict(os.environ, SVX_NODE_PROCESSES=str(len(shares)))
    tmp = tempfile.mkdtemp(prefix="svx-cohort-")
    procs, caught = [], []

    def stop_children(signo=None, frame=None):
        if signo is not None:
            caught.append(signo)
        for p in procs:
            if p.poll() is None:
                p.send_signal(signal.SIGTERM)

    handled = (signal.SIGINT, signal.SIGTERM) if threading.current_thread() is threading.main_thread() else ()
    before = {s: signal.signal(s, stop_children) for s in handled}

    def wait_for_children():
        deadline = None
        while any(p.poll() is None for p in procs):
            if caught and deadline is None:
                deadline = time.monotonic() + 10.0
            if deadline is not None and time.monotonic() > deadline:
                for p in procs:  # (a child that does not answer SIGTERM: nothing may outlive the parent)
                    if p.poll() is None:
                        p.kill()
            time.sleep(0.02)

    merge_proc = None
    try:
        for k, (device, share) in enumerate(shares):
            if caught:
                break
            path = os.path.join(tmp, "share_%d_of_%d.txt" % (k, len(shares)))
            with open(path, "w") as f:
                f.write("".join("%s %s\n" % (wd, " ".join(bams)) for wd, bams in share))
            procs.append(subprocess.Popen(_child_command(mode, path, genome, device, rest), env=env))
            if caught:  # (a signal that arrived while this child was being started has not reached it)
                stop_children()
        wait_for_children()
        if merge_dir is not None and not caught:
            if len(procs) == len(shares) and all(p.returncode == 0 for p in procs):
                # one more fresh child, alone on the first listed device: this process still never touches the GPU
                merge_proc = subprocess.Popen(_merge_command(mode, merge_dir, genome, [wd for wd, _ in samples], devices[0], rest, genotype),
                                              env=dict(os.environ, SVX_NODE_PROCESSES="1"))
                procs.append(merge_proc)
                wait_for_children()
            else:
                logging.info("MERGE: not attempted, a sample failed")
    finally:
        for p in procs:
            if p.poll() is None:  # (an exception on the way: the same promise)
                p.kill()
            p.wait()
        for s, handler in before.items():
            signal.signal(s, handler)
        shutil.rmtree(tmp, ignore_errors=True)
    worst = 0
    for p, (device, share) in zip(procs, shares):
        rc = p.returncode
        logging.info("CHILD: device %d, %d sample(s), %s", device, len(share),
                     "status %d" % rc if rc >= 0 else "killed by signal %d" % -rc)
        worst = max(worst, rc if rc >= 0 else 128 - rc)
    if merge_proc is not None:
        rc = merge_proc.returncode
        logging.info("MERGE: device %d, %d sample(s), %s", devices[0], len(samples),
                     "status %d" % rc if rc >= 0 else "killed by signal %d" % -rc)
        worst = max(worst, rc if rc >= 0 else 128 - rc)
    if caught:
        return 128 + int(caught[0])
    return worst


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) < 3 or argv[0] not in ("haploid", "diploid"):
        print(__doc__)
        return 2
    mode, manifest, genome, rest = argv[0], argv[1], argv[2], argv[3:]
    n_bams = 2 if mode == "diploid" else 1
    if shard.world()[1] > 1:
        # one process = one cohort: under a launcher every rank would collect everything and write the same files
        print("svim-asm-cohort runs as ONE process (WORLD_SIZE=%d): start one cohort per GPU with --device, or shard a "
              "single sample with `svim-asm` under the launcher" % shard.world()[1], file=sys.stderr)
        return 2
    if any(a in ("--gpus", "--devices") or a.startswith(("--gpus=", "--devices=")) for a in rest):
        return launch(mode, manifest, genome, rest)  # (the parent of one child per device: never touches the GPU itself)
    rest, workers = _take_option(rest, "--cohort_workers", 0)
    rest, per_group = _take_option(rest, "--cohort_group", 1)
    rest, reader_threads = _take_option(rest, "--cohort_threads", 0)
    rest, lanes = _take_option(rest, "--cohort_lanes", 0)
    rest, merge_dir = _take_merge(rest)
    try:
        rest, genotype = _take_genotype(rest)
        if genotype and merge_dir is None:
            raise ValueError("--genotype_non_carriers and --genotype_margin are options of the merge: give --merge OUT_DIR")
        rest, callable_bed = _take_callable(rest, merge_dir is not None)
        genotype = genotype + callable_bed  # (the merge's own options, one list)
    except ValueError as e:
        print("svim-asm-cohort: %s" % e, file=sys.stderr)
        return 2
    samples = read_manifest(manifest, n_bams)
    _timeline.mark("cohort main")
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)-7.7s]  %(message)s")
    # the CPUs this process plans with — ONCE, here: the workers narrow the affinity mask to the device's NUMA node
    # (bind_to_device_node), and a budget read behind that would divide the narrowed mask among the siblings again
    from svim_asm_amd import bamio
    cpus = bamio.process_cpus()
    # one options object per sample through the reference's own parser (working dir and BAM paths differ)
    opts = [parse_arguments(cli.__version__, [mode, wd] + bams + [genome] + rest) for wd, bams in samples]
    device = getattr(opts[0], "device", 0) or 0
    cli._warm_device(device)
    per_group = len(samples) if per_group <= 0 else per_group
    groups = [[(opts[k], samples[k][0], samples[k][1]) for k in range(g, min(g + per_group, len(samples)))]
              for g in range(0, len(samples), per_group)]
    workers = max(1, min(workers or default_workers(cpus), len(groups)))
    reader_threads = reader_threads or default_reader_threads(workers, n_bams, cpus)
    logging.info("****************** %d samples, %d BAM files: %d group(s) of up to %d, %d worker(s) ******************",
                 len(samples), len(samples) * n_bams, len(groups), per_group, workers)
    if bamio.env_node_processes() is not None:  # (one of a node's cohort processes: what it planned with, once)
        logging.info("BUDGET: %.2f CPUs for this process (%d cohort process(es) on the node): %d worker(s), %d thread(s) per "
                     "reader", cpus, bamio.env_node_processes(), workers, reader_threads)
    import threading
    from svim_asm_amd import _lib
    # inflate lanes of the device (svx_bam_set_inflate_lanes, before the first load): one per reader the workers keep in
    # flight — with the walks' check on the device leg the workers waited for the default's two lanes, not for CPUs
    lanes = max(1, min(16, lanes or int(os.environ.get("SVX_COHORT_LANES") or 0) or default_lanes(workers, n_bams)))
    _lib.load().svx_bam_set_inflate_lanes(lanes)
    gc.collect()
    gc.freeze()
    gc.disable()  # as the command does for its one sample; every worker collects once per group (run_group)
    lock, state = threading.Lock(), {"next": 0, "rc": 0, "error": None}

    def work(worker_no):
        try:
            box = {}

            def get_ctx():
                # worker 0 on the process's context (the one _warm_device is bringing up), the others on their own
                if "ctx" not in box:
                    box["ctx"] = _lib.default_context(device) if worker_no == 0 else _lib.new_context(device)
                    bound = bind_to_device_node(device)  # (behind the context: the device's address needs the runtime up)
                    if worker_no == 0:
                        logging.info("AFFINITY: %s", bound)
                return box["ctx"]
            while True:
                with lock:
                    g = state["next"]
                    if g >= len(groups) or state["rc"] or state["error"]:
                        return
                    state["next"] = g + 1
                rc = run_group(mode, groups[g], genome, get_ctx, g * per_group, len(samples), workers, reader_threads)
                if rc:
                    with lock:
                        state["rc"] = rc
                    return
        except BaseException as e:  # noqa: BLE001 — re-raised on the main thread
            with lock:
                state["error"] = state["error"] or e

    threads = [threading.Thread(target=work, args=(k,), name="cohort-%d" % k) for k in range(workers)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    gc.enable()
    _timeline.mark("workers done")
    _timeline.dump()
    if state["error"] is not None:
        raise state["error"]
    if merge_dir is not None:
        if state["rc"]:
            logging.info("MERGE: not attempted, a sample failed")
        else:
            # the workers have joined and every sample returned 0: here, on the process's default context
            from svim_asm_amd import merge_cli
            return merge_cli.main([merge_dir, genome] + [wd for wd, _ in samples] + ["--device", str(device)] + _merge_options(opts[0]) + genotype)
    return state["rc"]


def entry():
    sys.exit(main())
