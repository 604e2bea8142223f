"""The native SAM reader and the host CIGAR-text parser (csrc/svx_sam.cpp behind include/svx_sam.h) under
AddressSanitizer + UBSan and, in a second build, ThreadSanitizer on the CPU: every entry point on the config-1 records
and a synthetic sample rendered as shuffled SAMs (LF and CRLF), then on hundreds of damaged copies, and the batch parser
on random texts.  A damaged file may be refused or read as what it now says; any out-of-bounds access, use after free,
signed overflow, leak or data race fails the test.  (Host code only: the kernels are not in this build.)"""
import os
import shutil
import subprocess

import pytest

from tests import sam_text_writer as stw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", params=["address,undefined", "thread"])
def driver(request, tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("g++ or the HIP headers are not here")
    exe = str(tmp_path_factory.mktemp("san") / "sam_sanitize")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=" + request.param, "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "svim_asm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "sam_sanitize.cpp"),
           os.path.join(ROOT, "svim_asm_amd", "csrc", "svx_sam.cpp"), os.path.join(ROOT, "svim_asm_amd", "csrc", "svx_textaln.cpp"), "-L/opt/rocm/lib", "-lamdhip64", "-lpthread",
           "-ldl", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        pytest.skip("sanitizer build not possible here:\n" + res.stdout[-2000:])
    return exe


def _run(exe, scratch, mutations, files):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, str(scratch), str(mutations)] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, env=env, timeout=900)
    assert res.returncode == 0 and "sam_sanitize ok" in res.stdout and "WARNING: ThreadSanitizer" not in res.stdout, \
        res.stdout[-4000:]
    return res.stdout


def test_reader_is_clean_on_config1_and_its_damaged_copies(driver, tmp_path):
    files = [stw.bam_as_sam(os.path.join(GOLD, "config1", "hap%d.bam" % (k + 1)), str(tmp_path / ("h%d.sam" % k)),
                            shuffle_seed=k, eol="\n" if k == 0 else "\r\n") for k in range(2)]
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    out = _run(driver, scratch, 150, files)
    assert " read," in out


def test_reader_is_clean_on_a_synthetic_sample_with_splits_and_hand_written_lines(driver, tmp_path):
    from svim_asm_amd import synth_bam
    contigs = (("chrA", 200000), ("chrB", 120000), ("chrC", 70000))
    _, bams = synth_bam.write_dataset(str(tmp_path), seed=4, contigs=contigs, n_shared=6, n_private=2, median_aln=30000, mean_m=60)
    files = [stw.bam_as_sam(b, b[:-4] + ".sam", shuffle_seed=k) for k, b in enumerate(bams)]
    aux = ["XA:A:q", "Xc:i:-128", "XI:i:4294967295", "Xf:f:-1.5", "XZ:Z:hello", "SA:Z:chrB,100,+,5M5S,60,0;", "XH:H:1AE301",
           "Bc:B:c,-1,2", "BS:B:S,65535", "Bf:B:f,0.5,-2.25", "Be:B:C"]
    lines = [stw.record_line("r%d" % k, 16 * (k & 1), ("chrA", "chrB", "*")[k % 3], -1 if k % 3 == 2 else 7 * k, 60,
                             "*" if k % 3 == 2 else "4S6M", "*" if k % 4 == 3 else "acgtnNRYKM", aux[:k]) for k in range(12)]
    files.append(stw.write_sam(str(tmp_path / "hand.sam"), [c[0] for c in contigs], [c[1] for c in contigs], lines, so=None))
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    out = _run(driver, scratch, 80, files)
    assert " read," in out
