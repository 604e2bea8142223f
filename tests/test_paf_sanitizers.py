"""The native PAF reader (csrc/svx_paf.cpp behind include/svx_paf.h, with the CIGAR path it shares with csrc/svx_sam.cpp
and the oriented fetch of csrc/svx_text.cpp) under AddressSanitizer + UBSan and, in a second build, ThreadSanitizer on the
CPU: every entry point on the config-1 records and a synthetic sample rendered as shuffled PAFs (LF and CRLF) with their
query assemblies, then on hundreds of damaged copies.  A damaged file may be refused or read as what it now says; any
out-of-bounds access, use after free, signed overflow, leak or data race fails the test.  (Host code only.)"""
import os
import shutil
import subprocess

import pytest

from tests import paf_writer as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", params=["address,undefined", "thread"])
def driver(request, tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("g++ or the HIP headers are not here")
    exe = str(tmp_path_factory.mktemp("san") / "paf_sanitize")
    csrc = os.path.join(ROOT, "svim_asm_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=" + request.param, "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "native", "paf_sanitize.cpp"), os.path.join(csrc, "svx_paf.cpp"),
           os.path.join(csrc, "svx_sam.cpp"), os.path.join(csrc, "svx_textaln.cpp"), os.path.join(csrc, "svx_text.cpp"), "-L/opt/rocm/lib", "-lamdhip64", "-lpthread",
           "-ldl", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        pytest.skip("sanitizer build not possible here:\n" + res.stdout[-2000:])
    return exe


def _run(exe, scratch, mutations, ref_fai, pairs):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    args = [x for fa, paf in pairs for x in (fa, paf)]
    res = subprocess.run([exe, str(scratch), str(mutations), ref_fai] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, env=env, timeout=900)
    assert res.returncode == 0 and "paf_sanitize ok" in res.stdout and "WARNING: ThreadSanitizer" not in res.stdout, \
        res.stdout[-4000:]
    return res.stdout


def test_reader_is_clean_on_config1_and_its_damaged_copies(driver, tmp_path):
    g = os.path.join(GOLD, "config1")
    pairs = []
    for k in range(2):
        paf, fa = pw.bam_as_paf(os.path.join(g, "hap%d.bam" % (k + 1)), str(tmp_path / ("h%d.paf" % k)), str(tmp_path / ("q%d.fa" % k)),
                                shuffle_seed=k, eol="\n" if k == 0 else "\r\n", line=60 if k == 0 else 0)
        pairs.append((fa, paf))
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    out = _run(driver, scratch, 150, os.path.join(g, "ref.fa.fai"), pairs)
    assert " read," in out


def test_reader_is_clean_on_a_synthetic_sample_with_splits(driver, tmp_path):
    from svim_asm_amd import synth_bam
    contigs = (("chrA", 200000), ("chrB", 120000), ("chrC", 70000))
    ref, bams = synth_bam.write_dataset(str(tmp_path), seed=4, contigs=contigs, n_shared=6, n_private=2, median_aln=30000, mean_m=60)
    pairs = [pw.bam_as_paf(b, b[:-4] + ".paf", b[:-4] + ".q.fa", shuffle_seed=k)[::-1] for k, b in enumerate(bams)]
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    out = _run(driver, scratch, 80, ref + ".fai", pairs)
    assert " read," in out
