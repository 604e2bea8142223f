"""The host path of bgzip-compressed genomes (csrc/svx_fasta_bgzf.cpp behind svx_fasta_open_bgzf, with csrc/svx_text.cpp
and the BGZF member layer of csrc/svx_bgzf.cpp) under AddressSanitizer + UBSan and, as a second build, ThreadSanitizer: random
genomes bgzipped at random member sizes and levels, windows fetched by several caller threads on one handle, then
damaged copies (flipped bytes, truncations, damaged .gzi columns).  Any out-of-bounds access, use after free, signed
overflow, data race or leak fails the test, and so does a successful fetch whose bases differ from the text."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svim_asm_amd", "csrc")


@pytest.fixture(scope="module", params=["address,undefined", "thread"])
def driver(request, tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("g++ or the HIP headers are not here")
    exe = str(tmp_path_factory.mktemp("san") / "fasta_bgzf_sanitize")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=" + request.param, "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "native", "fasta_bgzf_sanitize.cpp"), os.path.join(CSRC, "svx_text.cpp"),
           os.path.join(CSRC, "svx_fasta_bgzf.cpp"), os.path.join(CSRC, "svx_bgzf.cpp"), "-L/opt/rocm/lib", "-lamdhip64",
           "-lz", "-lpthread", "-ldl", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        pytest.skip("sanitizer build not possible here:\n" + res.stdout[-2000:])
    return exe


def test_bgzf_host_path_is_clean_on_random_and_damaged_inputs(driver, tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([driver, str(tmp_path), "60"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                         timeout=900)
    assert res.returncode == 0 and "fasta_bgzf_sanitize ok" in res.stdout and "WARNING: ThreadSanitizer" not in res.stdout, \
        res.stdout[-4000:]
    assert " 0 wrong" in res.stdout and " opens refused" in res.stdout
