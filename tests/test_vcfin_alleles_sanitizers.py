"""The VCF reader's list of edits (svx_vcfin_open_alleles / svx_vcfin_get_alleles: csrc/svx_vcfin.cpp behind
include/svx_vcfin.h, compiled with csrc/svx_sam.cpp, the line scanner csrc/svx_textaln.cpp and the BGZF member layer
csrc/svx_bgzf.cpp) under AddressSanitizer + UBSan and, in a second build, ThreadSanitizer on the CPU: a stand-alone
driver (tests/native/vcfin_alleles_sanitize.cpp, its own main; nothing is loaded into Python and nothing is preloaded)
reads the valid files — plain, "\\r\\n", BGZF in one member, in two, in many and in members that split every record's
line —, then a small file truncated at every byte, then seeded byte flips of all of them.  A damaged file may be refused
or read as what it now says; any out-of-bounds access, use after free, signed overflow, leak or data race fails the
test.  (Host code only.)"""
import os
import shutil
import subprocess

import pytest

from tests import test_vcfin as V
from tests import test_vcfin_alleles as VA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "config1")


@pytest.fixture(scope="module", params=["address,undefined", "thread"])
def driver(request, tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("g++ or the HIP headers are not here")
    tmp = tmp_path_factory.mktemp("san")
    exe = str(tmp / "vcfin_alleles_sanitize")
    # the tool itself (the compiler's sanitizer runtime, the HIP library to link against): missing -> skip; anything that
    # goes wrong after that is a build error of the reader or the driver and fails
    (tmp / "probe.cpp").write_text("#include <hip/hip_runtime_api.h>\nint main() { int n = 0; (void)hipGetDeviceCount(&n); return 0; }\n")
    probe = subprocess.run([gxx, "-std=c++17", "-fsanitize=" + request.param, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            str(tmp / "probe.cpp"), "-L/opt/rocm/lib", "-lamdhip64", "-lz", "-lpthread", "-ldl", "-o", str(tmp / "probe")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer build possible here (-fsanitize=%s):\n%s" % (request.param, probe.stdout[-1500:]))
    csrc = os.path.join(ROOT, "svim_asm_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=" + request.param, "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "native", "vcfin_alleles_sanitize.cpp"), os.path.join(csrc, "svx_vcfin.cpp"),
           os.path.join(csrc, "svx_sam.cpp"), os.path.join(csrc, "svx_textaln.cpp"), os.path.join(csrc, "svx_bgzf.cpp"),
           "-L/opt/rocm/lib", "-lamdhip64", "-lz", "-lpthread", "-ldl", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, "the reader or its driver does not build:\n" + res.stdout[-4000:]
    return exe


def test_reader_is_clean_on_valid_truncated_and_damaged_files(driver, tmp_path):
    small = V.write(tmp_path, VA.BODY, name="small.vcf")
    crlf = V.write(tmp_path, VA.BODY, name="crlf.vcf", eol="\r\n")
    golden = os.path.join(GOLD, "diploid_default.vcf")
    files = [small, crlf, golden, V.bgzip(small, str(tmp_path / "one.vcf.gz"), 0xFF00), V.bgzip(golden, str(tmp_path / "two.vcf.gz"), 0xFF00),
             V.bgzip(small, str(tmp_path / "split.vcf.gz"), 23), V.bgzip(golden, str(tmp_path / "many.vcf.gz"), 1500)]
    assert len(V.data_members(files[3])) == 1 and len(V.data_members(files[4])) == 2
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([driver, str(scratch), "120", os.path.join(GOLD, "ref.fa.fai")] + files, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, env=env, timeout=900)
    assert res.returncode == 0 and "vcfin_alleles_sanitize ok" in res.stdout and "WARNING: ThreadSanitizer" not in res.stdout, res.stdout[-4000:]
    assert " read," in res.stdout
