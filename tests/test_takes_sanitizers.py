"""The scratch list of the host entry points (csrc/svx_takes.h) under AddressSanitizer + UBSan: tests/native/takes_sanitize.cpp
holds it to the arithmetic it replaces, restated in plain loops — every pointer of place(), the final `used`, bytes() —
for element sizes of 1 to 24 bytes, counts of 0, 1, 255, 256 and 257 (2^32 + 1 measured only), starting offsets of 0, 4096
and one that is no multiple of 256; the empty list, null slots, a list extended by a callee, uploads without a source or
without elements; and fills a malloc of exactly bytes() slot by slot.  Any out-of-bounds access or overflow fails the test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ is not here")
    exe = str(tmp_path_factory.mktemp("san") / "takes_sanitize")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "svim_asm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "takes_sanitize.cpp"), "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        pytest.skip("sanitizer build not possible here:\n" + res.stdout[-2000:])
    return exe


def test_the_list_places_what_the_takes_placed_and_stays_inside_its_bytes(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([driver], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert res.returncode == 0 and "takes_sanitize ok: 35 lists placed and filled" in res.stdout, res.stdout[-4000:]
