"""The device DEFLATE encoder's Huffman routines on the CPU (svim_asm_amd/csrc/svx_deflate_huff.h, the text
svx_deflate.hip's kernel runs on one lane): tests/native/deflate_huff.cpp compiles them for the host with AddressSanitizer
+ UBSan and gives build_lengths frequency vectors whose optimal tree is deeper than the limit — Fibonacci runs, permuted
and tied, geometric, one huge symbol over singletons, seeded random — for the three alphabets (286 / 15 bits, 30 / 15,
19 / 7), against plain Huffman and package-merge written in the program.  No GPU, nothing loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ is not here")
    exe = str(tmp_path_factory.mktemp("san") / "deflate_huff")
    cmd = [gxx, "-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "svim_asm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "deflate_huff.cpp"), "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        pytest.skip("sanitizer build not possible here:\n" + res.stdout[-2000:])
    return exe


def test_lengths_codes_and_runs_against_the_references(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([driver, "3000", "1"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
    print(res.stdout[-3000:])
    assert res.returncode == 0 and "deflate_huff ok" in res.stdout, res.stdout[-4000:]
    # a case that never reaches the limiter hides a failure: every alphabet must have needed it, and must have had
    # optimal trees exactly as deep as the limit (where the limiter must change nothing)
    rows = re.findall(r"^(.+): (\d+) vectors, limiter needed (\d+), optimal depth exactly at the limit (\d+), worst cost / optimum ([0-9.]+)",
                      res.stdout, re.M)
    assert [r[0] for r in rows] == ["literal/length 286/15", "distance 30/15", "code-length 19/7"]
    for name, vectors, limited, at_limit, worst in rows:
        assert int(vectors) > 3000 and int(limited) > 0 and int(at_limit) > 0 and float(worst) >= 1.0, name
    assert re.search(r"^worst cost ratio [0-9.]+$", res.stdout, re.M)
