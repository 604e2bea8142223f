"""The device BGZF encoder (svx_bgzf_deflate_dev, svim_asm_amd/csrc/svx_deflate.hip) and `--bgzip_output` on the device
path.  Every corpus case must come back exactly through zlib, the build's host decoder (svx_inflate_raw) and its device
decoder (svx_bgzf_inflate_dev), with bgzip's container structure; the bytes must not depend on the call or on how the
blocks are split across launches; the compressed size is compared with zlib level 6 over the same blocks."""
import ctypes as C
import gzip
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from svim_asm_amd import _lib, vcf_bgzf
from tests import tabix_reader
from tests.test_oracle_pins import RUNS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BLOCK = 65280


def corpus():
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    period = lambda p, n: np.tile(rng.integers(0, 256, p).astype(np.uint8), n // p + 1)[:n].tobytes()
    cases = {
        "empty": b"", "one": b"x", "b65279": rng.integers(0, 4, 65279).astype(np.uint8).tobytes(),
        "b65280": acgt[rng.integers(0, 4, 65280)].tobytes(), "b65281": acgt[rng.integers(0, 4, 65281)].tobytes(),
        "zeros": bytes(3 * BLOCK + 77), "period32768": period(32768, 2 * BLOCK), "period32769": period(32769, 2 * BLOCK),
        "random": rng.integers(0, 256, 3 * BLOCK + 5).astype(np.uint8).tobytes(), "acgt": acgt[rng.integers(0, 4, 400_000)].tobytes(),
        "repeat": b"G" * 200_000,
        "several_mb": b"".join(open(os.path.join(GOLD, "config1", n + ".vcf"), "rb").read() for n in sorted(RUNS)) * 12,
    }
    for n in sorted(RUNS):
        cases["vcf_" + n] = open(os.path.join(GOLD, "config1", n + ".vcf"), "rb").read()
    # the members of a test BAM, decompressed
    cases["bam"] = gzip.decompress(open(os.path.join(GOLD, "config1", "hap1.bam"), "rb").read())
    return cases


CORPUS = corpus()


def inflate_host(payload, isize):
    lib = _lib.load()
    out = np.zeros(max(isize, 1) + 64, np.uint8)
    n = C.c_uint64()
    src = np.frombuffer(payload, np.uint8) if payload else np.zeros(1, np.uint8)
    rc = lib.svx_inflate_raw(src.ctypes.data, len(payload), out.ctypes.data, len(out), None, 0, C.byref(n))
    assert rc == 0
    return out[:n.value].tobytes()


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_corpus_round_trips(svx_ctx, name):
    data = CORPUS[name]
    blob, sizes = svx_ctx.bgzf_deflate(data)
    if not data:
        assert blob == tabix_reader.EOF_MEMBER and len(sizes) == 0
        return
    assert tabix_reader.check_bgzf(blob, data) == list(sizes)  # zlib, structure, CRC, ISIZE, EOF member
    ms = tabix_reader.members(blob)[:-1]
    assert all(m[1] <= 65536 for m in ms)
    assert b"".join(inflate_host(m[2], m[4]) for m in ms) == data
    st, outs, _ = svx_ctx.bgzf_inflate([m[2] for m in ms], [m[4] for m in ms], [m[3] for m in ms])
    assert st.tolist() == [0] * len(ms) and b"".join(outs) == data
    if name == "random":
        assert all(m[2][0] & 7 == 1 for m in ms)  # stored blocks
    assert len(blob) <= len(data) + 28 + 31 * len(ms)  # never more than stored blocks
    # deterministic: a second call, and the blocks split across launches and calls
    assert svx_ctx.bgzf_deflate(data)[0] == blob
    lib = _lib.load()
    was = lib.svx_bgzf_deflate_set_slice(2)
    try:
        assert svx_ctx.bgzf_deflate(data)[0] == blob
    finally:
        lib.svx_bgzf_deflate_set_slice(was)
    cut = BLOCK * max(1, len(ms) // 2)
    if cut < len(data):
        a, b = svx_ctx.bgzf_deflate(data[:cut])[0], svx_ctx.bgzf_deflate(data[cut:])[0]
        assert a[:-28] + b == blob


def zlib6_size(data):
    total = 0
    for k in range(0, len(data), BLOCK):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        total += 26 + len(c.compress(data[k:k + BLOCK]) + c.flush())
    return total


@pytest.mark.parametrize("name", ["vcf_diploid_default", "several_mb"])
def test_compression_within_15_percent_of_zlib6(svx_ctx, name):
    data = CORPUS[name]
    blob, _ = svx_ctx.bgzf_deflate(data)
    ratio = (len(blob) - 28) / zlib6_size(data)
    print("device / zlib-6 size on %s: %.3f" % (name, ratio))
    assert ratio <= 1.15


@pytest.mark.parametrize("name", sorted(RUNS))
def test_cli_device_path_matches_the_goldens(tmp_path, monkeypatch, name):
    from svim_asm_amd import cli
    monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", "1")
    argv = list(RUNS[name])
    argv[1] = str(tmp_path)
    argv = [os.path.join(GOLD, "config1", a) if a.endswith((".bam", ".fa")) else a for a in argv]
    cli.main(argv + ["--bgzip_output"])
    blob = open(tmp_path / "variants.vcf.gz", "rb").read()
    text = gzip.decompress(blob)
    got = b"".join(l for l in text.splitlines(keepends=True) if not l.startswith(b"##fileDate="))
    assert got == open(os.path.join(GOLD, "config1", name + ".vcf"), "rb").read()
    tabix_reader.check_bgzf(blob, text)
    assert not os.path.exists(tmp_path / "variants.vcf")
    r = tabix_reader.Reader(blob, open(tmp_path / "variants.vcf.gz.tbi", "rb").read())
    for nm in r.index.names:
        nm = nm.decode()
        assert r.query(nm, 0, 1 << 31) == tabix_reader.brute(text, nm, 0, 1 << 31)


def test_cohort_device_path(tmp_path, monkeypatch):
    from svim_asm_amd import cohort
    monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", "1")
    g = os.path.join(GOLD, "config1")
    rows = [("s%d" % k, "hap1.bam", "hap2.bam") for k in range(3)]
    manifest = tmp_path / "cohort.tsv"
    manifest.write_text("".join("%s %s %s\n" % (tmp_path / wd, os.path.join(g, a), os.path.join(g, b)) for wd, a, b in rows))
    assert cohort.main(["diploid", str(manifest), os.path.join(g, "ref.fa"), "--bgzip_output", "--cohort_workers", "2"]) == 0
    for wd, _, _ in rows:
        text = gzip.decompress(open(tmp_path / wd / "variants.vcf.gz", "rb").read())
        got = b"".join(l for l in text.splitlines(keepends=True) if not l.startswith(b"##fileDate="))
        assert got == open(os.path.join(g, "diploid_default.vcf"), "rb").read()
        assert os.path.exists(tmp_path / wd / "variants.vcf.gz.tbi")


@pytest.fixture(scope="module")
def full_dataset(tmp_path_factory):
    from tests.test_full_golden import full_dataset as make
    return make.__wrapped__(tmp_path_factory)


def test_full_size_device_and_host_paths(full_dataset, tmp_path, monkeypatch):
    """The full-size sample: the device path's .vcf.gz decompresses to the committed digest, the host path's to the same
    text, and the index answers random regions exactly."""
    from svim_asm_amd import cli
    from tests.test_full_golden import META
    fasta, bams = full_dataset
    texts = {}
    for dev in ("1", "0"):
        monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", dev)
        wd = tmp_path / ("dev" + dev)
        cli.main(["diploid", str(wd), bams[0], bams[1], fasta, "--bgzip_output"])
        blob = open(wd / "variants.vcf.gz", "rb").read()
        texts[dev] = gzip.decompress(blob)
        if dev == "1":
            tabix_reader.check_bgzf(blob, texts[dev])
            reader = tabix_reader.Reader(blob, open(wd / "variants.vcf.gz.tbi", "rb").read())
    masked = b"".join(l for l in texts["1"].splitlines(keepends=True) if not l.startswith(b"##fileDate="))
    assert len(masked) == META["vcf_bytes"] and hashlib.sha256(masked).hexdigest() == META["vcf_sha256"]
    body = [l for l in masked.decode().split("\n") if l and l[0] != "#"]
    assert [l[:200] for l in body[:3]] == META["first_records"] and [l[:200] for l in body[-3:]] == META["last_records"]
    assert [l for l in texts["0"].split(b"\n") if not l.startswith(b"##fileDate=")] == \
        [l for l in texts["1"].split(b"\n") if not l.startswith(b"##fileDate=")]
    from tests.test_vcf_bgzf import random_regions
    random_regions(texts["1"], reader, seed=5, n=500)
