"""SAM input on the GPU: the CIGAR-text kernels (svx_cigar_text_parse_dev, csrc/svx_cigartext.hip) against the host
parser and the pure-Python oracle of tests/sam_text_writer.py, the SAM reader with a device (pool in HBM, result
independent of SVX_SAM_DEVICE), and shuffled SAMs through the real device pipeline against the committed golden VCFs."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

from tests import sam_text_writer as stw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CHUNK = 1024  # bytes per workgroup of the kernels (kChunk)


def _batch(texts):
    texts = [t.encode("latin-1") if isinstance(t, str) else t for t in texts]
    off = np.zeros(len(texts) + 1, np.uint64)
    if texts:
        np.cumsum([len(t) for t in texts], out=off[1:])
    return b"".join(texts), off


def _same(got, exp, what):
    for k in ("status", "cigar_off", "ref_len", "words"):
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), np.asarray(exp[k], dtype=np.int64)), (what, k)


def check(ctx, texts, what, oracle=True):
    from svim_asm_amd import _lib
    text, off = _batch(texts)
    dev = ctx.cigar_text_parse(text, off)
    host = _lib.cigar_text_parse_host(text, off, threads=4)
    _same(dev, host, what + ": device vs host")
    if oracle:
        _same(host, stw.parse_batch(texts), what + ": host vs oracle")
    return dev


BAD = ["12M*", "12Q3M", "5m", "M", "3M4", "268435456M", "1M\t2M", "12M 3I", "", "3MM", "0000000000268435456D", "**", "1M-2I"]
GOOD = ["1M", "268435455M", "*", "1M1I1D1N1S1H1P1=1X", "0000000012M", "100S20000M3I7D9=1X2N5P40H", "007M"]


def test_every_operator_and_every_rejected_form(svx_ctx):
    out = check(svx_ctx, GOOD + BAD, "forms")
    assert list(out["status"][:len(GOOD)]) == [0] * len(GOOD)
    assert all(s != 0 for s in out["status"][len(GOOD):])
    assert {int(s) for s in out["status"]} == {0, 1, 2, 3, 4, 5}


def test_empty_inputs(svx_ctx):
    out = check(svx_ctx, [], "no records")
    assert len(out["words"]) == 0 and list(out["cigar_off"]) == [0]
    check(svx_ctx, ["*"] * 5, "only stars")
    check(svx_ctx, [""] * 3, "only empty texts")


def test_numbers_and_records_across_every_chunk_boundary(svx_ctx):
    """The start of a fixed group of records is moved over one chunk length + 1: every number, operator and record
    boundary of the group meets the chunk boundary once."""
    group = ["123456789M", "268435455D1I", "*", "77=", "12Q", "5S100000000M9X", "3M4", "1N"]
    for start in range(CHUNK + 2):
        lead = "1M" * (start // 2) + ("7" if start % 2 else "")  # (odd starts: a leading record that ends in a digit)
        texts = ([lead] if lead else []) + group + ["9M"] * 3
        check(svx_ctx, texts, "start %d" % start, oracle=start % 64 == 0 or start >= CHUNK - 2)


def test_one_record_of_three_million_operations(svx_ctx):
    rng = np.random.default_rng(5)
    n = 3_000_000
    lens = rng.integers(1, 30000, n)
    ops = np.frombuffer(b"MIDNSHP=X", np.uint8)[rng.integers(0, 9, n)]
    text = "".join("%d%s" % (l, chr(o)) for l, o in zip(lens.tolist(), ops.tolist()))
    out = check(svx_ctx, ["5M", text, "6I"], "3e6 ops")
    assert len(out["words"]) == n + 2
    code = np.zeros(256, np.uint32)
    code[np.frombuffer(b"MIDNSHP=X", np.uint8)] = np.arange(9, dtype=np.uint32)
    assert np.array_equal(out["words"][1:-1], (lens.astype(np.uint32) << 4) | code[ops])


def test_five_thousand_short_records_with_bad_ones_in_the_middle(svx_ctx):
    rng = np.random.default_rng(6)
    texts = []
    for i in range(5000):
        k = int(rng.integers(1, 6))
        texts.append("".join("%d%s" % (int(rng.integers(1, 5000)), "MIDNSHP=X"[int(rng.integers(0, 9))]) for _ in range(k)))
    good = check(svx_ctx, texts, "5000 good")
    assert not good["status"].any()
    mixed = list(texts)
    for j, i in enumerate(range(100, 4900, 97)):
        mixed[i] = BAD[j % len(BAD)]
    out = check(svx_ctx, mixed, "5000 mixed")
    bad = np.zeros(5000, bool)
    bad[list(range(100, 4900, 97))] = True
    assert (out["status"][bad] != 0).all() and not out["status"][~bad].any()
    # the good neighbours' words are what they were
    n_good = np.diff(good["cigar_off"].astype(np.int64))
    keep = np.repeat(~bad, n_good)
    assert np.array_equal(out["words"], good["words"][keep])
    assert np.array_equal(out["ref_len"][~bad], good["ref_len"][~bad])


# ------------------------------------------------------------------ the reader with a device
def device_words(address, n):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(n, np.uint32)
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(address), n * 4, 2) == 0  # hipMemcpyDeviceToHost
    return out


@pytest.fixture(scope="module")
def small_sams(tmp_path_factory):
    from svim_asm_amd import synth_bam
    d = str(tmp_path_factory.mktemp("gpusam"))
    contigs = (("chrA", 900000), ("chrB", 600000), ("chrC", 400000))
    fa, bams = synth_bam.write_dataset(d, seed=23, contigs=contigs, n_shared=14, n_private=4, median_aln=120000, mean_m=12)
    sams = [stw.bam_as_sam(b, b[:-4] + ".sam", shuffle_seed=k) for k, b in enumerate(bams)]
    return fa, bams, sams


@pytest.mark.parametrize("device_parse", ["1", "0"])
def test_reader_pool_in_hbm_equals_the_host_column(svx_ctx, small_sams, device_parse, monkeypatch):
    from svim_asm_amd import bamio
    monkeypatch.setenv("SVX_SAM_DEVICE", device_parse)
    _, bams, sams = small_sams
    f = bamio.AlignmentFile(sams[0], device=0)
    f.load()
    assert f.is_sam and f.parsed_on_device == (device_parse == "1") and f.cigar_pinned
    address, _none, _us = f.device_pool(wait=True)
    assert np.array_equal(device_words(address, len(f._cigar)), f._cigar)
    b = bamio.AlignmentFile(bams[0])
    b.load()
    assert np.array_equal(f._cigar, b._cigar) and np.array_equal(f._cig_off, b._cig_off)
    for k in ("tid", "pos", "flag", "mapq", "l_seq", "ref_len"):
        assert np.array_equal(f._cols[k], b._cols[k]), k


def _vcf(path):
    return "".join(l for l in open(path) if not l.startswith("##fileDate="))


@pytest.mark.parametrize("device_parse", ["1", "0"])
def test_config1_diploid_from_shuffled_sams(svx_ctx, tmp_path, device_parse, monkeypatch):
    from svim_asm_amd import cli
    monkeypatch.setenv("SVX_SAM_DEVICE", device_parse)
    g = os.path.join(GOLD, "config1")
    sams = [stw.bam_as_sam(os.path.join(g, "hap%d.bam" % (k + 1)), str(tmp_path / ("h%d.sam" % k)), shuffle_seed=40 + k) for k in range(2)]
    cli.main(["diploid", str(tmp_path / "wd"), sams[0], sams[1], os.path.join(g, "ref.fa")])
    assert _vcf(tmp_path / "wd" / "variants.vcf") == open(os.path.join(g, "diploid_default.vcf")).read()


@pytest.fixture(scope="module")
def medium_sams(tmp_path_factory):
    from svim_asm_amd import synth, synth_bam
    from tests import helpers
    meta = json.load(open(os.path.join(GOLD, "medium_inputs.json")))
    prm = meta["params"]
    contigs = tuple((n, max(60000, int(l * prm["scale"]))) for n, l in zip(synth.GRCH38_NAMES, synth.GRCH38_LENGTHS))
    d = str(tmp_path_factory.mktemp("mediumsam"))
    fasta, bams = synth_bam.write_dataset(d, seed=prm["seed"], contigs=contigs, n_shared=prm["n_shared"],
                                          n_private=prm["n_private"], median_aln=prm["median_aln"], mean_m=prm["mean_m"])
    helpers.assert_inputs_are_the_golden_ones(meta, [fasta] + bams)
    return fasta, [stw.bam_as_sam(b, b[:-4] + ".sam", shuffle_seed=60 + k) for k, b in enumerate(bams)]


@pytest.mark.parametrize("device_parse", ["1", "0"])
def test_medium_diploid_from_shuffled_sams(svx_ctx, medium_sams, tmp_path, device_parse, monkeypatch):
    from svim_asm_amd import cli
    monkeypatch.setenv("SVX_SAM_DEVICE", device_parse)
    fasta, sams = medium_sams
    cli.main(["diploid", str(tmp_path), sams[0], sams[1], fasta])
    assert _vcf(tmp_path / "variants.vcf") == gzip.open(os.path.join(GOLD, "medium_diploid.vcf.gz"), "rb").read().decode()
