"""PAF input on the GPU: the oriented gather kernel (k_fasta_gather_oriented, csrc/svx_fasta_gather.hip) against the
restatement of tests/test_fasta_oriented.py, the PAF reader with a device (CIGAR text parsed by the kernels equals the
threads' words, pool in HBM), and PAF + bgzip-compressed query assemblies through the real device pipeline against the
committed golden VCFs."""
import gzip
import json
import os

import numpy as np
import pytest

from tests import paf_writer as pw
from tests.test_fasta_oriented import restated
from tests.test_gpu_sam import device_words

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _vcf(path):
    return "".join(l for l in open(path) if not l.startswith("##fileDate="))


@pytest.mark.parametrize("line", [60, 0, 1])
def test_oriented_gather_kernel_equals_the_restatement(svx_ctx, tmp_path, line, monkeypatch):
    """Members of several sizes (the file is compressed in pieces of 300 .. 65280 bytes), reversed windows that span two
    and more members, windows of one base, windows at both ends of a contig; every window once on the device and once
    on the host threads."""
    from svim_asm_amd import bamio, fasta
    rng = np.random.default_rng(9)
    letters = np.frombuffer(b"ACGTACGTacgtNnRYKMSWBDHVrykmswbdhv=Xu", np.uint8)
    seqs = {"s%d" % k: letters[rng.integers(0, len(letters), n)].tobytes() for k, n in enumerate((1, 70000, 400000, 123457, 61))}
    plain = pw.write_fasta(str(tmp_path / "q.fa"), list(seqs), list(seqs.values()), line=line)
    # members of several sizes: the file compressed piece by piece
    data = open(plain, "rb").read()
    sizes, parts, entries, at, coff = [300, 65280, 4096, 1, 20000, 65280, 777], [], [], 0, 0
    k = 0
    while at < len(data):
        n = sizes[k % len(sizes)]
        if at:
            entries.append((coff, at))
        parts.append(bamio._bgzf_member(memoryview(data)[at:at + n], 6))
        coff += len(parts[-1])
        at += n
        k += 1
    path = plain + ".gz"
    with open(path, "wb") as fh:
        fh.write(b"".join(parts) + bamio._BGZF_EOF)
    import struct
    with open(path + ".gzi", "wb") as fh:
        fh.write(struct.pack("<Q", len(entries)) + b"".join(struct.pack("<QQ", c, u) for c, u in entries))
    open(path + ".fai", "w").write(open(plain + ".fai").read())

    names, start, end = [], [], []
    for name, s in seqs.items():
        n = len(s)
        cases = [(0, n), (0, 1), (n - 1, n), (n // 2, n // 2 + 1), (0, min(n, 100)), (max(0, n - 100), n + 7)]
        cases += [tuple(sorted(rng.integers(0, n + 1, 2).tolist())) for _ in range(60)]
        cases += [(a, min(n, a + int(rng.integers(1, 500)))) for a in rng.integers(0, n, 200).tolist()]
        for a, b in cases:
            names.append(name); start.append(a); end.append(b)
    start, end = np.array(start), np.array(end)
    rev = rng.integers(0, 2, len(names)).astype(bool)
    rev[:6] = True
    monkeypatch.setenv("SVX_FASTA_DEVICE", "1")
    monkeypatch.setattr(fasta, "DEVICE_MIN_MEMBERS", 1)  # (every batch call on the device, however few members it touches)
    dev = fasta.FastaFile(path, device=0)
    for bam_alphabet in (True, False):
        out, off = dev.fetch_oriented(names, start, end, rev, bam_alphabet=bam_alphabet)
        for i, name in enumerate(names):
            exp = restated(seqs[name], int(start[i]), int(end[i]), bool(rev[i]), bam_alphabet)
            assert out[off[i]:off[i + 1]].tobytes() == exp, (name, int(start[i]), int(end[i]), bool(rev[i]), bam_alphabet)
    st = dev.stats()
    assert st["device_calls"] == 2 and st["device_members"] > 0, st   # (the kernel ran: no quiet host path)
    monkeypatch.setenv("SVX_FASTA_DEVICE", "0")
    host = fasta.FastaFile(path, device=0)
    h_out, h_off = host.fetch_oriented(names, start, end, rev)
    d_out, d_off = dev.fetch_oriented(names, start, end, rev)
    assert np.array_equal(h_out, d_out) and np.array_equal(h_off, d_off) and host.stats()["device_calls"] == 0
    # the unoriented gather beside it is what it was
    a, _ = dev.fetch_batch(names, start, end, upper=True)
    b, _ = host.fetch_batch(names, start, end, upper=True)
    assert np.array_equal(a, b)


@pytest.fixture(scope="module")
def small_pafs(tmp_path_factory):
    from svim_asm_amd import synth_bam
    d = str(tmp_path_factory.mktemp("gpupaf"))
    contigs = (("chrA", 900000), ("chrB", 600000), ("chrC", 400000))
    fa, bams = synth_bam.write_dataset(d, seed=23, contigs=contigs, n_shared=14, n_private=4, median_aln=120000, mean_m=12)
    return fa, bams, [pw.bam_as_paf(b, b[:-4] + ".paf", b[:-4] + ".query.fa", shuffle_seed=k) for k, b in enumerate(bams)]


def test_load_with_device_parse_equals_load_with_thread_parse(svx_ctx, small_pafs, monkeypatch):
    from svim_asm_amd import bamio
    ref, bams, pafs = small_pafs
    got = {}
    for device_parse in ("1", "0"):
        monkeypatch.setenv("SVX_SAM_DEVICE", device_parse)
        f = bamio.AlignmentFile(pafs[0][0], device=0, query=pafs[0][1], reference=ref)
        f.load()
        assert f.is_paf and f.parsed_on_device == (device_parse == "1") and f.cigar_pinned
        address, _none, _us = f.device_pool(wait=True)
        assert np.array_equal(device_words(address, len(f._cigar)), f._cigar)
        got[device_parse] = (f._cigar.copy(), f._cig_off.copy(), {k: v.copy() for k, v in f._cols.items()}, f._aux_pool, f._names_pool)
        f.close()
    a, b = got["1"], got["0"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3] and a[4] == b[4]
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k
    # and both are the BAM's records (flag-4 records have no row)
    bam = bamio.AlignmentFile(bams[0])
    bam.load()
    keep = (bam._cols["flag"] & 4) == 0
    for k in ("tid", "pos", "mapq", "l_seq", "ref_len", "n_cig"):
        assert np.array_equal(a[2][k], bam._cols[k][keep]), k


@pytest.mark.parametrize("device_parse", ["1", "0"])
def test_config1_diploid_from_pafs_and_compressed_assemblies(svx_ctx, tmp_path, device_parse, monkeypatch):
    from svim_asm_amd import cli, fasta
    monkeypatch.setenv("SVX_SAM_DEVICE", device_parse)
    g = os.path.join(GOLD, "config1")
    argv = ["diploid", str(tmp_path / "wd")]
    extra = []
    for k in range(2):
        paf, fa = pw.bam_as_paf(os.path.join(g, "hap%d.bam" % (k + 1)), str(tmp_path / ("h%d.paf" % k)), str(tmp_path / ("q%d.fa" % k)),
                                shuffle_seed=40 + k)
        argv.append(paf)
        extra += ["--query%d" % (k + 1), fasta.bgzip_fasta(fa, fa + ".gz", member_size=2000)]
    cli.main(argv + [os.path.join(g, "ref.fa")] + extra)
    assert _vcf(tmp_path / "wd" / "variants.vcf") == open(os.path.join(g, "diploid_default.vcf")).read()


@pytest.fixture(scope="module")
def medium_pafs(tmp_path_factory):
    from svim_asm_amd import fasta, synth, synth_bam
    from tests import helpers
    meta = json.load(open(os.path.join(GOLD, "medium_inputs.json")))
    prm = meta["params"]
    contigs = tuple((n, max(60000, int(l * prm["scale"]))) for n, l in zip(synth.GRCH38_NAMES, synth.GRCH38_LENGTHS))
    d = str(tmp_path_factory.mktemp("mediumpaf"))
    ref, bams = synth_bam.write_dataset(d, seed=prm["seed"], contigs=contigs, n_shared=prm["n_shared"],
                                        n_private=prm["n_private"], median_aln=prm["median_aln"], mean_m=prm["mean_m"])
    helpers.assert_inputs_are_the_golden_ones(meta, [ref] + bams)
    out = []
    for k, b in enumerate(bams):
        paf, fa = pw.bam_as_paf(b, b[:-4] + ".paf", b[:-4] + ".query.fa", shuffle_seed=60 + k)  # (asserts the lossless conditions)
        out.append((paf, fasta.bgzip_fasta(fa, fa + ".gz", threads=8)))
    return ref, out


@pytest.mark.parametrize("device_parse", ["1", "0"])
def test_medium_diploid_from_pafs_and_compressed_assemblies(svx_ctx, medium_pafs, tmp_path, device_parse, monkeypatch):
    """The medium inputs satisfy the lossless-conversion conditions (tests/paf_writer.alns_of_bam asserts them while it
    converts), so the committed golden, written from the BAMs, is the expected output."""
    from svim_asm_amd import cli
    monkeypatch.setenv("SVX_SAM_DEVICE", device_parse)
    ref, pafs = medium_pafs
    cli.main(["diploid", str(tmp_path), pafs[0][0], pafs[1][0], ref, "--query1", pafs[0][1], "--query2", pafs[1][1]])
    assert _vcf(tmp_path / "variants.vcf") == gzip.open(os.path.join(GOLD, "medium_diploid.vcf.gz"), "rb").read().decode()
