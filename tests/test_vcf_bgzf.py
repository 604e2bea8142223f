"""`--bgzip_output` on the host path (SVX_VCF_BGZF_DEVICE=0: zlib on host threads; the other kernels answered by the
oracle): variants.vcf.gz decompresses to the golden VCFs with the structure bgzip writes, its tabix index answers region
queries exactly (tests/tabix_reader.py, written from the specs), and the index builder (svx_tabix_build) follows
tbx_parse1's interval rules, switches to CSI beyond 2^29 and refuses records it cannot index."""
import gzip
import logging
import os
import zlib

import numpy as np
import pytest

from svim_asm_amd import vcf_bgzf
from tests import helpers, tabix_reader
from tests.test_fasta_bgzf import bgzipped_config1, damage_member, member_spans
from tests.test_oracle_pins import RUNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "config1")


def mask_date(text):
    return b"".join(l for l in text.splitlines(keepends=True) if not l.startswith(b"##fileDate="))


def run_cli(argv, wd):
    from svim_asm_amd import cli
    argv = list(argv)
    argv[1] = str(wd)
    for i, a in enumerate(argv):
        if a.endswith((".bam", ".fa")):
            argv[i] = os.path.join(GOLD, a)
    cli.main(argv + ["--bgzip_output"])


def random_regions(text, reader, seed, n=500):
    """The whole of every contig plus n seeded regions (some on multiples of 16 384) answer the brute-force set."""
    rng = np.random.default_rng(seed)
    names = [x.decode() for x in reader.index.names]
    ends = {}
    for line in text.split(b"\n"):
        if line and not line.startswith(b"#"):
            ends[line.split(b"\t")[0].decode()] = max(ends.get(line.split(b"\t")[0].decode(), 0), tabix_reader.interval(line)[1])
    for name in names:
        assert reader.query(name, 0, 1 << 31) == tabix_reader.brute(text, name, 0, 1 << 31)
        assert reader.index.record_count(name) == len(tabix_reader.brute(text, name, 0, 1 << 31))
    for k in range(n):
        name = names[int(rng.integers(0, len(names)))]
        top = ends[name] + 20000
        if k % 4 == 0:
            b = int(rng.integers(0, top // 16384 + 1)) * 16384
            e = b + int(rng.integers(1, 4)) * 16384
        else:
            b = int(rng.integers(0, top))
            e = b + int(rng.integers(1, 200000))
        assert reader.query(name, b, e) == tabix_reader.brute(text, name, b, e), (name, b, e)


@pytest.fixture
def host_path(monkeypatch):
    monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", "0")
    helpers.oracle_backed_device(monkeypatch)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_cli_bgzip_output_matches_the_goldens(tmp_path, host_path, name):
    run_cli(RUNS[name], tmp_path)
    assert not os.path.exists(tmp_path / "variants.vcf")
    blob = open(tmp_path / "variants.vcf.gz", "rb").read()
    text = gzip.decompress(blob)
    assert mask_date(text) == open(os.path.join(GOLD, name + ".vcf"), "rb").read()
    tabix_reader.check_bgzf(blob, text)
    assert os.path.exists(tmp_path / "variants.vcf.gz.tbi") and not os.path.exists(tmp_path / "variants.vcf.gz.csi")
    assert os.path.getmtime(tmp_path / "variants.vcf.gz.tbi") >= os.path.getmtime(tmp_path / "variants.vcf.gz")
    reader = tabix_reader.Reader(blob, open(tmp_path / "variants.vcf.gz.tbi", "rb").read())
    random_regions(text, reader, seed=len(name))


def test_cohort_passes_the_option_through(tmp_path, host_path, monkeypatch):
    from svim_asm_amd import cli, cohort
    monkeypatch.setattr(cli, "_warm_device", lambda device: None)
    rows = [("s1", "hap1.bam", "hap2.bam"), ("s2", "hap1.bam", "hap2.bam")]
    manifest = tmp_path / "cohort.tsv"
    manifest.write_text("".join("%s %s %s\n" % (tmp_path / wd, os.path.join(GOLD, a), os.path.join(GOLD, b)) for wd, a, b in rows))
    assert cohort.main(["diploid", str(manifest), os.path.join(GOLD, "ref.fa"), "--bgzip_output"]) == 0
    for wd, _, _ in rows:
        assert not os.path.exists(tmp_path / wd / "variants.vcf")
        got = mask_date(gzip.decompress(open(tmp_path / wd / "variants.vcf.gz", "rb").read()))
        assert got == open(os.path.join(GOLD, "diploid_default.vcf"), "rb").read()
        assert os.path.exists(tmp_path / wd / "variants.vcf.gz.tbi")


def test_damaged_genome_member_leaves_neither_file(tmp_path, host_path):
    from svim_asm_amd import cli
    d = bgzipped_config1(tmp_path, level=6)
    for k in range(len(member_spans(str(d / "ref.fa.gz"))) - 1):
        damage_member(str(d / "ref.fa.gz"), k, "crc")
    wd = tmp_path / "wd"
    wd.mkdir()
    with pytest.raises(ValueError):
        cli.main(["diploid", str(wd), str(d / "hap1.bam"), str(d / "hap2.bam"), str(d / "ref.fa.gz"), "--bgzip_output"])
    for f in ("variants.vcf.gz", "variants.vcf.gz.tbi", "variants.vcf.gz.csi", "variants.vcf"):
        assert not os.path.exists(wd / f)


# ------------------------------------------------------------------ the builder on handcrafted text
HEADER = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def rec(chrom, pos, ref=b"N", info=b"."):
    return b"%s\t%d\tid\t%s\t<DEL>\t.\tPASS\t%s\n" % (chrom.encode(), pos, ref, info)


def index_of(text):
    blob, sizes = vcf_bgzf.compress(text)
    raw, kind = vcf_bgzf.build_index(text, sizes)
    return blob, raw, kind


def reader_of(text):
    blob, raw, kind = index_of(text)
    return tabix_reader.Reader(blob, vcf_bgzf.compress(raw)[0]), kind


def test_end_rules():
    text = HEADER + rec("c", 100, b"ACGT", b"SVTYPE=DEL;END=5000") + rec("c", 200, b"A", b"CIEND=-5,5;SVEND=90000") + \
        rec("c", 300, b"AC", b"END=.") + rec("c", 400, b"ACGTA", b"END=350") + rec("c", 500, b"", b"END=500") + \
        rec("c", 600, b"A", b"END=70000;X=1")
    r, kind = reader_of(text)
    assert kind == "tbi"
    assert [tabix_reader.interval(l) for l in text.split(b"\n")[2:-1]] == \
        [(99, 5000), (199, 200), (299, 301), (399, 404), (499, 500), (599, 70000)]
    for b, e in [(0, 1 << 30), (4999, 5000), (5000, 5001), (200, 201), (300, 301), (403, 404), (404, 405), (65000, 65001),
                 (69999, 70000), (70000, 80000), (16384, 32768)]:
        assert r.query("c", b, e) == tabix_reader.brute(text, "c", b, e), (b, e)


def test_record_spanning_a_member_boundary():
    lines = [HEADER]
    pos = 1
    rng = np.random.default_rng(3)
    while sum(map(len, lines)) < 3 * 65280 + 1000:
        seq = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(rng.integers(1, 3000)))])
        lines.append(rec("chr1" if pos < 5_000_000 else "chr2", pos, seq, b"END=%d" % (pos + int(rng.integers(0, 40000)))))
        pos += int(rng.integers(0, 20000))
    text = b"".join(lines)
    blob, raw, kind = index_of(text)
    spans = np.cumsum([len(l) for l in lines])
    assert any(s % 65280 != 0 and (s // 65280) != ((s - len(l)) // 65280) for s, l in zip(spans, lines))  # crosses a boundary
    tabix_reader.check_bgzf(blob, text)
    r = tabix_reader.Reader(blob, vcf_bgzf.compress(raw)[0])
    random_regions(text, r, seed=7, n=300)


def test_positions_beyond_2_29_make_a_csi():
    text = HEADER + rec("big", 10) + rec("big", 600_000_000, b"A", b"END=600100000") + rec("big", 900_000_000) + \
        rec("small", 5, b"AC") + rec("small", 536_870_000, b"A", b"END=536871000")
    r, kind = reader_of(text)
    assert kind == "csi" and r.index.csi and (r.index.min_shift, r.index.depth) == (14, 6)
    for name, b, e in [("big", 0, 1 << 32), ("big", 600_050_000, 600_050_001), ("big", 899_999_999, 900_000_000),
                       ("big", 100, 599_999_999), ("small", 536_870_911, 536_870_913), ("small", 0, 10)]:
        assert r.query(name, b, e) == tabix_reader.brute(text, name, b, e), (name, b, e)
    assert r.index.record_count("big") == 3


@pytest.mark.parametrize("case", ["interleaved", "decreasing"])
def test_unordered_records_are_refused(case):
    if case == "interleaved":
        text = HEADER + rec("chr1", 10) + rec("chr01", 20) + rec("chr1", 30)
    else:
        text = HEADER + rec("chr1", 100) + rec("chr1", 50)
    blob, sizes = vcf_bgzf.compress(text)
    with pytest.raises(vcf_bgzf.Unordered) as ei:
        vcf_bgzf.build_index(text, sizes)
    assert ("chr1\t30" if case == "interleaved" else "chr1\t50") in str(ei.value)


def test_unordered_run_writes_the_vcf_without_index(tmp_path, caplog):
    text = HEADER + rec("chr1", 10) + rec("chr01", 20) + rec("chr1", 30)
    path = str(tmp_path / "variants.vcf.gz")
    for stale in (".tbi", ".csi"):
        open(path + stale, "wb").write(b"stale")
    with caplog.at_level(logging.WARNING):
        assert vcf_bgzf.write(path, text) is None
    assert gzip.decompress(open(path, "rb").read()) == text
    assert not os.path.exists(path + ".tbi") and not os.path.exists(path + ".csi")
    assert "not indexed" in caplog.text and "chr1\t30" in caplog.text


def test_host_compressor_edges():
    for data in [b"", b"x", bytes(65279), bytes(65280), bytes(65281), os.urandom(200_000), b"A" * 300_000]:
        blob, sizes = vcf_bgzf.compress(data)
        if data:
            assert tabix_reader.check_bgzf(blob, data) == list(sizes)
        else:
            assert blob == tabix_reader.EOF_MEMBER and len(sizes) == 0
        assert all(s <= 65536 for s in sizes)
    blob, _ = vcf_bgzf.compress(os.urandom(65280 * 2))
    for m in tabix_reader.members(blob)[:-1]:
        assert m[2][0] & 7 == 1  # stored (BFINAL 1, BTYPE 00)


def test_option_is_off_by_default():
    from svim_asm_amd import SVIM_input_parsing
    o = SVIM_input_parsing.parse_arguments("x", ["haploid", "/tmp/wd", "a.bam", "r.fa"])
    assert o.bgzip_output is False
    o = SVIM_input_parsing.parse_arguments("x", ["diploid", "/tmp/wd", "a.bam", "b.bam", "r.fa", "--bgzip_output"])
    assert o.bgzip_output is True
