"""The device path of bgzip-compressed reference genomes (svx_fasta_set_device: members staged, inflated and checked by
svx_inflate.hip's kernels, resident on the device, windows gathered by svx_fasta_gather.hip): forced on (minimum one
member) with a small token arena, it writes what the host path and the plain file write, counts exactly the distinct
members under the windows as inflated on the device (a silent fall-back to the host fails), inflates nothing again on a
repeated call, fails a damaged member as the host does; and `svim-asm` / `svim-asm-cohort` on a bgzipped config-1
genome write the golden VCFs."""
import os

import numpy as np
import pytest

from svim_asm_amd import _lib, fasta
from tests.test_fasta_bgzf import (FORMS, GENOMES, GOLD, RUNS, bgzipped_config1, compressed, damage_member, random_genome,
                                   random_windows, write_text_fasta)

pytestmark = pytest.mark.gpu


@pytest.fixture
def small_arena():
    lib = _lib.load()
    old = lib.svx_bgzf_inflate_set_arena(7)
    yield
    lib.svx_bgzf_inflate_set_arena(old)


def device_file(path):
    z = fasta.FastaFile(path)
    lib, h = z._native
    assert lib.svx_fasta_set_device(h, 0, 1) == 0
    return z


def distinct_members(z, names, ids, st, en):
    """Members under the windows, from the .gzi (uncompressed starts) and the .fai geometry."""
    _, uoff = fasta.read_gzi(z.filename + ".gzi")
    starts = np.concatenate([[0], uoff.astype(np.int64)])
    seen = set()
    for c, a, b in zip(ids.tolist(), st.tolist(), en.tolist()):
        length, off, lb, lw = z._idx[names[c]]
        b = min(b, length)
        if b <= a:
            continue
        u0 = off + (a // lb) * lw + a % lb
        u1 = off + ((b - 1) // lb) * lw + (b - 1) % lb
        seen.update(range(int(np.searchsorted(starts, u0, "right")) - 1, int(np.searchsorted(starts, u1, "right"))))
    return len(seen)


@pytest.mark.parametrize("line,crlf", GENOMES)
@pytest.mark.parametrize("level,member", FORMS[1:3] + FORMS[4:])
def test_device_fetch_equals_host_and_plain(tmp_path, small_arena, line, crlf, level, member):
    names, seqs = random_genome(line)
    plain = write_text_fasta(str(tmp_path / "ref.fa"), names, seqs, line, crlf)
    path = compressed(tmp_path, plain, level, member)
    p, host, dev = fasta.FastaFile(plain), fasta.FastaFile(path), device_file(path)
    _, uoff = fasta.read_gzi(path + ".gzi")
    rng = np.random.default_rng(line + level + member)
    ids, st, en = random_windows(rng, p, names, 20_000, [int(u) for u in uoff])
    want = distinct_members(dev, names, ids, st, en)
    for upper in (True, False):
        a = p.fetch_batch(names, st, en, upper=upper, ids=ids)
        b = host.fetch_batch(names, st, en, upper=upper, ids=ids)
        c = dev.fetch_batch(names, st, en, upper=upper, ids=ids)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    s = dev.stats()
    assert s["device_members"] == want, s           # every member once, on the device
    assert s["host_members"] == 0 and s["device_calls"] == 2
    assert s["cache_hits"] >= want                  # the second call found them all resident
    # a repeated call inflates nothing new
    dev.fetch_batch(names, st[:500], en[:500], ids=ids[:500])
    assert dev.stats()["device_members"] == want
    dev.close()
    fasta.release_deferred(background=False)


def test_damaged_member_fails_on_the_device_as_on_the_host(tmp_path):
    names, seqs = random_genome(60)
    plain = write_text_fasta(str(tmp_path / "ref.fa"), names, seqs, 60)
    path = str(tmp_path / "ref.fa.gz")
    fasta.bgzip_fasta(plain, path, level=6, member_size=5000)
    coff = damage_member(path, 5, "crc")
    host, dev = fasta.FastaFile(path), device_file(path)
    L = host.get_reference_length(names[0])
    st, en = np.arange(0, L - 100, 97, dtype=np.int64), np.arange(0, L - 100, 97, dtype=np.int64) + 100
    for z in (host, dev):
        with pytest.raises(ValueError) as ei:
            z.fetch_batch([names[0]] * len(st), st, en)
        assert str(coff) in str(ei.value)
    assert dev.stats()["host_members"] == 0
    # windows elsewhere still succeed on the device
    p = fasta.FastaFile(plain)
    out = dev.fetch_batch([names[2]] * 50, np.arange(50, dtype=np.int64) * 900, np.arange(50, dtype=np.int64) * 900 + 800)
    assert np.array_equal(out[0], p.fetch_batch([names[2]] * 50, np.arange(50) * 900, np.arange(50) * 900 + 800)[0])
    assert dev.stats()["device_members"] > 0


@pytest.mark.parametrize("name", ["haploid_default", "diploid_default", "diploid_options"])
def test_cli_goldens_with_a_bgzipped_genome_on_the_device(tmp_path, monkeypatch, name):
    from svim_asm_amd import cli
    monkeypatch.setenv("SVX_FASTA_DEVICE", "1")
    monkeypatch.setattr(fasta, "DEVICE_MIN_MEMBERS", 1)
    opened = []
    real = fasta.FastaFile.__init__

    def spy(self, *a, **k):
        real(self, *a, **k)
        opened.append(self)
    monkeypatch.setattr(fasta.FastaFile, "__init__", spy)
    d = bgzipped_config1(tmp_path)
    argv = list(RUNS[name])
    argv[1] = str(tmp_path / "wd")
    for i, a in enumerate(argv):
        if a.endswith(".bam"):
            argv[i] = str(d / a)
        elif a.endswith(".fa"):
            argv[i] = str(d / "ref.fa.gz")
    cli.main(argv)
    got = "".join(l for l in open(tmp_path / "wd" / "variants.vcf") if not l.startswith("##fileDate="))
    assert got == open(os.path.join(GOLD, "config1", name + ".vcf")).read()
    assert opened and opened[0].compressed
    s = opened[0].stats()
    assert s["device_members"] > 0 and s["host_members"] == 0, s


def test_cohort_with_a_bgzipped_genome_on_the_device(tmp_path, monkeypatch):
    from svim_asm_amd import cohort
    monkeypatch.setenv("SVX_FASTA_DEVICE", "1")
    monkeypatch.setattr(fasta, "DEVICE_MIN_MEMBERS", 1)
    d = bgzipped_config1(tmp_path)
    rows = [("s1", "hap1.bam", "hap2.bam"), ("s2", "hap1.bam", "hap2.bam"), ("s3", "hap1.bam", "hap2.bam")]
    manifest = tmp_path / "cohort.tsv"
    manifest.write_text("".join("%s %s %s\n" % (tmp_path / wd, d / a, d / b) for wd, a, b in rows))
    assert cohort.main(["diploid", str(manifest), str(d / "ref.fa.gz")]) == 0
    for wd, _, _ in rows:
        got = "".join(l for l in open(tmp_path / wd / "variants.vcf") if not l.startswith("##fileDate="))
        assert got == open(os.path.join(GOLD, "config1", "diploid_default.vcf")).read()


# ---- the medium and full-size samples with their genome bgzipped (the default arena: > 20 480 members at full size go
# out in slices; the arena grows by doubling as PAIR's windows and then the VCF's alleles need members)
from tests.test_full_golden import META as FULL_META, _check as check_full_vcf, full_dataset  # noqa: E402,F401
from tests.test_medium_golden import expected_vcf as medium_vcf, medium_dataset  # noqa: E402,F401


def bgzipped(fasta_path, out_dir):
    from tests.test_fasta_bgzf import have_libdeflate
    out = os.path.join(str(out_dir), os.path.basename(fasta_path) + ".gz")
    fasta.bgzip_fasta(fasta_path, out, level=106 if have_libdeflate() else 6, threads=16)
    return out


def device_stats_spy(monkeypatch):
    opened = []
    real = fasta.FastaFile.__init__

    def spy(self, *a, **k):
        real(self, *a, **k)
        opened.append(self)
    monkeypatch.setattr(fasta.FastaFile, "__init__", spy)
    return opened


@pytest.fixture(scope="module")
def medium_gz(medium_dataset, tmp_path_factory):
    return bgzipped(medium_dataset[0], tmp_path_factory.mktemp("medium_gz"))


@pytest.mark.parametrize("path", ["device", "host"])
def test_medium_golden_with_a_bgzipped_genome(svx_ctx, medium_dataset, medium_gz, tmp_path, monkeypatch, path):
    from svim_asm_amd import cli
    monkeypatch.setenv("SVX_FASTA_DEVICE", "1" if path == "device" else "0")
    monkeypatch.setattr(fasta, "DEVICE_MIN_MEMBERS", 1)
    opened = device_stats_spy(monkeypatch)
    bams = medium_dataset[1]
    cli.main(["diploid", str(tmp_path), bams[0], bams[1], medium_gz])
    got = "".join(l for l in open(tmp_path / "variants.vcf") if not l.startswith("##fileDate="))
    assert got == medium_vcf()
    s = opened[0].stats()
    if path == "device":
        assert s["device_members"] > 0 and s["host_members"] == 0, s
    else:
        assert s["device_members"] == 0 and s["host_members"] > 0, s


@pytest.mark.spawns_gpu_children
def test_two_rank_medium_golden_with_a_bgzipped_genome(medium_dataset, medium_gz, tmp_path, monkeypatch):
    from tests import helpers
    monkeypatch.setenv("SVX_FASTA_DEVICE", "1")
    bams = medium_dataset[1]
    res = helpers.run_cli_ranks(["diploid", str(tmp_path), bams[0], bams[1], medium_gz], 2)
    for rank, (rc, text) in enumerate(res):
        assert rc == 0, "rank %d failed:\n%s" % (rank, text)
    got = "".join(l for l in open(tmp_path / "variants.vcf") if not l.startswith("##fileDate="))
    assert got == medium_vcf()


def test_full_size_digest_with_a_bgzipped_genome(svx_ctx, full_dataset, tmp_path, monkeypatch):
    """`svim-asm diploid OUT h1.bam h2.bam GRCh38-sized.fa.gz` writes the VCF of the plain genome (the real reference's
    digest), with the members inflated on the device."""
    from svim_asm_amd import cli
    monkeypatch.setenv("SVX_FASTA_DEVICE", "1")
    opened = device_stats_spy(monkeypatch)
    fa, bams = full_dataset
    gz = bgzipped(fa, tmp_path)
    cli.main(["diploid", str(tmp_path / "wd"), bams[0], bams[1], gz])
    check_full_vcf(tmp_path / "wd" / "variants.vcf")
    s = opened[0].stats()
    # (PAIR's windows and the VCF's alleles in device calls; a call under fasta.DEVICE_MIN_MEMBERS stays on the host)
    assert s["device_members"] > 20480 and s["device_calls"] >= 2 and s["host_members"] < 64, s
