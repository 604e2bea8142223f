"""bgzip-compressed reference genomes (`ref.fa.gz` + `.fai` + `.gzi`, htslib faidx semantics) on the host path of
svim_asm_amd/fasta.py and libsvx.so (svx_fasta_open_bgzf): every fetch form equals the plain file's answer on seeded
genomes written plain and bgzipped at several levels and member sizes; malformed inputs are refused; a damaged member
fails the windows under it and no other; `svim-asm` on a bgzipped config-1 genome writes the golden VCFs (the device
answered by the oracle) and writes no VCF when the `.gzi` is missing or a member is damaged."""
import os
import shutil
import struct
import zlib

import numpy as np
import pytest

from svim_asm_amd import bamio, fasta
from tests import helpers
from tests.test_oracle_pins import RUNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def have_libdeflate():
    return bamio._libdeflate_compress(b"ACGT" * 100, 6) is not None


def write_text_fasta(path, names, seqs, line, crlf=False):
    """A plain FASTA (+ .fai) with `line` bases per line, LF or CRLF line ends, a partial last line where it falls."""
    eol = b"\r\n" if crlf else b"\n"
    with open(path, "wb") as fh, open(path + ".fai", "w") as fai:
        for name, seq in zip(names, seqs):
            fh.write(b">" + name.encode() + eol)
            off = fh.tell()
            for p in range(0, len(seq), line):
                fh.write(seq[p:p + line] + eol)
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), off, line, line + len(eol)))
    return path


def random_genome(seed):
    """Contigs with lower-case and N runs, one shorter than a line."""
    rng = np.random.default_rng(seed)
    names, seqs = [], []
    for k, n in enumerate((50_000, 7, 123_457, 65_280, 3_001)):
        a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
        for _ in range(6):
            p = int(rng.integers(0, n))
            q = min(n, p + int(rng.integers(1, 2000)))
            a[p:q] = ord("N") if rng.random() < 0.5 else a[p:q] | 0x20  # N run or lower case
        names.append("ctg%d" % k)
        seqs.append(a.tobytes())
    return names, seqs


GENOMES = [(60, False), (80, True), (1, False)]
FORMS = [(1, 0xFF00), (6, 0xFF00), (6, 4099), (106, 0xFF00), (106, 1777)]


@pytest.fixture(scope="module", params=GENOMES, ids=lambda p: "line%d%s" % (p[0], "crlf" if p[1] else ""))
def genome(request, tmp_path_factory):
    line, crlf = request.param
    d = tmp_path_factory.mktemp("genome")
    names, seqs = random_genome(line)
    plain = write_text_fasta(str(d / "ref.fa"), names, seqs, line, crlf)
    return d, plain, names


def compressed(d, plain, level, member, gzi_end=False):
    if level >= 100 and not have_libdeflate():
        pytest.skip("libdeflate is not installed here")
    out = str(d / ("ref.%d.%d.%d.fa.gz" % (level, member, gzi_end)))
    if not os.path.exists(out):
        fasta.bgzip_fasta(plain, out, level=level, member_size=member, threads=4, gzi_end=gzi_end)
    return out


def random_windows(rng, p, names, n, members):
    """Windows of every kind: empty, clipped at a contig end, ending on a member boundary, spanning many members, whole
    contigs."""
    ids, st, en = [], [], []
    for _ in range(n):
        c = int(rng.integers(0, len(names)))
        L = p.get_reference_length(names[c])
        kind = rng.integers(0, 6)
        a = int(rng.integers(0, L + 1))
        if kind == 0:
            b = a
        elif kind == 1:
            b = L + int(rng.integers(0, 100))
        elif kind == 2:
            b = a + int(rng.integers(0, 30_000))
        elif kind == 3:
            a, b = 0, L
        else:
            b = a + int(rng.integers(0, 300))
        ids.append(c)
        st.append(a)
        en.append(b)
    # windows that end exactly on a member boundary (uncompressed offsets of the members, mapped back to bases)
    for u in members[:200]:
        for c, name in enumerate(names):
            length, off, lb, lw = p._idx[name]
            if off <= u < off + (length // lb) * lw:
                base = (u - off) // lw * lb + min((u - off) % lw, lb)
                ids.append(c)
                st.append(max(0, base - int(rng.integers(0, 5000))))
                en.append(base)
    return np.array(ids), np.array(st, np.int64), np.array(en, np.int64)


@pytest.mark.parametrize("level,member", FORMS, ids=lambda v: str(v))
def test_every_fetch_form_equals_the_plain_file(genome, level, member):
    d, plain, names = genome
    path = compressed(d, plain, level, member)
    p, z = fasta.FastaFile(plain), fasta.FastaFile(path)
    assert z.compressed and not p.compressed
    _, uoff = fasta.read_gzi(path + ".gzi")
    rng = np.random.default_rng(level * 7 + member)
    ids, st, en = random_windows(rng, p, names, 20_000, [int(u) for u in uoff])
    for upper in (True, False):
        a, b = p.fetch_batch(names, st, en, upper=upper, ids=ids), z.fetch_batch(names, st, en, upper=upper, ids=ids)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    contigs = [names[i] for i in ids[:3000]]
    a, b = p.fetch_batch(contigs, st[:3000], en[:3000]), z.fetch_batch(contigs, st[:3000], en[:3000])
    assert np.array_equal(a[0], b[0])
    for k in range(0, len(ids), 37):
        c = names[ids[k]]
        assert z.fetch(c, int(st[k]), int(en[k])) == p.fetch(c, int(st[k]), int(en[k]))
        assert z.fetch_bytes(c, int(st[k]), int(en[k])) == p.fetch_bytes(c, int(st[k]), int(en[k]))
    for c in names:
        assert z.fetch(c) == p.fetch(c)
    s = z.stats()
    assert s["host_members"] > 0 and s["cache_hits"] > 0 and s["device_members"] == 0
    p.close()
    z.close()


def test_gzi_with_and_without_its_end_entry(genome):
    d, plain, names = genome
    p = fasta.FastaFile(plain)
    for end in (False, True):
        path = compressed(d, plain, 6, 3001, gzi_end=end)
        n = struct.unpack("<Q", open(path + ".gzi", "rb").read(8))[0]
        z = fasta.FastaFile(path)
        for c in names:
            assert z.fetch(c, 0, 10 ** 9) == p.fetch(c, 0, 10 ** 9)
        assert n == len(fasta.read_gzi(path + ".gzi")[0])


def test_plain_fasta_is_untouched(genome):
    _, plain, names = genome
    p = fasta.FastaFile(plain, device=0)
    assert not p.compressed and p._map is not None
    assert p.stats() == {k: 0 for k in ("host_members", "device_members", "bytes_staged", "cache_hits", "device_calls", "host_calls")}


# ------------------------------------------------------------------ refusals
@pytest.fixture
def small(tmp_path):
    names, seqs = random_genome(3)
    plain = write_text_fasta(str(tmp_path / "ref.fa"), names, seqs, 60)
    path = str(tmp_path / "ref.fa.gz")
    fasta.bgzip_fasta(plain, path, level=6, member_size=5000)
    return tmp_path, plain, path, names


def write_gzi(path, pairs):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<Q", len(pairs)))
        for c, u in pairs:
            fh.write(struct.pack("<QQ", c, u))


def test_missing_gzi_is_its_own_refusal(small):
    _, _, path, _ = small
    os.remove(path + ".gzi")
    with pytest.raises(fasta.MissingGziError):
        fasta.FastaFile(path)
    os.remove(path + ".fai")
    with pytest.raises(ValueError) as ei:
        fasta.FastaFile(path)
    assert not isinstance(ei.value, fasta.MissingGziError)  # a missing .fai is refused as before


@pytest.mark.parametrize("damage", ["not_monotone", "off_header", "past_end", "wrong_uoff"])
def test_malformed_gzi_is_refused(small, damage):
    _, _, path, _ = small
    coff, uoff = fasta.read_gzi(path + ".gzi")
    pairs = list(zip(coff.tolist(), uoff.tolist()))
    if damage == "not_monotone":
        pairs[2], pairs[3] = pairs[3], pairs[2]
    elif damage == "off_header":
        pairs[4] = (pairs[4][0] + 7, pairs[4][1])
    elif damage == "past_end":
        pairs.append((os.path.getsize(path) + 100, pairs[-1][1] + 5000))
    else:
        pairs[1] = (pairs[1][0], pairs[1][1] + 1)
    write_gzi(path + ".gzi", pairs)
    with pytest.raises(fasta.BgzfFormatError):
        fasta.FastaFile(path)


def test_plain_gzip_is_refused_with_a_bgzip_hint(small):
    tmp, plain, _, _ = small
    import gzip
    path = str(tmp / "plain.fa.gz")
    with open(plain, "rb") as a, gzip.open(path, "wb") as b:
        b.write(a.read())
    shutil.copy(plain + ".fai", path + ".fai")
    with pytest.raises(fasta.BgzfFormatError) as ei:
        fasta.FastaFile(path)
    assert "bgzip" in str(ei.value)


def test_truncated_file_is_refused(small):
    _, _, path, _ = small
    data = open(path, "rb").read()
    open(path, "wb").write(data[:len(data) // 2])
    with pytest.raises(fasta.BgzfFormatError):
        fasta.FastaFile(path)


def member_spans(path):
    """(offset, length, isize) of every member."""
    data = open(path, "rb").read()
    out, p = [], 0
    while p < len(data):
        bsize = struct.unpack_from("<H", data, p + 16)[0] + 1
        out.append((p, bsize, struct.unpack_from("<I", data, p + bsize - 4)[0]))
        p += bsize
    return out


def damage_member(path, k, how):
    """Member k made damaged in place, keeping its size: flipped CRC32, wrong ISIZE, or a malformed DEFLATE stream (a
    block of the reserved type 3 in front of garbage)."""
    data = bytearray(open(path, "rb").read())
    off, bsize, isize = member_spans(path)[k]
    if how == "crc":
        data[off + bsize - 8] ^= 0x5A
    elif how == "isize":
        struct.pack_into("<I", data, off + bsize - 4, isize - 1)
    else:
        data[off + 18] = 0x07  # BFINAL = 1, BTYPE = 11
    open(path, "wb").write(bytes(data))
    return off


@pytest.mark.parametrize("how", ["crc", "isize", "deflate"])
def test_damaged_member_fails_its_windows_only(small, how):
    _, plain, path, names = small
    p = fasta.FastaFile(plain)
    _, uoff = fasta.read_gzi(path + ".gzi")
    if how == "isize":
        # a wrong ISIZE in front of a .gzi entry contradicts the index: refused at open
        keep = open(path, "rb").read()
        damage_member(path, 5, how)
        with pytest.raises(fasta.BgzfFormatError):
            fasta.FastaFile(path)
        open(path, "wb").write(keep)
        k = len(uoff)  # ... in the last member with data, it is found when the member is inflated
        uoff = np.append(uoff, os.path.getsize(plain))
        name = names[-1]
    else:
        k = 5
        name = names[0]
    coff = damage_member(path, k, how)
    u0, u1 = int(uoff[k - 1]), int(uoff[k])  # member k holds uncompressed bytes [uoff[k - 1], uoff[k])
    z = fasta.FastaFile(path)
    length, off, lb, lw = p._idx[name]
    assert off < u0 and (u1 < off + length or how == "isize")
    base_at = lambda u: (u - off) // lw * lb + min((u - off) % lw, lb)  # the first base at or behind byte u
    inside = base_at(u0) + 3
    with pytest.raises(ValueError) as ei:
        z.fetch_batch([name], [inside], [inside + 10])
    assert str(coff) in str(ei.value)
    with pytest.raises(ValueError):
        z.fetch(name, inside, inside + 1)
    # a window elsewhere still succeeds
    if how != "isize":
        far = base_at(u1) + 200
        assert z.fetch(name, far, far + 500) == p.fetch(name, far, far + 500)
    assert z.fetch(names[2], 0, 1000) == p.fetch(names[2], 0, 1000)


# ------------------------------------------------------------------ the command
def bgzipped_config1(tmp_path, level=106):
    d = tmp_path / "in"
    d.mkdir()
    for f in ("hap1.bam", "hap1.bam.bai", "hap2.bam", "hap2.bam.bai"):
        os.symlink(os.path.join(GOLD, "config1", f), d / f)
    lvl = level if have_libdeflate() else 6
    fasta.bgzip_fasta(os.path.join(GOLD, "config1", "ref.fa"), str(d / "ref.fa.gz"), level=lvl, member_size=0xFF00, threads=4)
    return d


@pytest.mark.parametrize("name", sorted(RUNS))
def test_cli_reproduces_the_goldens_from_a_bgzipped_genome(tmp_path, monkeypatch, name):
    from svim_asm_amd import cli
    helpers.oracle_backed_device(monkeypatch)
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


def test_cli_writes_no_vcf_without_the_gzi(tmp_path, monkeypatch, caplog):
    from svim_asm_amd import cli
    helpers.oracle_backed_device(monkeypatch)
    d = bgzipped_config1(tmp_path)
    os.remove(str(d / "ref.fa.gz.gzi"))
    cli.main(["diploid", str(tmp_path / "wd"), str(d / "hap1.bam"), str(d / "hap2.bam"), str(d / "ref.fa.gz")])
    assert not os.path.exists(tmp_path / "wd" / "variants.vcf")
    assert ".gzi" in caplog.text and "ref.fa.gz.gzi" in caplog.text


@pytest.mark.parametrize("mode", ["haploid", "diploid"])
def test_cli_writes_no_vcf_over_a_damaged_member(tmp_path, monkeypatch, mode):
    from svim_asm_amd import cli
    helpers.oracle_backed_device(monkeypatch)
    d = bgzipped_config1(tmp_path, level=6)
    n = len(member_spans(str(d / "ref.fa.gz"))) - 1
    for k in range(n):  # every member with data: whatever the alleles touch
        damage_member(str(d / "ref.fa.gz"), k, "crc")
    bams = [str(d / "hap1.bam")] + ([str(d / "hap2.bam")] if mode == "diploid" else [])
    with pytest.raises(ValueError):
        cli.main([mode, str(tmp_path / "wd")] + bams + [str(d / "ref.fa.gz")])
    assert not os.path.exists(tmp_path / "wd" / "variants.vcf")


def test_cohort_with_a_bgzipped_genome(tmp_path, monkeypatch):
    from svim_asm_amd import cli, cohort
    helpers.oracle_backed_device(monkeypatch)
    monkeypatch.setattr(cli, "_warm_device", lambda device: None)
    d = bgzipped_config1(tmp_path)
    rows = [("s1", "hap1.bam", "hap2.bam"), ("s2", "hap1.bam", "hap2.bam")]
    manifest = tmp_path / "cohort.tsv"
    manifest.write_text("".join("%s %s %s\n" % (tmp_path / wd, d / a, d / b) for wd, a, b in rows))
    assert cohort.main(["diploid", str(manifest), str(d / "ref.fa.gz")]) == 0
    for wd, _, _ in rows:
        got = "".join(l for l in open(tmp_path / wd / "variants.vcf") if not l.startswith("##fileDate="))
        assert got == open(os.path.join(GOLD, "config1", "diploid_default.vcf")).read()


def test_writer_round_trip(tmp_path):
    names, seqs = random_genome(11)
    path = fasta.write_bgzf_fasta(str(tmp_path / "w.fa.gz"), names, seqs, line=70, level=1, member_size=0xFF00, threads=2)
    assert fasta.bgzf_kind(path) == "bgzf"
    z = fasta.FastaFile(path)
    for n, s in zip(names, seqs):
        assert z.fetch_bytes(n) == s
    # the file is an ordinary gzip stream of the FASTA text
    text = zlib.decompress(open(path, "rb").read(), 31)
    assert text.startswith(b">ctg0\n")


def test_concatenated_bgzip_files_with_an_empty_member_inside(small, tmp_path):
    """Two bgzip files joined (`cat a.gz b.gz`): the first one's end-of-file marker is an empty member in the middle,
    and its .gzi entry shares the uncompressed offset of the member behind it — accepted, and read as one stream."""
    _, plain, _, names = small
    text = open(plain, "rb").read()
    cut = len(text) // 2
    a, b = str(tmp_path / "a.fa"), str(tmp_path / "b.fa")
    open(a, "wb").write(text[:cut])
    open(b, "wb").write(text[cut:])
    for p in (a, b):
        open(p + ".fai", "w").close()
        fasta.bgzip_fasta(p, p + ".gz", level=6, member_size=7000, gzi_end=True)
    ca, ua = fasta.read_gzi(a + ".gz.gzi")
    cb, ub = fasta.read_gzi(b + ".gz.gzi")
    size_a = os.path.getsize(a + ".gz")
    joined = str(tmp_path / "j.fa.gz")
    open(joined, "wb").write(open(a + ".gz", "rb").read() + open(b + ".gz", "rb").read())
    pairs = list(zip(ca.tolist(), ua.tolist())) + [(size_a, cut)] + [(c + size_a, u + cut) for c, u in zip(cb.tolist(), ub.tolist())]
    assert pairs[len(ca) - 1][1] == pairs[len(ca)][1] == cut  # (the marker's entry and the next member's share it)
    write_gzi(joined + ".gzi", pairs)
    shutil.copy(plain + ".fai", joined + ".fai")
    p, z = fasta.FastaFile(plain), fasta.FastaFile(joined)
    for c in names:
        assert z.fetch(c) == p.fetch(c)
