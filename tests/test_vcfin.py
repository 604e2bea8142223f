"""The VCF reader (include/svx_vcfin.h, svim_asm_amd/vcfin.py) without a GPU: the round trip through the product's own
writer, the golden VCFs of the reference against the plain-Python parser of tests/compare_restatement.py, hand-written
lines for every class, edge and refusal, and plain text against BGZF."""
import gzip
import os

import pytest

from svim_asm_amd import bamio, vcfin
from svim_asm_amd.table import CandidateTable, T_DEL, T_INS
from tests import compare_restatement as R, helpers

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config1")
REF = os.path.join(GOLD, "ref.fa")
CONTIGS, LENGTHS = [], []
for _line in open(REF + ".fai"):
    CONTIGS.append(_line.split("\t")[0])
    LENGTHS.append(int(_line.split("\t")[1]))
LEN_OF = dict(zip(CONTIGS, LENGTHS))
HEADER = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n"
C0 = CONTIGS[0]


def rows_of(rec):
    """The reader's rows as the restatement's dictionaries."""
    t = rec.table
    out = []
    for i in range(len(t)):
        ins = t.type[i] == T_INS
        out.append({"class": "INS" if ins else "DEL", "contig": t.contigs[int(t.dc[i] if ins else t.sc[i])],
                    "start": int(t.ds[i] if ins else t.ss[i]), "end": int(t.de[i] if ins else t.se[i]),
                    "seq": bytes(t.seqs[int(t.q_off[i]):int(t.q_off[i] + t.q_len[i])]).decode() if ins else "", "gt": int(t.gt[i]),
                    "line": int(rec.line_no[i]), "id": rec.ids[i], "text": rec.lines[i]})
    return out


def same_as_restatement(path, **kw):
    rec = vcfin.read_vcf(path, CONTIGS, LENGTHS, **kw)
    want = R.parse_vcf(path, LEN_OF, **kw)
    assert rec.counts == R.counts_of(want)
    assert rec.n_lines == len(want["records"])
    keys = ("class", "contig", "start", "end", "seq", "gt", "line", "id", "text")
    assert rows_of(rec) == [{k: r[k] for k in keys} for r in R.rows_of(want)]
    assert rec.header == want["header"]
    return rec


def write(tmp_path, body, header=HEADER, name="t.vcf", eol="\n"):
    p = tmp_path / name
    p.write_bytes((header + body).replace("\n", eol).encode())
    return str(p)


def bgzip(src, dst, member_size):
    data = open(src, "rb").read()
    with open(dst, "wb") as fh:
        for at in range(0, len(data), member_size):
            fh.write(bamio._bgzf_member(memoryview(data)[at:at + member_size], 6))
        fh.write(bamio._BGZF_EOF)
    return dst


# ------------------------------------------------------------------------------------------------- golden files
@pytest.mark.parametrize("name", ["diploid_default.vcf", "haploid_default.vcf", "diploid_symbolic_dup_as_ins.vcf", "diploid_tolerances.vcf"])
def test_golden_vcfs_of_the_reference_equal_the_restatement(name):
    rec = same_as_restatement(os.path.join(GOLD, name))
    assert rec.counts["DEL"] > 0 and rec.n_lines == sum(rec.counts.values())
    if "symbolic" in name:
        assert rec.counts["INS"] == 0 and rec.counts["unresolved"] > 0


@pytest.mark.parametrize("extra", [(), ("--symbolic_alleles",)])
def test_round_trip_through_the_products_writer(tmp_path, monkeypatch, extra):
    """svim-asm diploid --keep_candidates: reading variants.vcf back gives the DEL and INS rows of candidates.svxt."""
    from svim_asm_amd import cli
    helpers.oracle_backed_device(monkeypatch)
    wd = tmp_path / "wd"
    cli.main(["diploid", str(wd), os.path.join(GOLD, "hap1.bam"), os.path.join(GOLD, "hap2.bam"), REF, "--keep_candidates"] + list(extra))
    t = CandidateTable.from_wire(open(wd / "candidates.svxt", "rb").read())
    bits = {"1/0": 1, "0/1": 2, "1/1": 3}
    want = []
    for i in range(len(t)):
        if t.type[i] == T_DEL:
            want.append(("DEL", t.contigs[int(t.sc[i])], int(t.ss[i]), int(t.se[i]), "", bits[t.genotypes[int(t.gt[i])]]))
        elif t.type[i] == T_INS and not extra:
            want.append(("INS", t.contigs[int(t.dc[i])], int(t.ds[i]), int(t.de[i]),
                         bytes(t.seqs[int(t.q_off[i]):int(t.q_off[i] + t.q_len[i])]).decode().upper(), bits[t.genotypes[int(t.gt[i])]]))
    rec = vcfin.read_vcf(str(wd / "variants.vcf"), CONTIGS, LENGTHS)
    got = [(r["class"], r["contig"], r["start"], r["end"], r["seq"], r["gt"]) for r in rows_of(rec)]
    assert sorted(got) == sorted(want) and len(want) > 50
    n_ins = int((t.type == T_INS).sum())
    assert n_ins > 0
    assert rec.counts["unresolved"] == (n_ins if extra else 0)
    assert rec.counts["INS"] == (0 if extra else n_ins)


# ------------------------------------------------------------------------------------------------- hand-written lines
BODY = "".join([
    C0 + "\t1\ta\tACGT\t.\t.\tPASS\t.\tGT\t1/1\t0/0\n",                      # start 0: POS 1, empty shared prefix -> DEL [0, 4)
    C0 + "\t10\tb\tACGT\tA\t.\tPASS\tEND=999;SVLEN=5\tGT\t0|1\t0/0\n",       # prefix 1 -> DEL [10, 13); END / SVLEN ignored
    C0 + "\t10\tc\tACGTT\tacg\t.\tq10\t.\tGT\t1|0\t0/0\n",                   # prefix 3 without regard to case -> DEL [12, 14)
    C0 + "\t1\td\t.\tTTT\t.\tPASS\t.\tGT\t1\t0\n",                           # INS at 0 of TTT; a one-allele GT sets both
    C0 + "\t20\te\tA\tAcgN\t.\t.\t.\tGT:DP\t./1:7\t0/0:3\n",                 # prefix 1 -> INS at 20 of CGN
    C0 + "\t20\tf\tACG\tACGTT\t.\tPASS\t.\tGT\t1/1\t0/0\n",                  # prefix 3 -> INS at 22 of TT
    C0 + "\t30\tg\tA\tC\t.\tPASS\t.\tGT\t1/1\t0/0\n",                        # SNV: complex
    C0 + "\t30\th\tAC\tAC\t.\tPASS\t.\tGT\t1/1\t0/0\n",                      # REF == ALT: complex
    C0 + "\t30\ti\tACG\tAT\t.\tPASS\t.\tGT\t1/1\t0/0\n",                     # neither a prefix of the other: complex
    C0 + "\t30\tj\tA\tAT,ATT\t.\tPASS\t.\tGT\t1/2\t0/0\n",                   # multiallelic
    C0 + "\t40\tk\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=100;SVLEN=-55\tGT\t0/1\t1/1\n",   # symbolic: [45, 100)
    C0 + "\t40\tl\tN\t<DEL>\t.\tPASS\tEND=100;SVLEN=55\tGT\t0/1\t1/1\n",     # SVLEN as a positive magnitude: [45, 100)
    C0 + "\t40\tm\tN\t<DEL>\t.\tPASS\tEND=100\tGT\t0/1\t1/1\n",              # no SVLEN: [40, 100)
    C0 + "\t40\tn\tN\t<INS>\t.\tPASS\tEND=40;SVLEN=60\tGT\t0/1\t0/0\n",      # unresolved
    C0 + "\t40\to\tN\t<INV>\t.\tPASS\tEND=90\tGT\t0/1\t0/0\n",               # other
    C0 + "\t40\tp\tN\t<DUP:TANDEM>\t.\tPASS\tEND=90\tGT\t0/1\t0/0\n",        # other
    C0 + "\t40\tq\tN\tN[" + C0 + ":77[\t.\tPASS\t.\tGT\t0/1\t0/0\n",         # breakend: other
    C0 + "\t50\tr\tACGT\tA\t.\tPASS\t.\tGT\t0/0\t1/1\n",                     # not carried by S1
    C0 + "\t50\ts\tACGT\tA\t.\tPASS\t.\tGT\t./.\t1/1\n",                     # not carried by S1
    C0 + "\t50\tt\tACGT\tA\t.\tPASS\t.\tGT\t0/.\t0/1\n",                     # not carried by S1
    "\n",                                                                   # an empty line
    C0 + "\t60\tu\tACGT\tA\t.\tPASS\t.\n",                                   # 8 columns in a file with samples: refused below
])
LINES = BODY.split("\n")[:-1]


def body(*ids):
    return "".join(l + "\n" for l in LINES if not l or l.split("\t")[2] in ids)


ALL_BUT_U = [l.split("\t")[2] for l in LINES if l and l.split("\t")[2] != "u"]


def test_every_class_and_edge_by_hand(tmp_path):
    p = write(tmp_path, body(*ALL_BUT_U))
    rec = same_as_restatement(p)
    assert rec.counts == {"DEL": 6, "INS": 3, "multiallelic": 1, "complex": 3, "unresolved": 1, "other": 3, "not_carried": 3, "filtered": 0}
    got = [(r["id"], r["class"], r["start"], r["end"], r["seq"], r["gt"], r["line"]) for r in rows_of(rec)]
    assert got == [("a", "DEL", 0, 4, "", 3, 3), ("b", "DEL", 10, 13, "", 2, 4), ("c", "DEL", 12, 14, "", 1, 5), ("d", "INS", 0, 3, "TTT", 3, 6),
                   ("e", "INS", 20, 23, "CGN", 2, 7), ("f", "INS", 22, 24, "TT", 3, 8), ("k", "DEL", 45, 100, "", 2, 13),
                   ("l", "DEL", 45, 100, "", 2, 14), ("m", "DEL", 40, 100, "", 2, 15)]
    assert rec.header == HEADER.encode() and rec.lines[0] == LINES[0].encode()
    # the second sample by name; --passonly
    s2 = same_as_restatement(p, sample="S2")
    assert [r["id"] for r in rows_of(s2)] == ["k", "l", "m", "r", "s", "t"] and s2.counts["not_carried"] == 6
    assert [r["gt"] for r in rows_of(s2)] == [3, 3, 3, 3, 3, 2]
    po = same_as_restatement(p, passonly=True)
    assert po.counts["filtered"] == 1 and "c" not in [r["id"] for r in rows_of(po)] and "b" in [r["id"] for r in rows_of(po)]


def test_crlf_and_a_last_line_without_its_end(tmp_path):
    plain = vcfin.read_vcf(write(tmp_path, body(*ALL_BUT_U)), CONTIGS, LENGTHS)
    crlf = same_as_restatement(write(tmp_path, body(*ALL_BUT_U), name="crlf.vcf", eol="\r\n"))
    assert rows_of(crlf) == rows_of(plain) and crlf.counts == plain.counts
    p = tmp_path / "open.vcf"
    p.write_bytes((HEADER + body(*ALL_BUT_U)).encode()[:-1])
    assert rows_of(same_as_restatement(str(p))) == rows_of(plain)


def test_sites_only_file_every_record_carried_genotype_unknown(tmp_path):
    header = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    rec = same_as_restatement(write(tmp_path, body("u") + C0 + "\t70\tv\tA\tACC\t.\t.\t.\n", header=header))
    assert [(r["id"], r["class"], r["gt"]) for r in rows_of(rec)] == [("u", "DEL", 0), ("v", "INS", 0)]
    with pytest.raises(vcfin.VcfFormatError, match=r"line 2: .*no sample 'S1'"):
        vcfin.read_vcf(write(tmp_path, body("u"), header=header), CONTIGS, LENGTHS, sample="S1")


REFUSALS = [
    (C0 + "\t60\tu\tACGT\tA\t.\tPASS\n", "fewer than 8 columns"),
    (C0 + "\t0\tu\tACGT\tA\t.\tPASS\t.\tGT\t1/1\t0/0\n", "POS"),
    (C0 + "\t-5\tu\tACGT\tA\t.\tPASS\t.\tGT\t1/1\t0/0\n", "POS"),
    (C0 + "\t6x\tu\tACGT\tA\t.\tPASS\t.\tGT\t1/1\t0/0\n", "POS"),
    ("chrNowhere\t60\tu\tACGT\tA\t.\tPASS\t.\tGT\t1/1\t0/0\n", "chrNowhere"),
    (C0 + "\t%d\tu\tA\tAT\t.\tPASS\t.\tGT\t1/1\t0/0\n" % (LENGTHS[0] + 1), "beyond the length"),
    (C0 + "\t%d\tu\tACGT\tA\t.\tPASS\t.\tGT\t1/1\t0/0\n" % (LENGTHS[0] - 1), "beyond the length"),
    (C0 + "\t40\tu\tN\t<DEL>\t.\tPASS\tEND=%d\tGT\t1/1\t0/0\n" % (LENGTHS[0] + 1), "beyond the length"),
    (C0 + "\t40\tu\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL\tGT\t1/1\t0/0\n", "END"),
    (C0 + "\t40\tu\tN\t<DEL>\t.\tPASS\tEND=40\tGT\t1/1\t0/0\n", "empty interval"),
    (C0 + "\t40\tu\tN\t<DEL>\t.\tPASS\tEND=90;SVLEN=0\tGT\t1/1\t0/0\n", "empty interval"),
    (C0 + "\t60\tu\tACGT\tA\t.\tPASS\t.\n", "no column for the sample"),
    (C0 + "\t60\tu\tACGT\tA\t.\tPASS\t.\tGT\t1/1\n", "no column for the sample"),
]


@pytest.mark.parametrize("line,what", REFUSALS)
def test_refusals_name_the_line(tmp_path, line, what):
    p = write(tmp_path, body("a", "b") + "\n" + line + body("f"))  # (body() ends with the empty line: two of them in front)
    with pytest.raises(vcfin.VcfFormatError, match=r"t\.vcf: line 7: .*" + what):
        vcfin.read_vcf(p, CONTIGS, LENGTHS, sample="S2" if line.endswith("1/1\n") else None)
    with pytest.raises(R.Refused) as e:
        R.parse_vcf(p, LEN_OF, sample="S2" if line.endswith("1/1\n") else None)
    assert e.value.line == 7


def test_header_refusals(tmp_path):
    with pytest.raises(vcfin.VcfFormatError, match="line 2: no #CHROM line"):
        vcfin.read_vcf(write(tmp_path, body("a"), header="##fileformat=VCFv4.2\n"), CONTIGS, LENGTHS)
    with pytest.raises(vcfin.VcfFormatError, match="no #CHROM line"):
        vcfin.read_vcf(write(tmp_path, "", header="##fileformat=VCFv4.2\n"), CONTIGS, LENGTHS)
    with pytest.raises(vcfin.VcfFormatError, match="no #CHROM line"):
        vcfin.read_vcf(write(tmp_path, "", header=""), CONTIGS, LENGTHS)
    with pytest.raises(vcfin.VcfFormatError, match="line 2: .*no sample 'S3'"):
        vcfin.read_vcf(write(tmp_path, body("a")), CONTIGS, LENGTHS, sample="S3")
    with pytest.raises(vcfin.VcfFormatError, match="cannot open"):
        vcfin.read_vcf(str(tmp_path / "missing.vcf"), CONTIGS, LENGTHS)
    empty = vcfin.read_vcf(write(tmp_path, ""), CONTIGS, LENGTHS)
    assert len(empty) == 0 and empty.n_lines == 0 and empty.header == HEADER.encode()


# ------------------------------------------------------------------------------------------------- BGZF
def data_members(path):
    """ISIZE of every BGZF member of the file that holds data (the empty end-of-file member left out)."""
    raw, at, sizes = open(path, "rb").read(), 0, []
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 16] == b"BC\x02\x00"
        bsize = int.from_bytes(raw[at + 16:at + 18], "little") + 1
        sizes.append(int.from_bytes(raw[at + bsize - 4:at + bsize], "little"))
        at += bsize
    assert sizes[-1] == 0
    return sizes[:-1]


@pytest.mark.parametrize("which,member_size,n_members", [("small", 0xFF00, 1), ("golden", 0xFF00, 2), ("golden", 4096, 18), ("small", 23, None)])
def test_plain_against_bgzf(tmp_path, which, member_size, n_members):
    """ONE data member (the small hand-written file in a member of bgzip's size), two and eighteen (the golden file),
    and members shorter than the shortest record, so that every record's line is split across members."""
    src = os.path.join(GOLD, "diploid_default.vcf") if which == "golden" else write(tmp_path, body(*ALL_BUT_U))
    plain = vcfin.read_vcf(src, CONTIGS, LENGTHS)
    gz = bgzip(src, str(tmp_path / "x.vcf.gz"), member_size)
    sizes = data_members(gz)
    assert sum(sizes) == os.path.getsize(src) and len(sizes) == (n_members if n_members else -(-os.path.getsize(src) // member_size))
    if n_members is None:
        assert min(len(l) for l in LINES if l) > member_size  # no record's line fits into one member
    packed = same_as_restatement(gz)
    assert rows_of(packed) == rows_of(plain) and packed.counts == plain.counts and packed.header == plain.header
    assert packed.lines == plain.lines and len(plain) > 0


def test_gzip_that_is_not_bgzf_is_refused_and_damage_is_named(tmp_path):
    src = write(tmp_path, body(*ALL_BUT_U))
    p = tmp_path / "plain.vcf.gz"
    p.write_bytes(gzip.compress(open(src, "rb").read()))
    with pytest.raises(vcfin.VcfFormatError, match="not BGZF.*bgzip"):
        vcfin.read_vcf(str(p), CONTIGS, LENGTHS)
    good = bytearray(open(bgzip(src, str(tmp_path / "x.vcf.gz"), 300), "rb").read())
    good[40] ^= 0x55  # inside the first member's payload
    (tmp_path / "bad.vcf.gz").write_bytes(bytes(good))
    with pytest.raises(vcfin.VcfFormatError, match="does not inflate or fails its CRC32|BGZF"):
        vcfin.read_vcf(str(tmp_path / "bad.vcf.gz"), CONTIGS, LENGTHS)
