"""The second VCF reader (svx_vcfin_open_alleles in include/svx_vcfin.h, vcfin.read_alleles) without a GPU: hand-written
lines for the trimming rule, every class and count and `phased`; lower case, "\\r\\n" and BGZF input; every refusal with
its line number; the fixture's golden VCFs — all against the plain-Python parser of tests/replay_restatement.py; and
svx_vcfin_open on the same files still gives what it gave."""
import os

import pytest

from svim_asm_amd import vcfin
from tests import replay_restatement as RR
from tests import test_vcfin as V

C0, CONTIGS, LENGTHS, LEN_OF = V.C0, V.CONTIGS, V.LENGTHS, V.LEN_OF
END = LENGTHS[0]

BODY = "".join([
    C0 + "\t30\tsnv\tA\tC\t.\tPASS\t.\tGT\t0|1\t0/0\n",                     # (29, 1, C), phased
    C0 + "\t30\tmnp\tACG\tTCA\t.\tPASS\t.\tGT\t0/1\t0/0\n",                 # no prefix, no suffix: (29, 3, TCA), not phased
    C0 + "\t30\tmid\tACG\tATG\t.\tPASS\t.\tGT\t1/1\t0/0\n",                 # prefix 1, suffix 1: (30, 1, T); both alleles 1: phased
    C0 + "\t10\tdel\tACGT\tA\t.\tPASS\t.\tGT\t1\t0\n",                      # prefix 1: (10, 3, ""); one allele: phased, both bits
    C0 + "\t10\tins\tA\tAcgN\t.\t.\t.\tGT:DP\t./1:7\t0/0:3\n",              # (10, 0, CGN), upper case; ./1: not phased
    C0 + "\t10\trun\tCAAA\tCAA\t.\tPASS\t.\tGT\t1|.\t0/0\n",                # prefix first: 3, then no suffix left: (12, 1, ""); 1|.: phased
    C0 + "\t10\trep\tcaTg\tCGGG\t.\tq10\t.\tGT\t1|0\t0/0\n",                # case ignored: prefix 1, suffix 1: (10, 2, GG)
    C0 + "\t1\tall\tACGT\t.\t.\tPASS\t.\tGT\t1/1\t0/0\n",                   # ALT "." is the empty string: (0, 4, "")
    C0 + "\t1\tfront\t.\tTTT\t.\tPASS\t.\tGT\t1/1\t0/0\n",                  # REF ".": (0, 0, TTT)
    C0 + "\t30\tsame\tAc\taC\t.\tPASS\t.\tGT\t1/1\t0/0\n",                  # no_change (before the genotype is looked at)
    C0 + "\t30\tsame0\tAC\tAC\t.\tPASS\t.\tGT\t0/0\t0/0\n",                 # no_change
    C0 + "\t30\tmulti\tA\tAT,ATT\t.\tPASS\t.\tGT\t1/2\t0/0\n",              # multiallelic
    C0 + "\t40\tsym\tN\t<DEL>\t.\tPASS\tEND=100\tGT\t0/1\t1/1\n",           # symbolic_or_other
    C0 + "\t40\tsym2\tN\t<INS>\t.\tPASS\t.\tGT\t0/1\t1/1\n",
    C0 + "\t40\tbnd\tN\tN[" + C0 + ":77[\t.\tPASS\t.\tGT\t0/1\t0/0\n",
    C0 + "\t40\tstar\tA\t*\t.\tPASS\t.\tGT\t0/1\t0/0\n",
    C0 + "\t50\tnc\tA\tC\t.\tPASS\t.\tGT\t0/0\t1/1\n",                      # not carried by S1
    C0 + "\t50\tnc2\tA\tC\t.\tPASS\t.\tGT\t./.\t1|1\n",
    "\n",
    C0 + "\t%d\tlast\tAA\tG\t.\tPASS\t.\tGT\t0|1\t0/0\n" % (END - 1),       # REF reaches the contig's end
])
KEYS = ("contig", "start", "ref_len", "alt", "pos", "ref_text", "gt", "phased", "line", "id", "text")


def rows_of(a):
    out = []
    for i in range(len(a)):
        out.append({"contig": CONTIGS[int(a.contig[i])], "start": int(a.start[i]), "ref_len": int(a.ref_len[i]),
                    "alt": bytes(a.alts[int(a.alt_off[i]):int(a.alt_off[i]) + int(a.alt_len[i])]).decode(), "pos": int(a.pos[i]),
                    "ref_text": a.text[int(a.ref_off[i]):int(a.ref_off[i]) + int(a.ref_text_len[i])].decode("latin-1"),
                    "gt": int(a.gt[i]), "phased": int(a.phased[i]), "line": int(a.line_no[i]),
                    "id": a.text[int(a.id_off[i]):int(a.id_off[i]) + int(a.id_len[i])].decode("latin-1"), "text": a.line(i)})
    return out


def same_as_restatement(path, **kw):
    got = vcfin.read_alleles(path, CONTIGS, LENGTHS, **kw)
    want = RR.parse_alleles(path, LEN_OF, **kw)
    assert got.counts == want["counts"] and got.n_lines == want["n_lines"] == sum(got.counts.values())
    assert rows_of(got) == [{k: r[k] for k in KEYS} for r in want["rows"]]
    assert got.header == want["header"]
    for threads in (1, 3):
        again = vcfin.read_alleles(path, CONTIGS, LENGTHS, threads=threads, **kw)
        assert rows_of(again) == rows_of(got) and again.counts == got.counts
    return got


def test_hand_written_lines(tmp_path):
    got = same_as_restatement(V.write(tmp_path, BODY))
    rows = {r["id"]: (r["start"], r["ref_len"], r["alt"], r["gt"], r["phased"]) for r in rows_of(got)}
    assert rows == {"snv": (29, 1, "C", 2, 1), "mnp": (29, 3, "TCA", 2, 0), "mid": (30, 1, "T", 3, 1), "del": (10, 3, "", 3, 1),
                    "ins": (10, 0, "CGN", 2, 0), "run": (12, 1, "", 1, 1), "rep": (10, 2, "GG", 1, 1), "all": (0, 4, "", 3, 1),
                    "front": (0, 0, "TTT", 3, 1), "last": (END - 2, 2, "G", 2, 1)}
    assert got.counts == {"rows": 10, "multiallelic": 1, "symbolic_or_other": 4, "not_carried": 2, "filtered": 0, "no_change": 2}
    assert [r["ref_text"] for r in rows_of(got)][:7] == ["A", "ACG", "ACG", "ACGT", "A", "CAAA", "caTg"]
    assert [r["pos"] for r in rows_of(got)][:7] == [29, 29, 29, 9, 9, 9, 9]


@pytest.mark.parametrize("gt,bits,phased", [("0|1", 2, 1), ("0/1", 2, 0), ("1/1", 3, 1), ("1", 3, 1), ("./1", 2, 0), ("1|.", 1, 1),
                                            ("1|0", 1, 1), ("1/0", 1, 0), ("1|1", 3, 1), ("1/.", 1, 0)])
def test_phased(tmp_path, gt, bits, phased):
    got = same_as_restatement(V.write(tmp_path, C0 + "\t30\tx\tA\tC\t.\tPASS\t.\tGT:DP\t%s:3\t0/0:1\n" % gt))
    assert (got.gt.tolist(), got.phased.tolist()) == ([bits], [phased])


def test_the_other_sample_passonly_and_files_without_samples(tmp_path):
    path = V.write(tmp_path, BODY)
    s2 = same_as_restatement(path, sample="S2")
    assert [r["id"] for r in rows_of(s2)] == ["nc", "nc2"] and s2.gt.tolist() == [3, 3] and s2.phased.tolist() == [1, 1]
    assert s2.counts["not_carried"] == 10
    po = same_as_restatement(path, passonly=True)
    assert po.counts["filtered"] == 1 and "rep" not in [r["id"] for r in rows_of(po)]
    bare = "\n".join("\t".join(l.split("\t")[:8]) for l in BODY.split("\n") if l) + "\n"
    nos = same_as_restatement(V.write(tmp_path, bare, header=V.HEADER.replace("\tFORMAT\tS1\tS2", ""), name="bare.vcf"))
    assert nos.counts["not_carried"] == 0 and nos.counts["rows"] == 12 and set(nos.gt.tolist()) == {0} and set(nos.phased.tolist()) == {1}
    nogt = same_as_restatement(V.write(tmp_path, C0 + "\t30\tx\tA\tC\t.\tPASS\t.\tDP\t3\t1\n", name="nogt.vcf"))
    assert nogt.gt.tolist() == [0] and nogt.phased.tolist() == [1]


def test_crlf_and_bgzf(tmp_path):
    plain = V.write(tmp_path, BODY)
    want = rows_of(vcfin.read_alleles(plain, CONTIGS, LENGTHS))
    crlf = same_as_restatement(V.write(tmp_path, BODY, name="crlf.vcf", eol="\r\n"))
    assert [{k: v for k, v in r.items()} for r in rows_of(crlf)] == want
    for size in (0xFF00, 23):
        gz = same_as_restatement(V.bgzip(plain, str(tmp_path / ("m%d.vcf.gz" % size)), size))
        assert rows_of(gz) == want


@pytest.mark.parametrize("name", ["diploid_default.vcf", "haploid_default.vcf", "diploid_symbolic_dup_as_ins.vcf"])
def test_golden_vcfs(name):
    got = same_as_restatement(os.path.join(V.GOLD, name))
    assert got.n_lines > 0 and (got.counts["rows"] > 0) == ("symbolic" not in name)


@pytest.mark.parametrize("line,word", [
    (C0 + "\t60\tu\tACGT\tA\t.\tPASS\n", "fewer than 8 columns"),
    (C0 + "\t0\tu\tA\tC\t.\tPASS\t.\tGT\t1/1\t0/0\n", "POS"),
    (C0 + "\tx\tu\tA\tC\t.\tPASS\t.\tGT\t1/1\t0/0\n", "POS"),
    ("nowhere\t5\tu\tA\tC\t.\tPASS\t.\tGT\t1/1\t0/0\n", "nowhere"),
    (C0 + "\t%d\tu\tA\tC\t.\tPASS\t.\tGT\t1/1\t0/0\n" % (END + 1), "beyond"),
    (C0 + "\t%d\tu\tAAA\tC\t.\tPASS\t.\tGT\t1/1\t0/0\n" % (END - 1), "REF ends at %d" % (END + 1)),
    (C0 + "\t60\tu\tA\tC\t.\tPASS\t.\tGT\n", "no column for the sample"),
])
def test_refusals_name_the_line(tmp_path, line, word):
    good = C0 + "\t30\tsnv\tA\tC\t.\tPASS\t.\tGT\t0|1\t0/0\n"
    path = V.write(tmp_path, good + "\n" + good + line + good)
    with pytest.raises(vcfin.VcfFormatError) as ei:
        vcfin.read_alleles(path, CONTIGS, LENGTHS)
    assert "line 6:" in str(ei.value) and word in str(ei.value), str(ei.value)
    with pytest.raises(RR.Refused, match="line 6:"):
        RR.parse_alleles(path, LEN_OF)


def test_header_refusals_and_a_missing_sample(tmp_path):
    with pytest.raises(vcfin.VcfFormatError, match="no sample 'S9'"):
        vcfin.read_alleles(V.write(tmp_path, BODY), CONTIGS, LENGTHS, sample="S9")
    with pytest.raises(vcfin.VcfFormatError, match="line 1: no #CHROM"):
        vcfin.read_alleles(V.write(tmp_path, BODY, header="", name="bare.vcf"), CONTIGS, LENGTHS)
    with pytest.raises(vcfin.VcfFormatError, match="cannot open"):
        vcfin.read_alleles(str(tmp_path / "none.vcf"), CONTIGS, LENGTHS)


def test_the_first_reader_still_gives_what_it_gave(tmp_path):
    for path in (V.write(tmp_path, BODY), os.path.join(V.GOLD, "diploid_default.vcf")):
        V.same_as_restatement(path)
    rec = vcfin.read_vcf(V.write(tmp_path, BODY), CONTIGS, LENGTHS)
    assert rec.counts["DEL"] + rec.counts["INS"] == len(rec) == 6 and rec.counts["complex"] == 9 and rec.n_lines == 19
    # a handle is of one kind
    import ctypes as C
    from svim_asm_amd import _lib
    lib = _lib.load()
    names = (C.c_char_p * len(CONTIGS))(*[c.encode() for c in CONTIGS])
    import numpy as np
    lengths = np.array(LENGTHS, np.int64)
    path = V.write(tmp_path, BODY).encode()
    for opener, good, bad, box in ((lib.svx_vcfin_open_alleles, lib.svx_vcfin_get_alleles, lib.svx_vcfin_get_columns, _lib.VcfinColumns()),
                                   (lib.svx_vcfin_open, lib.svx_vcfin_get_columns, lib.svx_vcfin_get_alleles, _lib.VcfinAlleles())):
        h, err = C.c_void_p(), C.create_string_buffer(256)
        assert opener(path, len(CONTIGS), C.cast(names, C.c_void_p), lengths.ctypes.data, None, 0, 1, C.byref(h), err, 256) == 0
        assert bad(h, C.byref(box)) == _lib.SVX_E_INVALID
        lib.svx_vcfin_close(h)
