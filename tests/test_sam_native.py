"""The native SAM reader (csrc/svx_sam.cpp, include/svx_sam.h) on the CPU: its columns against the native BAM reader's
on the sorted BAM of the same records, the order definition, the host CIGAR-text parser against the pure-Python oracle
of tests/sam_text_writer.py, malformed files, the base alphabet and line ends."""
import os

import numpy as np
import pytest

from svim_asm_amd import _lib, bamio
from tests import sam_text_writer as stw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFS, LENS = ("chr1", "chr2", "chrM"), (100000, 50000, 16000)


def _sam(tmp_path, lines, name="t.sam", **kw):
    return stw.write_sam(str(tmp_path / name), REFS, LENS, lines, **kw)


def _line(q, flag, rname, pos0, cigar="10M", seq="ACGTACGTAC", aux=(), mapq=60):
    return stw.record_line(q, flag, rname, pos0, mapq, cigar, seq, aux)


# ------------------------------------------------------------------ columns against the BAM reader
def _compare_with_bam(bam_path, sam_path):
    b = bamio.AlignmentFile(bam_path, reader="native")
    s = bamio.AlignmentFile(sam_path)
    assert s.is_sam and not b.is_sam
    assert s.references == b.references and s.lengths == b.lengths
    b.load()
    s.load()
    assert len(s) == len(b)
    for k in ("tid", "pos", "flag", "mapq", "l_seq", "ref_len", "n_cig"):
        assert np.array_equal(s._cols[k], b._cols[k]), k
    assert np.array_equal(s._cigar, b._cigar) and np.array_equal(s._cig_off, b._cig_off)
    assert s.blocks_inflated == 0 and s.blocks_spanned == 0 and s.check_index() and s.contig_spans() is None
    for i in range(len(b)):
        rb, rs = b.record(i), s.record(i)
        assert rs.query_name == rb.query_name
        assert stw.aux_values(rs._tags_raw) == stw.aux_values(rb._tags_raw)
        assert rs._sa == rb._sa and rs._sa_absent == rb._sa_absent
        assert rs._parse_tags().keys() == rb._parse_tags().keys()
    # voffset: the byte offset of the record's line
    data = open(sam_path, "rb").read()
    for i in range(len(s)):
        o = int(s._cols["voffset"][i])
        assert (o == 0 or data[o - 1:o] == b"\n") and data[o:].startswith(s.record(i).query_name.encode() + b"\t")
    # bases
    rec = np.arange(len(b), dtype=np.uint32)
    l_seq = b._cols["l_seq"]
    for lo, hi in ((0, 50), (17, 4000), (l_seq // 2, l_seq // 2 + 333), (np.maximum(l_seq - 40, 0), l_seq + 10)):
        lo, hi = np.broadcast_to(lo, rec.shape), np.broadcast_to(hi, rec.shape)
        assert s.sequence_slices(rec, lo, hi) == b.sequence_slices(rec, lo, hi)
    return s, b


@pytest.mark.parametrize("name", ["hap1", "hap2"])
def test_columns_equal_the_bam_readers_config1(tmp_path, name):
    bam = os.path.join(GOLD, "config1", name + ".bam")
    _compare_with_bam(bam, stw.bam_as_sam(bam, str(tmp_path / "x.sam"), shuffle_seed=11))


def test_columns_equal_the_bam_readers_synthetic_with_splits(tmp_path):
    from svim_asm_amd import synth_bam
    contigs = (("chrA", 300000), ("chrB", 200000), ("chrC", 120000))
    _, bams = synth_bam.write_dataset(str(tmp_path), seed=9, contigs=contigs, n_shared=8, n_private=3, median_aln=40000, mean_m=200)
    for k, bam in enumerate(bams):
        s, b = _compare_with_bam(bam, stw.bam_as_sam(bam, bam[:-4] + ".sam", shuffle_seed=k))
        assert (s._sa_off >= 0).any()
        # per-contig loads keep only the asked contigs, in the same order
        t = bamio.AlignmentFile(bam[:-4] + ".sam")
        t.load(["chrC", "chrA"])
        keep = np.isin(b._cols["tid"], [0, 2])
        assert np.array_equal(t._cols["pos"], b._cols["pos"][keep]) and np.array_equal(t._cols["tid"], b._cols["tid"][keep])
        assert [r.query_name for r in t.fetch("chrC")] == [r.query_name for r in b.fetch("chrC")]
        cg, off, pos, tid = t.batch()
        assert len(cg) == int(off[-1]) and len(pos) == len(tid) == keep.sum()


def test_every_aux_type_is_reencoded(tmp_path):
    aux = ["XA:A:q", "Xc:i:-128", "XC:i:255", "Xs:i:-32768", "XS:i:65535", "Xi:i:-2147483648", "XI:i:4294967295", "Xz:i:0",
           "Xf:f:-1.5", "XZ:Z:hello world", "SA:Z:chr2,100,+,5M5S,60,0;", "XH:H:1AE301", "Bc:B:c,-1,2", "BC:B:C,0,255",
           "Bs:B:s,-300,300", "BS:B:S,65535", "Bi:B:i,-70000", "BI:B:I,4000000000,1", "Bf:B:f,0.5,-2.25", "Be:B:C"]
    f = bamio.AlignmentFile(_sam(tmp_path, [_line("r", 0, "chr1", 5, aux=aux)]))
    r = f.record(0)
    tags = r._parse_tags()
    assert tags == {"XA": "q", "Xc": -128, "XC": 255, "Xs": -32768, "XS": 65535, "Xi": -2147483648, "XI": 4294967295, "Xz": 0,
                    "Xf": -1.5, "XZ": "hello world", "SA": "chr2,100,+,5M5S,60,0;", "XH": "1AE301", "Bc": [-1, 2], "BC": [0, 255],
                    "Bs": [-300, 300], "BS": [65535], "Bi": [-70000], "BI": [4000000000, 1], "Bf": [0.5, -2.25], "Be": []}
    assert r.get_tag("SA") == "chr2,100,+,5M5S,60,0;"
    # the smallest integer type that holds the value, unsigned for a value >= 0
    raw = bytes(r._tags_raw)
    for tag, typ in (("Xc", "c"), ("XC", "C"), ("Xs", "s"), ("XS", "S"), ("Xi", "i"), ("XI", "I"), ("Xz", "C")):
        assert raw[raw.index(tag.encode()) + 2:][:1] == typ.encode(), tag


# ------------------------------------------------------------------ the order definition
def test_order_is_tid_pos_strand_then_place_in_the_file(tmp_path):
    lines = [_line("unplaced_b", 4, "*", -1, "*", "*"), _line("c2_late", 0, "chr2", 900), _line("c1_p7_rev_a", 16, "chr1", 7),
             _line("c1_p7_fwd_a", 0, "chr1", 7), _line("unplaced_a", 4, "*", -1, "*", "*"), _line("c1_p7_rev_b", 16, "chr1", 7),
             _line("c1_p7_fwd_b", 0, "chr1", 7), _line("cM", 0, "chrM", 0), _line("c1_p3", 16, "chr1", 3), _line("c2_early", 2048, "chr2", 1)]
    f = bamio.AlignmentFile(_sam(tmp_path, lines, so="queryname"))
    assert [r.query_name for r in f.fetch()] == ["c1_p3", "c1_p7_fwd_a", "c1_p7_fwd_b", "c1_p7_rev_a", "c1_p7_rev_b", "c2_early",
                                                 "c2_late", "cM", "unplaced_b", "unplaced_a"]
    assert f._cols["tid"].tolist() == [0, 0, 0, 0, 0, 1, 1, 2, -1, -1]
    g = bamio.AlignmentFile(_sam(tmp_path, lines, name="u.sam"))
    g.load(["chr2"])
    assert [g.record(i).query_name for i in range(len(g))] == ["c2_early", "c2_late"]


# ------------------------------------------------------------------ the host CIGAR-text parser
def _host(texts, threads=3):
    texts = [t.encode("latin-1") if isinstance(t, str) else t for t in texts]
    off = np.zeros(len(texts) + 1, np.uint64)
    if texts:
        np.cumsum([len(t) for t in texts], out=off[1:])
    got = _lib.cigar_text_parse_host(b"".join(texts), off, threads=threads)
    exp = stw.parse_batch(texts)
    for k in ("status", "cigar_off", "ref_len", "words"):
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), np.asarray(exp[k], dtype=np.int64)), k
    return got


def test_host_parser_every_operator_and_both_ends_of_the_length_range():
    got = _host(["1M1I1D1N1S1H1P1=1X", "268435455M268435455D", "*", "0M", "00042="])
    assert got["words"].tolist()[:9] == [16 | k for k in range(9)]
    assert got["ref_len"].tolist() == [5, 2 * 268435455, 0, 0, 42] and not got["status"].any()


@pytest.mark.parametrize("text,status", [
    ("12M*", stw.BAD_CHAR), ("1M\t2M", stw.BAD_CHAR), ("1M 2M", stw.BAD_CHAR), ("1M-2I", stw.BAD_CHAR), ("**", stw.BAD_CHAR),
    ("1M\xe9", stw.BAD_CHAR), ("12Q3M", stw.BAD_OP), ("5m", stw.BAD_OP), ("M", stw.EMPTY_NUMBER), ("3MM", stw.EMPTY_NUMBER),
    ("", stw.EMPTY_NUMBER), ("268435456M", stw.NUMBER_TOO_BIG), ("99999999999999999999999I", stw.NUMBER_TOO_BIG),
    ("0000000000268435456D", stw.NUMBER_TOO_BIG), ("3M4", stw.TRAILING_DIGITS), ("7", stw.TRAILING_DIGITS),
    ("3M4Q5", stw.BAD_OP), ("Q", stw.BAD_OP)])
def test_host_parser_rejected_forms(text, status):
    got = _host(["5M", text, "6D"])
    assert got["status"].tolist() == [0, status, 0] and got["words"].tolist() == [5 << 4, 6 << 4 | 2]


def test_host_parser_a_million_operations():
    rng = np.random.default_rng(2)
    text = "".join("%d%s" % (l, "MIDNSHP=X"[o]) for l, o in zip(rng.integers(1, 100000, 10 ** 6).tolist(), rng.integers(0, 9, 10 ** 6).tolist()))
    for threads in (1, 8):
        got = _host(["3S", text, "*", text[:5000] + "!", "4M"], threads)
        assert int(got["cigar_off"][-1]) == 10 ** 6 + 2


# ------------------------------------------------------------------ malformed files
def _error_of(path):
    try:
        bamio.AlignmentFile(path).load()
    except ValueError as e:
        return str(e)
    return None


@pytest.mark.parametrize("what,bad", [
    ("fewer than 11 fields", "r\t0\tchr1\t5\t60\t10M\t*\t0\t0\tACGTACGTAC"),
    ("FLAG", _line("r", 0, "chr1", 5).replace("\t0\tchr1", "\tx\tchr1")),
    ("FLAG", _line("r", 65536, "chr1", 5)),
    ("POS", _line("r", 0, "chr1", 5).replace("\t6\t60", "\t-6\t60")),
    ("MAPQ", _line("r", 0, "chr1", 5, mapq=256)),
    ("RNAME", _line("r", 0, "chr9", 5)),
    ("CIGAR", _line("r", 0, "chr1", 5, cigar="10Q")),
    ("CIGAR", _line("r", 0, "chr1", 5, cigar="10")),
    ("CIGAR", _line("r", 0, "chr1", 5, cigar="268435456M")),
    ("query length", _line("r", 0, "chr1", 5, cigar="4S5M3D")),
    ("optional field", _line("r", 0, "chr1", 5, aux=["NM:i:abc"])),
    ("optional field", _line("r", 0, "chr1", 5, aux=["NM:q:1"]))])
def test_malformed_line_is_refused_with_its_line_number(tmp_path, what, bad):
    good = [_line("g%d" % k, 0, "chr2", 10 * k) for k in range(6)]
    msg = _error_of(_sam(tmp_path, good[:4] + [bad] + good[4:]))
    # 1 @HD + 3 @SQ + 4 good lines in front of it
    assert msg is not None and "line 9" in msg and what in msg, msg
    assert _error_of(_sam(tmp_path, good, name="good.sam")) is None


def test_cigar_and_seq_may_each_be_absent(tmp_path):
    f = bamio.AlignmentFile(_sam(tmp_path, [_line("a", 0, "chr1", 5, cigar="*"), _line("b", 0, "chr1", 6, seq="*"), _line("c", 4, "*", -1, "*", "*")]))
    f.load()
    assert f._cols["l_seq"].tolist() == [10, 0, 0] and f._cols["n_cig"].tolist() == [0, 1, 0] and f._cols["ref_len"].tolist() == [0, 10, 0]


def test_files_that_are_no_sam(tmp_path):
    import gzip
    p = tmp_path / "nosq.sam"
    p.write_text("@HD\tVN:1.6\n" + _line("r", 0, "chr1", 5) + "\n")
    with pytest.raises(ValueError, match="@SQ"):
        bamio.AlignmentFile(str(p))
    (tmp_path / "empty.sam").write_bytes(b"")
    with pytest.raises(ValueError, match="@SQ"):
        bamio.AlignmentFile(str(tmp_path / "empty.sam"))
    # gzip-compressed SAM: the SAM reader itself names the two accepted forms; AlignmentFile keeps gzip input with the BAM reader
    z = str(tmp_path / "z.sam.gz")
    gzip.open(z, "wb").write(open(_sam(tmp_path, [_line("r", 0, "chr1", 5)]), "rb").read())
    import ctypes as C
    h, err = C.c_void_p(), C.create_string_buffer(512)
    assert _lib.load().svx_sam_open(os.fsencode(z), 1, C.byref(h), err, len(err)) == _lib.SVX_E_INVALID and not h.value
    assert b"uncompressed SAM" in err.value and b"BAM" in err.value
    assert not bamio.is_sam(z)
    with pytest.raises(ValueError):
        bamio.AlignmentFile(z)
    # a header only: no records, no error
    assert len(bamio.AlignmentFile(_sam(tmp_path, [], name="h.sam"))) == 0


# ------------------------------------------------------------------ alphabet and line ends
def test_bases_read_like_a_bam_round_trip(tmp_path):
    seq = "acgtnACGTN=MRSVWYHKDBmrsvwyhkdbXx.-*?uU" + "".join(chr(c) for c in range(33, 127) if chr(c) not in "\t")
    seq = seq.replace("\t", "")
    f = bamio.AlignmentFile(_sam(tmp_path, [_line("r", 0, "chr1", 5, cigar="%dM" % len(seq), seq=seq)]))
    packed = bamio.encode_seq(seq)
    exp = "".join("=ACMGRSVTWYHKDBN"[(int(packed[i >> 1]) >> (0 if i & 1 else 4)) & 15] for i in range(len(seq)))
    assert f.sequence_slices([0], [0], [len(seq)])[0] == exp
    assert f.sequence_slices([0, 0], [3, len(seq) - 2], [9, len(seq) + 50]) == [exp[3:9], exp[-2:]]
    assert f.record(0).seq_slice(2, 12) == exp[2:12]


def test_crlf_and_missing_last_line_end_and_empty_lines(tmp_path):
    lines = [_line("a", 0, "chr1", 5, aux=["NM:i:3"]), _line("b", 16, "chr2", 9)]
    ref = bamio.AlignmentFile(_sam(tmp_path, lines, name="lf.sam"))
    crlf = bamio.AlignmentFile(_sam(tmp_path, lines, name="crlf.sam", eol="\r\n"))
    raw = open(tmp_path / "lf.sam", "rb").read()
    (tmp_path / "noeol.sam").write_bytes(raw[:-1])
    (tmp_path / "blank.sam").write_bytes(raw.replace(b"\nb\t", b"\n\nb\t") + b"\n")
    for other in (crlf, bamio.AlignmentFile(str(tmp_path / "noeol.sam")), bamio.AlignmentFile(str(tmp_path / "blank.sam"))):
        assert [(r.query_name, r.flag, r.reference_start, r._parse_tags()) for r in other.fetch()] == \
               [(r.query_name, r.flag, r.reference_start, r._parse_tags()) for r in ref.fetch()]
        assert other.sequence_slices([0, 1], [0, 0], [10, 10]) == ["ACGTACGTAC"] * 2
        assert "\r" not in other.text
