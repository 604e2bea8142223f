"""The native PAF reader (csrc/svx_paf.cpp behind include/svx_paf.h) without a GPU: hand-written rows against the column
table of the header value for value, every refusal with its line number, and the differential test — random record sets
rendered once as SAM (tests/sam_text_writer.py: soft clips, full SEQ, SA as the header defines it) and once as PAF + FASTA
must give the same columns and the same bases through the SAM handle (merged code, the yardstick) and the PAF handle."""
import os

import numpy as np
import pytest

from tests import paf_writer as pw, sam_text_writer as stw

REFS, LENS = ["chrA", "chrB", "chrC"], [100000, 50000, 7000]


def write_ref(tmp_path):
    path = str(tmp_path / "ref.fa")
    with open(path + ".fai", "w") as f:
        off = 0
        for n, l in zip(REFS, LENS):
            f.write("%s\t%d\t%d\t60\t61\n" % (n, l, off + len(n) + 2))
            off += len(n) + 2 + l + (l + 59) // 60
    return path


def open_paf(tmp_path, rows, seqs=None, eol="\n", name="a.paf", threads=3, line=60):
    from svim_asm_amd import bamio
    ref = write_ref(tmp_path)
    paf = pw.write_paf(str(tmp_path / name), rows, eol=eol)
    seqs = seqs or {}
    fa = pw.write_fasta(str(tmp_path / (name + ".fa")), list(seqs), list(seqs.values()), line=line)
    return bamio.AlignmentFile(paf, query=fa, reference=ref, threads=threads)


def columns(f):
    f.load()
    out = []
    for i in range(f.n_records):
        sa = f._aux_pool[f._sa_off[i]:f._sa_off[i] + f._sa_len[i]].decode() if f._sa_off[i] >= 0 else None
        words = f._cigar[f._cig_off[i]:f._cig_off[i + 1]]
        out.append(dict(name=f._names_pool[f._name_off[i]:f._name_off[i + 1]].decode(), tid=int(f._cols["tid"][i]),
                        pos=int(f._cols["pos"][i]), flag=int(f._cols["flag"][i]), mapq=int(f._cols["mapq"][i]),
                        l_seq=int(f._cols["l_seq"][i]), ref_len=int(f._cols["ref_len"][i]), cigar=stw.cigar_string(words),
                        sa=sa, nm=stw.aux_values(f._aux_pool[f._aux_off[i]:f._aux_off[i + 1]]).get("NM"),
                        voffset=int(f._cols["voffset"][i])))
    return out


def row(q, qlen, qs, qe, strand, t, ts, te, mapq, *tags):
    tl = LENS[REFS.index(t)] if t in REFS else 1000
    return "\t".join([q, str(qlen), str(qs), str(qe), strand, t, str(tl), str(ts), str(te), "0", "0", str(mapq)] + list(tags))


HAND = [
    row("q1", 1000, 100, 400, "+", "chrA", 5000, 5300, 60, "tp:A:P", "NM:i:3", "cg:Z:300M"),            # 0 primary of q1
    row("q2", 500, 0, 500, "-", "chrB", 10, 530, 7, "cg:Z:200M20D300M"),                                  # 1 no tp, no NM
    row("q1", 1000, 400, 900, "-", "chrA", 9000, 9450, 50, "tp:A:P", "NM:i:300", "cg:Z:100M50I350M"),   # 2 supplementary, I
    row("q1", 1000, 900, 1000, "+", "chrC", 100, 300, 0, "tp:A:I", "cg:Z:50M100D50M"),                    # 3 supplementary, D
    row("q1", 1000, 0, 50, "+", "chrA", 100, 150, 3, "tp:A:S", "cg:Z:50M"),                               # 4 secondary
    row("q3", 60, 10, 60, "-", "chrA", 5000, 5050, 255, "tp:A:i", "NM:i:70000", "cg:Z:50="),            # 5 same pos as row 0
    row("q1", 1000, 0, 100, "+", "chrB", 0, 100, 1, "tp:A:S"),                                            # 6 secondary, no cg
]


def test_hand_written_rows_give_the_columns_of_the_header(tmp_path):
    text = "\n".join(HAND) + "\n"
    offs = [0]
    for r in HAND:
        offs.append(offs[-1] + len(r) + 1)
    got = columns(open_paf(tmp_path, HAND))
    by_line = {c["voffset"]: c for c in got}
    c = [by_line[offs[k]] for k in range(len(HAND))]
    assert [x["voffset"] for x in got] == [offs[k] for k in (4, 0, 5, 2, 6, 1, 3)]  # (tid, pos, strand, place in the file)
    assert c[0] == dict(name="q1", tid=0, pos=5000, flag=0, mapq=60, l_seq=1000, ref_len=300, cigar="100S300M600S", nm=3,
                        sa="chrA,9001,-,100S450M50I400S,50,300;chrC,101,+,900S100M100D,0,0;", voffset=offs[0])
    assert c[1] == dict(name="q2", tid=1, pos=10, flag=16, mapq=7, l_seq=500, ref_len=520, cigar="200M20D300M", nm=None, sa=None,
                        voffset=offs[1])
    assert c[2] == dict(name="q1", tid=0, pos=9000, flag=0x810, mapq=50, l_seq=1000, ref_len=450, cigar="100S100M50I350M400S",
                        nm=300, sa="chrA,5001,+,100S300M600S,60,3;chrC,101,+,900S100M100D,0,0;", voffset=offs[2])
    assert c[3] == dict(name="q1", tid=2, pos=100, flag=0x800, mapq=0, l_seq=1000, ref_len=200, cigar="900S50M100D50M", nm=None,
                        sa="chrA,5001,+,100S300M600S,60,3;chrA,9001,-,100S450M50I400S,50,300;", voffset=offs[3])
    assert c[4] == dict(name="q1", tid=0, pos=100, flag=0x100, mapq=3, l_seq=1000, ref_len=50, cigar="50M950S", nm=None, sa=None,
                        voffset=offs[4])
    assert c[5] == dict(name="q3", tid=0, pos=5000, flag=16, mapq=255, l_seq=60, ref_len=50, cigar="50=10S", nm=70000, sa=None,
                        voffset=offs[5])
    assert c[6] == dict(name="q1", tid=1, pos=0, flag=0x100, mapq=1, l_seq=1000, ref_len=0, cigar="*", nm=None, sa=None,
                        voffset=offs[6])
    assert len(text) == offs[-1]


def test_the_handle_presents_the_reference_dictionary(tmp_path):
    f = open_paf(tmp_path, HAND)
    assert f.is_paf and f.is_sam and list(f.references) == REFS and list(f.lengths) == LENS
    assert [(d["SN"], int(d["LN"])) for d in f.header["SQ"]] == list(zip(REFS, LENS)) and "HD" not in f.header
    assert f.get_reference_length("chrB") == 50000 and f.check_index() is True and f.contig_spans() is None


def test_crlf_empty_lines_and_shuffles_do_not_change_the_records(tmp_path):
    import random
    base = [{k: v for k, v in c.items() if k != "voffset"} for c in columns(open_paf(tmp_path, HAND))]
    crlf = columns(open_paf(tmp_path, [HAND[0], ""] + HAND[1:], eol="\r\n", name="b.paf"))
    assert [{k: v for k, v in c.items() if k != "voffset"} for c in crlf] == base
    # rows of other queries moved about, the rows of q1 kept in their order: the same records in the same order
    for seed in range(5):
        others = [1, 5]
        order = [0, 2, 3, 4, 6]
        for k in others:
            order.insert(random.Random(seed * 7 + k).randrange(len(order) + 1), k)
        got = columns(open_paf(tmp_path, [HAND[k] for k in order], name="s%d.paf" % seed, threads=1 + seed))
        assert [{k: v for k, v in c.items() if k != "voffset"} for c in got] == base


def test_file_order_decides_the_primary(tmp_path):
    got = columns(open_paf(tmp_path, [HAND[3], HAND[0], HAND[2]]))
    flags = {c["pos"]: c["flag"] for c in got}
    assert flags == {100: 0, 5000: 0x800, 9000: 0x810}
    assert {c["pos"]: c["sa"] for c in got}[5000] == "chrC,101,+,900S100M100D,0,0;chrA,9001,-,100S450M50I400S,50,300;"


def test_load_of_some_contigs_keeps_flags_and_sa_of_the_whole_file(tmp_path):
    f = open_paf(tmp_path, HAND)
    whole = {c["voffset"]: c for c in columns(f)}
    f.load(["chrC"])
    f2 = open_paf(tmp_path, HAND, name="c.paf")
    f2.load(["chrC"])
    assert f2.n_records == 1 and int(f2._cols["flag"][0]) == 0x800
    assert f2._aux_pool[f2._sa_off[0]:f2._sa_off[0] + f2._sa_len[0]].decode() == [c for c in whole.values() if c["tid"] == 2][0]["sa"]


GOOD = row("q", 100, 10, 90, "+", "chrA", 1000, 1080, 60, "tp:A:P", "cg:Z:80M")
REFUSED = [
    ("\t".join(GOOD.split("\t")[:11]), "fewer than 12"),
    (row("q", "x", 10, 90, "+", "chrA", 1000, 1080, 60, "cg:Z:80M"), "column 2"),
    (row("q", 100, 95, 90, "+", "chrA", 1000, 1080, 60, "cg:Z:80M"), "columns 3 and 4"),
    (row("q", 100, 10, 101, "+", "chrA", 1000, 1091, 60, "cg:Z:91M"), "columns 3 and 4"),
    (row("q", 100, 10, 90, "+", "chrA", 1080, 1000, 60, "cg:Z:80M"), "columns 8 and 9"),
    (row("q", 100, 10, 90, "+", "chrA", 99990, 100070, 60, "cg:Z:80M"), "columns 8 and 9"),
    (row("q", 100, 10, 90, "+", "chrA", 1000, 1080, 256, "cg:Z:80M"), "MAPQ"),
    (row("q", 100, 10, 90, "+", "chrA", 1000, 1080, "-1", "cg:Z:80M"), "MAPQ"),
    (row("q", 100, 10, 90, "*", "chrA", 1000, 1080, 60, "cg:Z:80M"), "strand"),
    (row("q", 100, 10, 90, "+", "chrZ", 1000, 1080, 60, "cg:Z:80M"), "chrZ"),
    (GOOD.replace("\t100000\t", "\t100001\t"), "has length 100001 here and 100000"),
    (row("q", 100, 10, 90, "+", "chrA", 1000, 1080, 60, "tp:A:P"), "minimap2 runs with -c"),
    (row("q", 100, 10, 90, "+", "chrA", 1000, 1080, 60, "cg:Z:80Q"), "CIGAR has an operator outside"),
    (row("q", 100, 10, 90, "+", "chrA", 1000, 1080, 60, "cg:Z:80"), "CIGAR has digits without"),
    (row("q", 100, 10, 90, "+", "chrA", 1000, 1080, 60, "cg:Z:80M0"), "CIGAR has digits without"),
    (row("q", 100, 10, 90, "+", "chrA", 1000, 1080, 60, "cg:Z:"), "operator without a length"),
    (row("q", 100, 10, 90, "+", "chrA", 1000, 1080, 60, "cg:Z:40M*40M"), "CIGAR has a character"),
    (row("q", 100, 10, 90, "+", "chrA", 1000, 1080, 60, "cg:Z:70M10D"), "query length differs"),
    (row("q", 100, 10, 90, "+", "chrA", 1000, 1080, 60, "cg:Z:80M5D"), "reference length differs"),
    (row("q", 101, 10, 90, "+", "chrA", 2000, 2080, 60, "cg:Z:80M"), "has length 101 here and 100 in an earlier row"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_refusals_name_the_line(tmp_path, k):
    bad, what = REFUSED[k]
    f = open_paf(tmp_path, [GOOD, "", GOOD.replace("1000\t1080", "3000\t3080"), bad, GOOD.replace("1000\t1080", "5000\t5080")])
    with pytest.raises(ValueError) as e:
        f.load()
    assert "line 4: " in str(e.value) and what in str(e.value), str(e.value)


def test_what_open_refuses(tmp_path):
    for name, content, what in (("e.paf", b"", "is empty"), ("n.paf", b"\n\r\n", "is empty"),
                                ("s.paf", b"\n@HD\tVN:1.6\n@SQ\tSN:chrA\tLN:100000\n", "SAM"),
                                ("g.paf", b"\x1f\x8b\x08\x00", "gzip")):
        p = tmp_path / name
        p.write_bytes(content)
        from svim_asm_amd import bamio
        fa = pw.write_fasta(str(tmp_path / (name + ".fa")), ["q"], [b"ACGT"])
        with pytest.raises(ValueError, match=what):
            bamio.AlignmentFile(str(p), query=fa, reference=write_ref(tmp_path))


def test_query_names_and_lengths_are_checked_against_the_assembly(tmp_path):
    f = open_paf(tmp_path, [GOOD], seqs={"other": b"A" * 100})
    with pytest.raises(ValueError, match="line 1: the query 'q' is not in the query FASTA's index"):
        f.sequence_slices_raw([0], [0], [10])
    f = open_paf(tmp_path, [GOOD], seqs={"q": b"A" * 99}, name="l.paf")
    with pytest.raises(ValueError, match="line 1: the query 'q' has length 100 here and 99"):
        f.sequence_slices_raw([0], [0], [10])


# ---------------------------------------------------------------------------------------------- differential
def random_set(seed):
    """Queries with IUPAC and lower-case bases and one to four alignments each on both strands."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTACGTACGTacgtNnRYKMSWBDHVrykmswbdhvXu", np.uint8)
    alns, seqs = [], {}
    for q in range(int(rng.integers(5, 25))):
        qlen = int(rng.integers(50, 4000))
        name = "ctg%d" % q
        seqs[name] = letters[rng.integers(0, len(letters), qlen)].tobytes()
        cuts = sorted(set(rng.integers(0, qlen + 1, int(rng.integers(2, 6))).tolist()))
        for a, b in zip(cuts[:-1], cuts[1:]):
            if rng.random() < 0.15:
                continue
            left, ops = b - a, []
            while left > 0:  # M / I / X / = take query bases, D / N only reference
                l = int(min(left, rng.integers(1, 200)))
                ops.append((l, "M=XI"[int(rng.integers(0, 4))] if ops and ops[-1][1] != "I" else (l, "M")[1]))
                left -= l
                if left > 0 and rng.random() < 0.4:
                    ops.append((int(rng.integers(1, 300)), "DN"[int(rng.integers(0, 2))]))
            if ops[-1][1] in "DNI":
                ops[-1] = (ops[-1][0], "M") if ops[-1][1] == "I" else ops[-1]
                if ops[-1][1] in "DN":
                    ops.pop()
            t = int(rng.integers(0, 3))
            span = sum(l for l, o in ops if o in "MDN=X")
            alns.append(pw.Aln(name, qlen, a, b, "+-"[int(rng.integers(0, 2))], REFS[t], int(rng.integers(0, LENS[t] - span)),
                               int(rng.integers(0, 61)), ops, nm=int(rng.integers(0, 100000)) if rng.random() < 0.7 else None,
                               tp=[None, "P", "P", "S", "I"][int(rng.integers(0, 5))]))
    order = rng.permutation(len(alns))
    return [alns[k] for k in order], seqs


@pytest.mark.parametrize("seed", range(8))
def test_paf_plus_fasta_equals_the_sam_of_the_same_records(tmp_path, seed):
    from svim_asm_amd import bamio
    alns, seqs = random_set(seed)
    meta = pw.flags_and_sa(alns)
    sam = stw.write_sam(str(tmp_path / "a.sam"), REFS, LENS, [pw.sam_line(a, fl, sa, seqs[a.qname].decode("latin-1"))
                                                               for a, (fl, sa) in zip(alns, meta)], so=None)
    S = bamio.AlignmentFile(sam, threads=2)
    P = open_paf(tmp_path, [pw.paf_row(a, LENS[REFS.index(a.tname)]) for a in alns], seqs=seqs, line=[60, 1, 0, 7][seed % 4])
    S.load(); P.load()
    assert S.n_records == P.n_records == len(alns)
    for k in ("tid", "pos", "l_seq", "ref_len", "flag", "mapq", "n_cig"):
        assert np.array_equal(S._cols[k], P._cols[k]), k
    assert np.array_equal(S._cigar, P._cigar) and np.array_equal(S._cig_off, P._cig_off)
    assert S._names_pool == P._names_pool and np.array_equal(S._name_off, P._name_off)
    for i in range(S.n_records):
        sa = [f._aux_pool[f._sa_off[i]:f._sa_off[i] + f._sa_len[i]] if f._sa_off[i] >= 0 else None for f in (S, P)]
        assert sa[0] == sa[1], i
        nm = [stw.aux_values(f._aux_pool[f._aux_off[i]:f._aux_off[i + 1]]).get("NM") for f in (S, P)]
        assert nm[0] == nm[1], i
    rng = np.random.default_rng(seed + 100)
    n = 400
    rec = rng.integers(0, S.n_records, n)
    l = S._cols["l_seq"][rec]
    begin = (rng.random(n) * (l + 40)).astype(np.int64) - 20   # (also before 0 and behind l_seq)
    end = begin + rng.integers(0, 300, n)
    rec = np.concatenate([rec, np.arange(S.n_records)])
    begin = np.concatenate([begin, np.zeros(S.n_records, np.int64)])
    end = np.concatenate([end, S._cols["l_seq"]])
    a, b = S.sequence_slices_raw(rec, begin, end), P.sequence_slices_raw(rec, begin, end)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    assert S.sequence_slices(rec[:20], begin[:20], end[:20]) == P.sequence_slices(rec[:20], begin[:20], end[:20])
