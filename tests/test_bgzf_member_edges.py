"""The edges of a BGZF member header (SAM specification §4.1) as BOTH front ends that read BGZF see them: the bgzip-FASTA
handle (svx_fasta_open_bgzf) and the native BAM reader (svx_bam_open).  One table of hand-made members; each is placed
once as the second member of a small bgzipped FASTA (with the .fai / .gzi an indexer would write for it) and once as the
member behind a BAM's header and first record (with the .bai to match).  The two front ends must agree on accept / refuse
for every case, and an accepted case must yield the bytes that were written.  CPU only."""
import struct
import zlib

import numpy as np
import pytest

from svim_asm_amd import bamio, fasta
from tests import deflate_writer as DW
from tests import spec_bam_writer as W


def sub(si, payload):
    return si + struct.pack("<H", len(payload)) + payload


def member(data, front=b"", back=b"", bc_slen=2, xlen=None, bsize=None, isize=None, crc=None):
    """A gzip member around `data` whose header is written field by field: extra subfields in front of / behind BC, the
    BC subfield's SLEN, and XLEN, BSIZE, ISIZE, CRC32 as given instead of the true values."""
    comp = zlib.compressobj(6, zlib.DEFLATED, -15)
    cdata = comp.compress(data) + comp.flush()
    true_xlen = len(front) + 4 + bc_slen + len(back)
    total = 12 + true_xlen + len(cdata) + 8
    assert total <= 65536
    bc = b"BC" + struct.pack("<HH", bc_slen, total - 1 if bsize is None else bsize(true_xlen, total)) + bytes(bc_slen - 2)
    head = struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, true_xlen if xlen is None else xlen)
    return head + front + bc + back + cdata + struct.pack("<II", DW.crc32(data) ^ (crc or 0), len(data) if isize is None else isize)


# name, accepted?, what refuses it ("header": the member chain; "stream": the inflated bytes), bytes of data in the member,
# member() arguments, cut (int: the file ends that many bytes into the member; "end": right behind it; None: members follow)
CASES = [
    ("extra_subfield_in_front_of_bc", True, None, 300, dict(front=sub(b"XY", b"\xCD\xAB")), None),
    ("extra_subfield_behind_bc", True, None, 300, dict(back=sub(b"ZZ", b"abc")), None),
    ("bc_subfield_slen_not_2", False, "header", 300, dict(bc_slen=4), None),
    ("xlen_past_the_file", False, "header", 300, dict(xlen=60000), 40),
    ("bsize_below_xlen_plus_20", False, "header", 300, dict(bsize=lambda xlen, total: xlen + 18), None),
    ("bsize_past_the_file", False, "header", 300, dict(bsize=lambda xlen, total: total - 1 + 100), "end"),
    ("isize_65536", True, None, 65536, dict(), None),
    ("isize_65537", False, "header", 65537, dict(), None),
    ("file_cut_17_bytes_into_header", False, "header", 300, dict(), 17),
    ("empty_member_in_the_middle", True, None, 0, dict(), None),
    ("wrong_crc", False, "stream", 300, dict(crc=1), None),
    ("wrong_isize", False, "stream", 300, dict(isize=301), None),
]


def lay_out(stream, a, n, kw, cut):
    """The file: stream[:a] | the case's member with stream[a:a + n] | the rest in members of 65280 | the end marker.
    Returns (file bytes, compressed offset of the case's member, [(coff, true uoff, declared uoff)] of every member)."""
    parts = [stream[:a], stream[a:a + n]] + [stream[p:p + 65280] for p in range(a + n, len(stream), 65280)] + [b""]
    blobs = [member(bytes(p), **kw) if k == 1 else W.bgzf_member(bytes(p)) for k, p in enumerate(parts)]
    table, c, u, du = [], 0, 0, 0
    for k, (p, bl) in enumerate(zip(parts, blobs)):
        table.append((c, u, du))
        c += len(bl)
        u += len(p)
        du += kw.get("isize", len(p)) if k == 1 else len(p)
    if cut is not None:
        blobs = [blobs[0], blobs[1] if cut == "end" else blobs[1][:cut]]
    return b"".join(blobs), table[1][0], table


# ------------------------------------------------------------------ the two front ends
@pytest.fixture(scope="module")
def genome():
    rng = np.random.default_rng(11)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150_000)].tobytes()
    text = b">c\n" + b"".join(seq[p:p + 60] + b"\n" for p in range(0, len(seq), 60))
    return seq, text


@pytest.fixture(scope="module")
def alignments():
    refs = [("chrA", 2_000_000)]
    rng = np.random.default_rng(12)
    seq = lambda n: "".join(rng.choice(list("ACGTN"), size=n))
    recs = [dict(name="first", flag=0, tid=0, pos=100, mapq=60, cigar=[(0, 50)], seq=seq(50), tags=[]),
            dict(name="long", flag=0, tid=0, pos=500, mapq=60, cigar=[(4, 7), (0, 99_993)], seq=seq(100_000), tags=[("NM", "i", 3)]),
            dict(name="last", flag=16, tid=0, pos=900_000, mapq=7, cigar=[(0, 80)], seq=seq(80), tags=[])]
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrA\tLN:2000000\n".encode()
    stream = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1))
    stream += struct.pack("<i", 5) + b"chrA\x00" + struct.pack("<i", 2_000_000)
    bounds = []
    for r in recs:
        bounds.append(len(stream))
        stream += W.encode_record(r)
    bounds.append(len(stream))
    return refs, recs, bytes(stream), bounds


def fasta_front_end(tmp, name, genome, n, kw, cut):
    """(accepted, bytes or the refusal's text, coff of the case's member)"""
    seq, text = genome
    data, coff, table = lay_out(text, 200, n, kw, cut)
    path = str(tmp / (name + ".fa.gz"))
    open(path, "wb").write(data)
    open(path + ".fai", "w").write("c\t%d\t3\t60\t61\n" % len(seq))
    entries = [(c, du) for c, _, du in table[1:-1] if c < len(data)]
    with open(path + ".gzi", "wb") as fh:
        fh.write(struct.pack("<Q", len(entries)) + b"".join(struct.pack("<QQ", c, u) for c, u in entries))
    try:
        z = fasta.FastaFile(path)
        got = z.fetch_bytes("c")
        z.close()
        return True, got, coff
    except ValueError as e:
        return False, str(e), coff


def bam_front_end(tmp, name, alignments, n, kw, cut):
    """(accepted, [(name, pos, flag, sequence)] or the refusal's text)"""
    refs, recs, stream, bounds = alignments
    data, _, table = lay_out(stream, bounds[1], n, kw, cut)
    path = str(tmp / (name + ".bam"))
    open(path, "wb").write(data)
    ends = [u for _, u, _ in table[1:]] + [len(stream)]

    def voffset(u):  # canonical: never at the end of a member, empty members passed
        for (c, u0, _), u1 in zip(table, ends):
            if u0 <= u < u1:
                return (c << 16) | (u - u0)
        return table[-1][0] << 16
    W.write_bai(path + ".bai", len(refs), recs, [voffset(u) for u in bounds[:-1]], [voffset(u) for u in bounds[1:]])
    try:
        f = bamio.AlignmentFile(path)
        got = [(a.query_name, a.reference_start, a.flag, a.query_sequence) for a in (f.record(i) for i in range(len(f)))]
        f.close()
        return True, got
    except ValueError as e:
        return False, str(e)


def test_both_front_ends_agree_on_every_member_edge(tmp_path, genome, alignments):
    ran, wrong = 0, []
    want_records = [(r["name"], r["pos"], r["flag"], r["seq"]) for r in alignments[1]]
    for name, accepted, why, n, kw, cut in CASES:
        f_ok, f_got, coff = fasta_front_end(tmp_path, name, genome, n, kw, cut)
        b_ok, b_got = bam_front_end(tmp_path, name, alignments, n, kw, cut)
        print("%-32s fasta %-8s bam %-8s" % (name, "accepts" if f_ok else "refuses", "accepts" if b_ok else "refuses"),
              "" if f_ok else "| " + f_got[-110:], "" if b_ok else "| " + b_got[-110:])
        if f_ok != b_ok:
            wrong.append("%s: the front ends disagree (FASTA %s, BAM %s)" % (name, f_ok, b_ok))
        if f_ok != accepted or b_ok != accepted:
            wrong.append("%s: expected %s" % (name, "accepted" if accepted else "refused"))
        if f_ok and f_got != genome[0]:
            wrong.append("%s: the FASTA handle's bases differ from the text" % name)
        if b_ok and b_got != want_records:
            wrong.append("%s: the BAM reader's records differ from what was written" % name)
        if not f_ok:  # the refusal names the member, in the words of its kind
            words = {"header": "truncated or malformed BGZF member at compressed offset %d (not a complete BGZF file)" % coff,
                     "stream": "damaged or malformed BGZF member at compressed offset %d (CRC32, ISIZE or DEFLATE stream)" % coff}
            if why and words[why] not in f_got:
                wrong.append("%s: the FASTA handle refused with `%s`" % (name, f_got))
        ran += 1
    assert not wrong, "\n".join(wrong)
    assert ran == len(CASES) == 12
