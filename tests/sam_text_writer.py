"""SAM text written from the SAM specification alone (SAMv1 §1.3-1.5, §4.2.4), for the tests of the native SAM reader:
records -> lines, BAM binary aux -> TAG:TYPE:VALUE, and a pure-Python CIGAR-string parser that serves as the oracle of
svx_cigar_text_parse / svx_cigar_text_parse_dev.  Nothing here calls the code under test (same spirit as
tests/spec_bam_writer.py)."""
import random
import struct

OPS = "MIDNSHP=X"
# status codes of include/svx_sam.h, restated
OK, BAD_CHAR, BAD_OP, EMPTY_NUMBER, NUMBER_TOO_BIG, TRAILING_DIGITS = range(6)
_AUX = {"c": ("<b", 1), "C": ("<B", 1), "s": ("<h", 2), "S": ("<H", 2), "i": ("<i", 4), "I": ("<I", 4), "f": ("<f", 4)}


def cigar_string(words):
    """BAM words (len << 4 | op) -> text; no words: `*` (SAMv1 §1.4.6)."""
    words = [int(w) for w in words]
    return "".join("%d%s" % (w >> 4, OPS[w & 15]) for w in words) if words else "*"


def parse_cigar(text):
    """(status, words, ref_len) of one CIGAR string by the contract of include/svx_sam.h: the error that comes first in
    the text decides (two at one byte: the smaller code); a record with an error has no words."""
    if isinstance(text, str):
        text = text.encode("latin-1")
    if len(text) == 0:
        return EMPTY_NUMBER, [], 0
    if text == b"*":
        return OK, [], 0
    words, ref_len, digits = [], 0, b""
    for c in text:
        ch = bytes([c])
        if ch.isdigit() and c < 128:
            digits += ch
            continue
        if ch == b"*":
            return BAD_CHAR, [], 0
        if ch not in b"MIDNSHP=X":
            return (BAD_OP if (ch.isalpha() and c < 128) else BAD_CHAR), [], 0
        if not digits:
            return EMPTY_NUMBER, [], 0
        v = int(digits)
        if v >= 1 << 28:
            return NUMBER_TOO_BIG, [], 0
        op = OPS.index(ch.decode())
        words.append(v << 4 | op)
        if ch in b"MDN=X":
            ref_len += v
        digits = b""
    if digits:
        return TRAILING_DIGITS, [], 0
    return OK, words, ref_len & 0xFFFFFFFF


def parse_batch(texts):
    """The oracle of the batch entries: dict(words, cigar_off, ref_len, status) as plain lists (ref_len as int32)."""
    words, off, ref_len, status = [], [0], [], []
    for t in texts:
        st, w, rl = parse_cigar(t)
        status.append(st)
        words += w
        off.append(len(words))
        ref_len.append(rl - (1 << 32) if rl >= 1 << 31 else rl)
    return {"words": words, "cigar_off": off, "ref_len": ref_len, "status": status}


def aux_text(raw):
    """BAM binary aux bytes -> list of TAG:TYPE:VALUE (integers of every width as `i`, §1.5)."""
    out, q, raw = [], 0, bytes(raw or b"")
    while q + 3 <= len(raw):
        tag, typ = raw[q:q + 2].decode(), chr(raw[q + 2])
        q += 3
        if typ in "ZH":
            e = raw.index(b"\x00", q)
            out.append("%s:%s:%s" % (tag, typ, raw[q:e].decode()))
            q = e + 1
        elif typ == "A":
            out.append("%s:A:%s" % (tag, chr(raw[q])))
            q += 1
        elif typ == "f":
            out.append("%s:f:%r" % (tag, struct.unpack_from("<f", raw, q)[0]))
            q += 4
        elif typ in _AUX:
            fmt, size = _AUX[typ]
            out.append("%s:i:%d" % (tag, struct.unpack_from(fmt, raw, q)[0]))
            q += size
        elif typ == "B":
            sub, cnt = chr(raw[q]), struct.unpack_from("<i", raw, q + 1)[0]
            fmt, size = _AUX[sub]
            vals = struct.unpack_from("<%d%s" % (cnt, fmt[1]), raw, q + 5)
            out.append("%s:B:%s%s" % (tag, sub, "".join(",%r" % v if sub == "f" else ",%d" % v for v in vals)))
            q += 5 + cnt * size
        else:
            raise ValueError("aux type %r" % typ)
    return out


def aux_values(raw):
    """BAM binary aux bytes -> {tag: value} (integers as int whatever their width, B arrays as lists)."""
    vals = {}
    for f in aux_text(raw):
        tag, typ, v = f.split(":", 2)
        if typ == "i":
            vals[tag] = int(v)
        elif typ == "f":
            vals[tag] = struct.unpack("<f", struct.pack("<f", float(v)))[0]
        elif typ == "B":
            items = v.split(",")
            vals[tag] = [struct.unpack("<f", struct.pack("<f", float(x)))[0] if items[0] == "f" else int(x) for x in items[1:]]
        else:
            vals[tag] = v
    return vals


def record_line(qname, flag, rname, pos0, mapq, cigar, seq, aux=(), qual="*"):
    """One alignment line (§1.4); pos0 is 0-based (-1: unplaced), cigar a string, aux a list of TAG:TYPE:VALUE."""
    return "\t".join([qname, str(flag), rname, str(pos0 + 1), str(mapq), cigar, "*", "0", "0", seq or "*", qual] + list(aux))


def records_of_bam(bam):
    """Lines for every record of a bamio.AlignmentFile opened with reader="python", in file order."""
    lines = []
    for r in bam.fetch():
        rname = bam.references[r.reference_id] if r.reference_id >= 0 else "*"
        lines.append(record_line(r.query_name, r.flag, rname, r.reference_start, r.mapping_quality,
                                 cigar_string(r.cigar_words), r.query_sequence or "", aux_text(r._tags_raw)))
    return lines


def header_text(references, lengths, so="unsorted", extra=()):
    """@HD (so=None: no @HD line at all), @SQ per contig, then `extra` lines."""
    lines = [] if so is None else ["@HD\tVN:1.6\tSO:%s" % so]
    lines += ["@SQ\tSN:%s\tLN:%d" % (n, l) for n, l in zip(references, lengths)]
    return lines + list(extra)


def write_sam(path, references, lengths, lines, so="unsorted", shuffle_seed=None, eol="\n"):
    lines = list(lines)
    if shuffle_seed is not None:
        random.Random(shuffle_seed).shuffle(lines)
    with open(path, "w", newline="") as f:
        f.write("".join(l + eol for l in header_text(references, lengths, so) + lines))
    return path


def bam_as_sam(bam_path, sam_path, so="unsorted", shuffle_seed=1, eol="\n"):
    """The records of a BAM rendered as a SAM with the lines shuffled."""
    from svim_asm_amd import bamio
    bam = bamio.AlignmentFile(bam_path, reader="python")
    return write_sam(sam_path, bam.references, bam.lengths, records_of_bam(bam), so=so, shuffle_seed=shuffle_seed, eol=eol)
