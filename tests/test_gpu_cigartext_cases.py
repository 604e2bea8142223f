"""The CIGAR text kernels (svim_asm_amd/csrc/svx_cigartext.hip) held to the case table of tests/cigartext_cases.py: every
case and the combined batch through svx_cigar_text_parse_dev against the pure-Python oracle
(tests/sam_text_writer.parse_batch) on status, cigar_off, ref_len and words, with a capacity of n_bytes / 2 + 1 and of
exactly n_bytes / 2, on output buffers that were filled beforehand (every byte behind the documented rows stays the
fill); the two refusals of the entry point; the combined batch on poisoned scratch and behind calls of other sizes; and
the SAM reader's own launches (svx_cigar_text_parse_on_stream) on the good records of the combined batch and on one bad
record per error code.  tests/test_cigartext_cases.py holds the table to its preconditions where there is no GPU."""
import random

import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import cigartext_cases as T
from tests import sam_text_writer as stw
from tests import test_gpu_sam as tsam

pytestmark = pytest.mark.gpu
GUARD = 64     # bytes behind every caller-owned output that no call may touch
FILL = 0x5A
KEYS = ("status", "cigar_off", "ref_len", "words")


def parse_dev(ctx, text, rec_off, cap, fill=FILL, n_bytes=None):
    """A raw call of svx_cigar_text_parse_dev with `cap` word slots, every output pre-filled with `fill` and GUARD bytes
    longer than documented: -> (return code, dict(status, cigar_off, ref_len, words, untouched) or None when refused;
    `untouched`: whether every byte behind the documented rows is still the fill, after a refusal every byte)."""
    n = len(rec_off) - 1
    n_bytes = len(text) if n_bytes is None else n_bytes

    def filled(nbytes):
        return ctx.dev_array(np.full(nbytes + GUARD, fill, np.uint8))
    d_text = ctx.dev_array(np.concatenate((np.asarray(text, np.uint8), np.zeros(1, np.uint8))))
    d_off = ctx.dev_array(np.ascontiguousarray(rec_off, np.uint64))
    bufs = {"words": filled(4 * cap), "cigar_off": filled(8 * (n + 1)), "ref_len": filled(4 * n), "status": filled(4 * n)}
    try:
        rc = ctx.lib.svx_cigar_text_parse_dev(ctx.h, d_text.ptr, n_bytes, d_off.ptr, n, bufs["words"].ptr, cap, bufs["cigar_off"].ptr,
                                              bufs["ref_len"].ptr, bufs["status"].ptr)
        ctx.sync()
        raw = {key: d.download(np.uint8) for key, d in bufs.items()}
    finally:
        for d in [d_text, d_off] + list(bufs.values()):
            d.free()
    if rc != 0:
        return rc, {"untouched": all(bool((a == fill).all()) for a in raw.values())}
    coff = raw["cigar_off"][:8 * (n + 1)].view(np.uint64)
    total = int(coff[-1])
    assert total <= cap, (total, cap)
    out = {"cigar_off": coff, "words": raw["words"][:4 * total].view(np.uint32), "ref_len": raw["ref_len"][:4 * n].view(np.int32),
           "status": raw["status"][:4 * n].view(np.uint32)}
    out["untouched"] = bool((raw["words"][4 * total:] == fill).all() and (raw["cigar_off"][8 * (n + 1):] == fill).all() and
                            (raw["ref_len"][4 * n:] == fill).all() and (raw["status"][4 * n:] == fill).all())
    return rc, out


def case_of(name):
    return T.combined() if name == "combined" else T.CASES[name]


def run(ctx, name, exact_cap=False, what="", fill=FILL):
    c, E = case_of(name), T.case_expected(name)
    cap = len(c.text) // 2 + (0 if exact_cap else 1)
    rc, got = parse_dev(ctx, c.text, c.rec_off, cap, fill)
    where = "%s, cap %d of %d bytes %s" % (name, cap, len(c.text), what)
    assert rc == 0, (where, rc)
    for key in KEYS:
        a, b = np.asarray(got[key], np.int64), getattr(E, key)
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0]) if a.shape == b.shape else -1
            raise AssertionError("%s: %s differs (first at %d: %s, expected %s; %d entries)" % (
                where, key, at, a[at] if at >= 0 else a.shape, b[at] if at >= 0 else b.shape, len(b)))
    assert got["untouched"], (where, "bytes behind the documented rows were written")


@pytest.mark.parametrize("family", T.FAMILIES)
def test_every_case(svx_ctx, family):
    """Each case with one spare word slot (what every caller of the library passes) and with none."""
    cases = T.family(family)
    assert cases
    for c in cases:
        run(svx_ctx, c.name)
        run(svx_ctx, c.name, exact_cap=True)


def test_every_word_slot_is_used(svx_ctx):
    """`1M` over and over with cap == n_bytes / 2: the last word lies in the last slot."""
    for c in T.family("capacity"):
        E = T.case_expected(c.name)
        assert int(E.cigar_off[-1]) == len(c.text) // 2 and len(c.text) in (2, 1024, 2050)
        rc, got = parse_dev(svx_ctx, c.text, c.rec_off, len(c.text) // 2)
        assert rc == 0 and len(got["words"]) == len(c.text) // 2 and (got["words"] == (1 << 4)).all() and got["untouched"], c.name


def test_combined_batch(svx_ctx):
    run(svx_ctx, "combined")
    run(svx_ctx, "combined", exact_cap=True)


def test_refusals_leave_the_context_usable(svx_ctx):
    good = "wave-over-2-3-32-records"
    c = T.CASES[good]
    # one word slot fewer than the documented minimum
    rc, got = parse_dev(svx_ctx, c.text, c.rec_off, len(c.text) // 2 - 1)
    assert rc == _lib.SVX_E_INVALID and got["untouched"]
    assert b"cap" in (svx_ctx.lib.svx_last_error(svx_ctx.h) or b"")
    run(svx_ctx, good, what="(behind a refused capacity)")
    # a text of 2^40 bytes: refused on the host before anything is launched (the buffers are those of the small case)
    rc, got = parse_dev(svx_ctx, c.text, c.rec_off, len(c.text) // 2 + 1, n_bytes=1 << 40)
    assert rc == _lib.SVX_E_INVALID and got["untouched"]
    run(svx_ctx, good, what="(behind a refused length)")
    run(svx_ctx, good, exact_cap=True, what="(behind a refused length)")


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_combined_batch_on_poisoned_scratch(svx_ctx, byte):
    """chunk_cnt, chunk_base, rank, the error keys and n_ops are written before they are read, ref_len is cleared."""
    run(svx_ctx, "combined")                      # (the regions have their size: the fill lands on what the next call uses)
    svx_ctx.scratch_fill(byte)
    run(svx_ctx, "combined", what="(scratch 0x%02X)" % byte, fill=byte)
    svx_ctx.scratch_fill(byte)
    run(svx_ctx, "combined", exact_cap=True, what="(scratch 0x%02X)" % byte, fill=byte ^ 0xFF)


def test_combined_batch_behind_calls_of_other_sizes(svx_ctx):
    """The five scratch arrays lie one behind the other, sized by the chunk and record counts: behind a call of another
    size every one of them begins elsewhere, on what that call left."""
    for other in ("size-1", "records-2049", "chunks-1025", "records-only-empty-1025"):
        run(svx_ctx, other, what="(in front of the combined batch)")
        run(svx_ctx, "combined", what="(behind %s)" % other)


# ------------------------------------------------------------------ the reader's own launches
REFS, LENS = ("chr1", "chr2"), (2_000_000_000, 1000)


def _line(q, cigar, pos0=7):
    return stw.record_line(q, 0, "chr1", pos0, 60, cigar, "*")


@pytest.fixture(scope="module")
def good_sam(tmp_path_factory):
    """The good records of the combined batch as SAM lines in shuffled order, SEQ `*`; -> (path, the texts in the
    reader's order: by position, then by place in the file)."""
    comb, E = T.combined(), T.case_expected("combined")
    texts = [t for t, ok in zip(comb.texts, E.good) if ok]
    assert len(texts) > 10_000 and b"*" in texts
    rnd = random.Random(7)
    rnd.shuffle(texts)
    pos = [rnd.randrange(0, 1000) for _ in texts]
    path = str(tmp_path_factory.mktemp("cigartext") / "good.sam")
    stw.write_sam(path, REFS, LENS, [_line("r%d" % i, t.decode("ascii"), p) for i, (t, p) in enumerate(zip(texts, pos))])
    order = np.argsort(np.asarray(pos), kind="stable")
    return path, [texts[i] for i in order]


@pytest.mark.parametrize("device_parse", ["1", "0"])
def test_reader_parses_the_good_records_of_the_combined_batch(svx_ctx, good_sam, device_parse, monkeypatch):
    from svim_asm_amd import bamio
    monkeypatch.setenv("SVX_SAM_DEVICE", device_parse)
    path, texts = good_sam
    exp = stw.parse_batch(texts)
    f = bamio.AlignmentFile(path, device=0)
    f.load()
    assert f.is_sam and f.parsed_on_device == (device_parse == "1") and f.cigar_pinned and len(f) == len(texts)
    assert np.array_equal(f._cigar, np.asarray(exp["words"], np.uint32))
    assert np.array_equal(f._cig_off, np.asarray(exp["cigar_off"], np.int64))
    assert np.array_equal(f._cols["ref_len"], np.asarray(exp["ref_len"], np.int64))
    address, _none, _us = f.device_pool(wait=True)
    assert np.array_equal(tsam.device_words(address, len(f._cigar)), np.asarray(exp["words"], np.uint32))


BAD_RECORDS = {stw.BAD_CHAR: "12M!3M", stw.BAD_OP: "12Q3M", stw.EMPTY_NUMBER: "3MM", stw.NUMBER_TOO_BIG: "5M268435456D",
               stw.TRAILING_DIGITS: "3M4"}
STATUS_TEXT = {stw.BAD_CHAR: "a character that cannot stand in a CIGAR", stw.BAD_OP: "an operator outside MIDNSHP=X",
               stw.EMPTY_NUMBER: "an operator without a length", stw.NUMBER_TOO_BIG: "a length of 2^28 or more",
               stw.TRAILING_DIGITS: "digits without an operator at its end"}


@pytest.mark.parametrize("code", sorted(BAD_RECORDS))
def test_reader_refuses_one_bad_record_among_good_ones(svx_ctx, tmp_path, code, monkeypatch):
    from svim_asm_amd import bamio
    assert stw.parse_cigar(BAD_RECORDS[code])[0] == code
    good = ["%dM%dI%dD" % (k + 1, k + 2, k + 3) for k in range(12)]
    lines = [_line("g%d" % k, t, 10 * k) for k, t in enumerate(good)]
    lines.insert(6, _line("bad", BAD_RECORDS[code], 55))
    path = stw.write_sam(str(tmp_path / "bad.sam"), REFS, LENS, lines)
    line_no = 1 + len(REFS) + 6 + 1                       # @HD, the @SQ lines, six good lines in front of it
    said = {}
    for device_parse in ("1", "0"):
        monkeypatch.setenv("SVX_SAM_DEVICE", device_parse)
        with pytest.raises(ValueError) as e:
            bamio.AlignmentFile(path, device=0).load()
        said[device_parse] = str(e.value)
        assert "line %d: the CIGAR has %s" % (line_no, STATUS_TEXT[code]) in said[device_parse], said
    assert said["1"] == said["0"]
    # the same lines without the bad one load, on the device
    monkeypatch.setenv("SVX_SAM_DEVICE", "1")
    del lines[6]
    f = bamio.AlignmentFile(stw.write_sam(str(tmp_path / "good.sam"), REFS, LENS, lines), device=0)
    f.load()
    assert f.parsed_on_device and np.array_equal(f._cigar, np.asarray(stw.parse_batch(good)["words"], np.uint32))
