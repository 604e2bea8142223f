"""svx_bgzf_inflate_dev on the seeded corpus of tests/deflate_writer.py: streams written from RFC 1951 alone — the encodings
zlib's and libdeflate's compressors never use, malformed streams with a CONSISTENT trailer (only a structural check can
refuse them), valid streams with a wrong ISIZE / CRC32, streams cut short.  The three forms of the decoder in one test body
(svx_bgzf_inflate_set_two_pass): the same statuses and bytes (include/svx.h), each the corpus's expectation; writes only
inside a member's stretch and the 7 bytes behind it; inputs at every offset mod 16; the token arena cut into slices."""
import numpy as np
import pytest

from tests import deflate_writer as dw

pytestmark = pytest.mark.gpu

FORMS = {"one_pass": 0, "lane_parse": 2, "wave_parse": 1}
SENTINEL = 0xA5
GAP = 64            # bytes between two members' output stretches (svx.h asks for 8)


@pytest.fixture(scope="module")
def corpus():
    return dw.spec_corpus(0)


def inflate_raw(svx_ctx, members, in_residue=0):
    """One svx_bgzf_inflate_dev call over `members`, buffers laid out by hand: member k's input at an offset of residue
    (k + in_residue) % 16, 3 bytes of padding behind the last input; the output buffer filled with SENTINEL, GAP bytes
    between stretches and behind the last one.  A member with ISIZE > 65536 gets a stretch of 65536 bytes (nothing may be
    written into it).  Returns (status, the whole output buffer, out_off, stretch lengths)."""
    n = len(members)
    in_off, at = [], 0
    for k, m in enumerate(members):
        at = (at + 15) // 16 * 16 + (k + in_residue) % 16
        in_off.append(at)
        at += len(m.payload)
    blob = np.zeros(at + 3, np.uint8)
    for m, o in zip(members, in_off):
        blob[o:o + len(m.payload)] = np.frombuffer(m.payload, np.uint8)
    stretch = [min(m.isize, 65536) for m in members]
    out_off, at = [], GAP
    for ln in stretch:
        out_off.append(at)
        at = (at + ln + GAP + 15) // 16 * 16
    host = [blob, np.array(in_off, np.uint64), np.array([len(m.payload) for m in members], np.uint32),
            np.array([m.isize for m in members], np.uint32), np.array([m.crc for m in members], np.uint32),
            np.array(out_off, np.uint64)]
    d = [svx_ctx.dev_array(x) for x in host]
    d_out = svx_ctx.dev_array(np.full(at, SENTINEL, np.uint8))
    d_st = svx_ctx.dev_array(np.full(n, 0xFFFFFFFF, np.uint32))
    try:
        svx_ctx._check(svx_ctx.lib.svx_bgzf_inflate_dev(svx_ctx.h, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, n,
                                                        d_out.ptr, d[5].ptr, d_st.ptr))
        svx_ctx.sync()
        return d_st.download(np.uint32), d_out.download(np.uint8), out_off, stretch
    finally:
        for x in d + [d_out, d_st]:
            x.free()


def check_guards(members, flat, out_off, stretch):
    """Every byte more than 7 bytes behind a member's stretch, and in front of the first one, is still the sentinel; a
    member with ISIZE > 65536 has left its whole stretch alone."""
    guard = np.ones(len(flat), bool)
    for m, o, ln in zip(members, out_off, stretch):
        if m.isize <= 65536:
            guard[o:o + ln + 7] = False
    bad = np.flatnonzero(guard & (flat != SENTINEL))
    assert len(bad) == 0, "bytes written outside the stretches at %s" % bad[:16].tolist()


def check_expectation(members, status, flat, out_off):
    for k, m in enumerate(members):
        st = int(status[k])
        if m.status == dw.TRUNC:
            assert st != 0, (k, m.name)  # (1, 2 or 4: the zero bits behind the cut decide; svx.h does not pin it)
        else:
            assert st == m.status, (k, m.name, st)
        if st == 0:
            got = flat[out_off[k]:out_off[k] + m.isize].tobytes()
            assert got == m.expect, (k, m.name)


def run_forms(svx_ctx, members, in_residue=0):
    """The three forms over the same call: statuses identical, bytes identical where the status is 0, and both what the
    corpus expects; the guard bytes intact after each."""
    results = {}
    was = svx_ctx.lib.svx_bgzf_inflate_set_two_pass(1)
    try:
        for name, form in FORMS.items():
            svx_ctx.lib.svx_bgzf_inflate_set_two_pass(form)
            status, flat, out_off, stretch = inflate_raw(svx_ctx, members, in_residue)
            check_guards(members, flat, out_off, stretch)
            results[name] = (status, flat)
    finally:
        svx_ctx.lib.svx_bgzf_inflate_set_two_pass(was)
    ref_status, ref_flat = results["wave_parse"]
    for name, (status, flat) in results.items():
        assert status.tolist() == ref_status.tolist(), (name, [(k, members[k].name, int(a), int(b)) for k, (a, b) in
                                                                enumerate(zip(status, ref_status)) if a != b][:10])
        for k, m in enumerate(members):
            if status[k] == 0:
                o = out_off[k]
                assert np.array_equal(flat[o:o + m.isize], ref_flat[o:o + m.isize]), (name, k, m.name)
        check_expectation(members, status, flat, out_off)
    return ref_status


def test_three_forms_same_statuses_and_bytes(svx_ctx, corpus):
    status = run_forms(svx_ctx, corpus)
    got = {}
    for m, st in zip(corpus, status.tolist()):
        got.setdefault(m.status, set()).add(st)
    # every pinned category came out as pinned; the cut streams are refused
    assert got[dw.OK] == {0} and got[dw.BAD] == {1} and got[dw.SIZE] == {2} and got[dw.CRC] == {3}
    assert 0 not in got[dw.TRUNC]


def test_inputs_at_every_offset_mod_16(svx_ctx, corpus):
    """svx.h: the payloads lie anywhere in one buffer — here at every residue mod 16 (the reader and the wrapper only use
    multiples of 4), each member at each residue across the sixteen calls of the shipped form; all three forms at
    three more."""
    was = svx_ctx.lib.svx_bgzf_inflate_set_two_pass(1)
    try:
        for residue in range(16):
            status, flat, out_off, stretch = inflate_raw(svx_ctx, corpus, residue)
            check_guards(corpus, flat, out_off, stretch)
            check_expectation(corpus, status, flat, out_off)
    finally:
        svx_ctx.lib.svx_bgzf_inflate_set_two_pass(was)
    for residue in (1, 6, 11):
        run_forms(svx_ctx, corpus, residue)


def test_slices_of_the_token_arena(svx_ctx, corpus):
    """svx_bgzf_inflate_set_arena(7): the call goes out in slices of seven members, so that the wave parse's give-ups and
    the lane parse's members land in different slices; statuses and bytes as in one slice."""
    was = svx_ctx.lib.svx_bgzf_inflate_set_arena(7)
    try:
        run_forms(svx_ctx, corpus, 3)
        # the same members in another order: each slice a different mix
        order = np.random.default_rng(9).permutation(len(corpus))
        run_forms(svx_ctx, [corpus[k] for k in order], 0)
    finally:
        svx_ctx.lib.svx_bgzf_inflate_set_arena(was)


def test_reader_device_leg_on_odd_encodings(svx_ctx, tmp_path):
    """A BAM from tests/spec_bam_writer.py whose members are written by the compressors of tests/deflate_writer.py (short
    end-of-block codes and 284 + 31 lengths, 15-bit codes and runs across HLIT / HDIST, stored blocks, codes that never
    resynchronise): the reader's device leg (every member on the device: device_inflate_percent 100, no minimum) returns
    the bases the host leg does and the bases the records were written with."""
    from svim_asm_amd import bamio
    from tests import spec_bam_writer as W
    rng = np.random.default_rng(17)
    refs = [("chrA", 5_000_000)]
    recs = []
    for i in range(60):
        n = int(rng.integers(500, 9000))
        seq = "".join(rng.choice(list("ACGTN"), size=n, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
        recs.append(dict(name="r%d" % i, flag=0, tid=0, pos=1000 + 60_000 * i, mapq=60, cigar=[(0, n)], seq=seq, tags=[]))
    path = str(tmp_path / "odd.bam")
    W.write_bam(path, refs, recs, chunk=20_000, compress=dw.compress_cycling())
    host = bamio.AlignmentFile(path, device=0)
    host.device_inflate_percent = 0
    host.load(None)
    assert len(host) == len(recs)
    idx, lo, hi = [], [], []
    for i, r in enumerate(recs):
        n = len(r["seq"])
        for _ in range(40):  # (the leg takes calls of 2 048 slices or more)
            a = int(rng.integers(0, n))
            idx.append(i); lo.append(a); hi.append(int(rng.integers(a + 1, n + 1)))
        idx.append(i); lo.append(0); hi.append(n)
    rec, a, b = np.array(idx, np.uint32), np.array(lo, np.int64), np.array(hi, np.int64)
    assert len(idx) >= 2048
    exp, exp_off = host.sequence_slices_raw(rec, a, b)
    assert host.device_members == 0
    assert list(host.sequence_slices(idx, lo, hi)) == [recs[i]["seq"][x:y] for i, x, y in zip(idx, lo, hi)]
    dev = bamio.AlignmentFile(path, device=0)
    dev.device_inflate_percent = 100
    dev.device_inflate_min_members = 0
    dev.load(None)
    import time
    for attempt in range(200):  # (the lanes come up beside the first load of the process: tens of milliseconds)
        got, got_off = dev.sequence_slices_raw(rec, a, b)
        assert np.array_equal(got_off, exp_off) and np.array_equal(got, exp)
        if dev.device_members:
            break
        time.sleep(0.05)
    assert dev.device_members > 0
    assert list(dev.sequence_slices(idx, lo, hi)) == [recs[i]["seq"][x:y] for i, x, y in zip(idx, lo, hi)]
