"""Plain Python restatement of what the edit distance's host plan (ed_run, svim_asm_amd/csrc/svx_editdist.hip) decides
per pair, and of the string a three-piece haplotype recipe denotes (include/svx.h).  Nothing here calls the code under
test: tests/editdist_cases.py uses it to build its table, tests/test_editdist_cases.py to show that the table holds
every state it claims, tests/test_gpu_editdist_cases.py for the strings k_hap_build has to write.

The constants are restated from svx.h (svx_ctx_set_edit_wavefront_cap: "min(k_max, max_edits, max(64, (|a| + |b|) /
32))") and from the kernel file's header comment (64-row blocks, strips of 64 blocks, bands that start at 256)."""

BLOCK = 64              # rows of the pattern one lane owns
STRIP = 64 * BLOCK      # rows one wave covers at a time (kStripRows)
EXACT = 0xFFFFFFFF      # k_max of an exact request, and the answer to a miss
FLOOR = 64              # the first stage always gets this many edits ...
LENGTH_SHARE = 32       # ... and 1/32 of the two lengths beyond it
FIRST_BAND = 256        # band of an exact request's first bit-vector round
WIDEN = 4               # ... and what each further round multiplies it by
UPPER, REVCOMP = 1, 2   # SVX_PIECE_UPPER, SVX_PIECE_REVCOMP

_COMPLEMENT = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}


def piece(pool, off, length, repeat, flags):
    """One piece: slice, ASCII upper-casing, reverse + complement of A/C/G/T only, repeat — in this order."""
    s = bytes(pool[off:off + length]) if length else b""
    if flags & UPPER:
        s = bytes(c - 32 if ord("a") <= c <= ord("z") else c for c in s)
    if flags & REVCOMP:
        s = bytes(_COMPLEMENT.get(c, c) for c in reversed(s))
    return s * repeat


def assemble(pool, pieces):
    """The bytes a haplotype recipe — three (off, len, repeat, flags) — denotes."""
    assert len(pieces) == 3
    return b"".join(piece(pool, int(o), int(l), int(r), int(f)) for o, l, r, f in pieces)


def length_bound(la, lb):
    return max(FLOOR, (la + lb) // LENGTH_SHARE)


def first_stage_cap(la, lb, k, wfa_cap):
    """Edits the wavefront pass runs for on a pair of lengths la, lb asked with threshold k (EXACT: none)."""
    cap = min(length_bound(la, lb), wfa_cap)
    return cap if k == EXACT else min(cap, k)


def binding(la, lb, k, wfa_cap):
    """Which of the terms of first_stage_cap decides it: the first that attains the minimum of "k", "wfa_cap",
    "floor", "length"."""
    cap = first_stage_cap(la, lb, k, wfa_cap)
    if k != EXACT and k == cap:
        return "k"
    if wfa_cap == cap:
        return "wfa_cap"
    return "floor" if cap == FLOOR else "length"


def first_band(la, lb, k, wfa_cap, resolved_by_wfa):
    """Band of the pair's first bit-vector round (None: there is none).  An exact request starts at 256, or at twice the
    cap the first stage failed at when that is more; a threshold request uses its threshold."""
    if wfa_cap > 0 and resolved_by_wfa:
        return None
    if k != EXACT:   # (a first stage that ran for k edits and failed has answered "> k" already)
        return None if wfa_cap > 0 and first_stage_cap(la, lb, k, wfa_cap) == k else k
    if wfa_cap == 0:
        return FIRST_BAND
    return max(FIRST_BAND, 2 * first_stage_cap(la, lb, k, wfa_cap))


def strips(la, lb):
    """Strips of the pattern — the longer side."""
    return (max(la, lb) + STRIP - 1) // STRIP
