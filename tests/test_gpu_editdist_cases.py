"""The edit distance's kernels and host plan (svim_asm_amd/csrc/svx_editdist.hip) held to the case table of
tests/editdist_cases.py: pairs on the first-stage cap and one to each side of it for every term that can decide it, on
k_edit_wfa's diagonal batches, clipped diagonals and run lengths at every pair of start addresses mod 8, on the exact
request's band rounds, the 16 | 17 and 255 | 256 symbol switch and the strip edges — against the oracle's full-matrix
distance —, and k_hap_build byte for byte against the restatement of tests/editdist_restatement.py.  What the table
holds is shown without a GPU by tests/test_editdist_cases.py.  Every comparison is integer equality; a miss of a
threshold is 0xFFFFFFFF (include/svx.h)."""
import numpy as np
import pytest

from tests import editdist_cases as E
from tests import editdist_restatement as R

pytestmark = pytest.mark.gpu

EXACT = R.EXACT
MISS = 0xFFFFFFFF


@pytest.fixture(autouse=True, params=["wavefront_1024", "wavefront_48", "bitvector_only"])
def edit_stage(request, svx_ctx):
    """As in tests/test_gpu_editdist.py: the default two-stage plan, a first stage so short that most pairs fall through
    to the bit-vector kernel, and the bit-vector kernel alone."""
    svx_ctx.set_edit_wavefront_cap({"wavefront_1024": 1024, "wavefront_48": 48, "bitvector_only": 0}[request.param])
    yield request.param
    svx_ctx.set_edit_wavefront_cap(1024)


@pytest.fixture(scope="module")
def table():
    """(names, pairs, reference distances): the oracle runs once per module."""
    ref = E.reference()
    return E.NAMES, [E.CASES[n] for n in E.NAMES], np.array([ref[n] for n in E.NAMES], dtype=np.int64)


def wrong(names, got, exp):
    return [(n, int(g), int(e)) for n, g, e in zip(names, got, exp) if int(g) != int(e)]


def thresholded(exp, k):
    k = np.broadcast_to(np.asarray(k, dtype=np.int64), exp.shape)
    return np.where((exp <= k) | (k == EXACT), exp, MISS)


LAYOUTS = {"adversarial": dict(), "zero_padding": dict(adversarial=False), "packed": dict(residues="packed")}


@pytest.mark.parametrize("how", sorted(LAYOUTS))
def test_exact(svx_ctx, table, how):
    names, pairs, exp = table
    got = svx_ctx.edit_distance_batch(*E.layout(pairs, **LAYOUTS[how]))
    assert wrong(names, got, exp) == []


@pytest.mark.parametrize("cap", [100, 1])
def test_exact_at_a_dedicated_cap(svx_ctx, table, cap):
    """(svx_ctx_set_edit_wavefront_cap(100): the table's 99 | 100 | 101 pairs; 1: the smallest first stage.  The module's
    fixture restores the default.)"""
    names, pairs, exp = table
    svx_ctx.set_edit_wavefront_cap(cap)
    assert wrong(names, svx_ctx.edit_distance_batch(*E.layout(pairs)), exp) == []
    k = 100
    assert wrong(names, svx_ctx.edit_distance_batch(*E.layout(pairs), k_max=k), thresholded(exp, k)) == []


def test_runs_at_every_pair_of_start_addresses(svx_ctx):
    """The run family once per (a's address mod 8, b's address mod 8): load8_unaligned's 8 x 8 shifts under match8 and
    coop_extend.  One batch (64 x 52 short pairs)."""
    ref = E.reference()
    names, pairs, residues = E.runs_at_every_residue()
    exp = np.array([ref[n] for n in names], dtype=np.int64)
    got = svx_ctx.edit_distance_batch(*E.layout(pairs, residues=residues))
    assert wrong(["%s@%d,%d" % ((n,) + r) for n, r in zip(names, residues)], got, exp) == []
    got = svx_ctx.edit_distance_batch(*E.layout(pairs, residues=residues), k_max=1)
    assert wrong(names, got, thresholded(exp, 1)) == []


def test_thresholds(svx_ctx, table):
    names, pairs, exp = table
    lay = E.layout(pairs)
    ks = E.thresholds(E.reference())
    assert set(E.FIXED_KS) <= set(ks)
    for k in ks:
        want = thresholded(exp, k)
        if k < exp.max():
            assert (want == MISS).any() and (want != MISS).any(), k
        assert wrong(names, svx_ctx.edit_distance_batch(*lay, k_max=k), want) == [], k


def single_piece_recipes(lay):
    from svim_asm_amd import _lib
    pool, ao, al, bo, bl = lay
    pieces = np.zeros(6 * len(ao), dtype=_lib.HAP_PIECE_DTYPE)
    for p, (xo, xl, yo, yl) in enumerate(zip(ao, al, bo, bl)):
        pieces[6 * p] = (xo, xl, 1, 0)
        pieces[6 * p + 3] = (yo, yl, 1, 0)
    return pool, pieces


def test_per_pair_thresholds(svx_ctx, table):
    """One submission of exact and thresholded pairs, fast and rich alphabets, one to three strips
    (svx_haplotype_distance_batch_mixed, each pair a single plain piece per side)."""
    names, pairs, exp = table
    pool, pieces = single_piece_recipes(E.layout(pairs))
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        ks = []
        for (a, b), d in zip(pairs, exp.tolist()):
            cap = R.first_stage_cap(len(a), len(b), EXACT, 1024)
            ks.append(int(rng.choice([EXACT, max(d - 1, 0), d, d + 1, cap - 1, cap + 1, 0, 1 << 31, 0xFFFFFFFE])))
        assert len(set(ks)) > 20 and ks.count(EXACT) > 5
        got = svx_ctx.haplotype_distance_batch_mixed(pool, pieces, np.array(ks, dtype=np.uint32))
        assert wrong(names, got, thresholded(exp, ks)) == [], seed


def test_order_independence(svx_ctx, table):
    names, pairs, exp = table
    got = svx_ctx.edit_distance_batch(*E.layout(pairs[::-1]))
    assert wrong(names[::-1], got, exp[::-1]) == []
    swapped = [(b, a) for a, b in pairs]
    assert wrong(names, svx_ctx.edit_distance_batch(*E.layout(swapped)), exp) == []
    k = 256
    assert wrong(names, svx_ctx.edit_distance_batch(*E.layout(swapped), k_max=k), thresholded(exp, k)) == []


def hap_batch():
    """Every recipe of HAP_CASES against one plain piece holding the expected string (appended to the pool): distance 0
    iff k_hap_build wrote exactly that string; the length forms once more against the string without its last byte."""
    from svim_asm_amd import _lib
    pool = [E.HAP_POOL.tobytes()]
    at = len(pool[0])
    rows, names, exp = [], [], []
    for name, recipe in E.HAP_CASES.items():
        s = E.hap_expected(name)
        for drop in ((0, 1) if name in E.HAP_LENGTH_FORMS else (0,)):
            rows += list(recipe) + [(at, len(s) - drop, 1, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
            names.append(name + ("" if not drop else "_less_one"))
            exp.append(drop)
        pool.append(s)
        at += len(s)
    pieces = np.zeros(len(rows), dtype=_lib.HAP_PIECE_DTYPE)
    for i, row in enumerate(rows):
        pieces[i] = row
    return np.frombuffer(b"".join(pool), np.uint8), pieces, names, exp


@pytest.mark.parametrize("form", ["host_pool", "dev_pool"])
def test_haplotype_assembly_byte_for_byte(svx_ctx, form):
    pool, pieces, names, exp = hap_batch()
    if form == "dev_pool":
        dev = svx_ctx.dev_array(pool)
        try:
            got = svx_ctx.haplotype_distance_batch(dev, pieces)
            thr = svx_ctx.haplotype_distance_batch(dev, pieces, 0)
        finally:
            dev.free()
    else:
        got = svx_ctx.haplotype_distance_batch(pool, pieces)
        thr = svx_ctx.haplotype_distance_batch(pool, pieces, 0)
    assert wrong(names, got, exp) == []
    assert wrong(names, thr, [0 if e == 0 else MISS for e in exp]) == []


def test_byte_classes(svx_ctx):
    """Every byte value as a one-byte piece under each flag combination against the restatement's byte as a plain
    piece: hap_byte's ranges and their neighbours, complement after upper-casing, the 252 bytes that stay."""
    from svim_asm_amd import _lib
    raw = bytes(range(256))
    want = b"".join(R.piece(raw, c, 1, 1, f) for f in range(4) for c in range(256))
    pool = np.frombuffer(raw + want, np.uint8)
    pieces = np.zeros(6 * 1024, dtype=_lib.HAP_PIECE_DTYPE)
    for f in range(4):
        for c in range(256):
            p = 256 * f + c
            pieces[6 * p + 1] = (c, 1, 1, f)                # (the middle piece of a, its flanks absent)
            pieces[6 * p + 3] = (256 + p, 1, 1, 0)
    got = svx_ctx.haplotype_distance_batch(pool, pieces)
    assert wrong(["byte %d flags %d" % (p % 256, p // 256) for p in range(1024)], got, np.zeros(1024, np.int64)) == []
    # (and a distance of 0 is not all this call can say: against the plain byte, exactly the changed ones differ)
    for p in range(1024):
        pieces[6 * p + 3] = (p % 256, 1, 1, 0)
    got = svx_ctx.haplotype_distance_batch(pool, pieces)
    assert got.tolist() == [int(want[p] != raw[p % 256]) for p in range(1024)]
