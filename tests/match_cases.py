"""Seeded distance matrices for tests/test_gpu_match.py (and tools/match_probe.py's shapes are of the same families).

A family says how the values of an nb x nc matrix are drawn:
  ties       values from {0..3}, one cell in eight ineligible — edit distances tie constantly
  wide       full 32-bit values, one cell in eight ineligible
  edge       0xFFFFFFFE (the largest eligible distance) beside 0xFFFFFFFF (ineligible), half and half
  same_rows  every row the same permutation-like row: all bases want one comp, then the next
  none       nothing eligible
  last       only the last cell eligible
  equal      every cell 7
"""
import functools

import numpy as np

from tests import match_restatement

NONE = match_restatement.NONE
FAMILIES = ("ties", "wide", "edge", "same_rows")


@functools.lru_cache(maxsize=None)
def matrix(family, nb, nc):
    """The family's nb x nc matrix, flat and read-only (one array per case and session)."""
    rng = np.random.default_rng(100003 * nb + 17 * nc + sum(map(ord, family)))
    n = nb * nc
    if family == "ties":
        m = rng.integers(0, 4, n, dtype=np.uint32)
        m[rng.integers(0, 8, n) == 0] = NONE
    elif family == "wide":
        m = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        m[rng.integers(0, 8, n) == 0] = NONE
    elif family == "edge":
        m = np.where(rng.integers(0, 2, n) == 0, NONE - 1, NONE).astype(np.uint32)
    elif family == "same_rows":
        m = np.tile(rng.integers(0, max(2, nc // 2), nc, dtype=np.uint32), nb)
    elif family == "none":
        m = np.full(n, NONE, np.uint32)
    elif family == "last":
        m = np.full(n, NONE, np.uint32)
        if n:
            m[-1] = 5
    elif family == "equal":
        m = np.full(n, 7, np.uint32)
    else:
        raise ValueError(family)
    m = m.astype(np.uint32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected(family, nb, nc):
    """The restatement's answer for one partition, computed once per session."""
    mb, mc = match_restatement.match_one(matrix(family, nb, nc).tolist(), nb, nc)
    return tuple(mb), tuple(mc)


def batch(parts):
    """parts: (family, nb, nc) triples -> (dist, n_base, n_comp, want_base, want_comp)."""
    dist = np.concatenate([matrix(*p) for p in parts] + [np.zeros(0, np.uint32)])
    n_base = np.array([p[1] for p in parts], np.uint32)
    n_comp = np.array([p[2] for p in parts], np.uint32)
    want_base = [v for p in parts for v in expected(*p)[0]]
    want_comp = [v for p in parts for v in expected(*p)[1]]
    return dist, n_base, n_comp, want_base, want_comp


def many_parts(n_parts=100000):
    """1 x 1, 1 x 0 and 0 x 1 partitions with a dozen larger shapes interleaved."""
    larger = [("ties", 7, 5), ("wide", 33, 65), ("same_rows", 16, 16), ("ties", 1, 257), ("edge", 15, 17), ("wide", 2, 1),
              ("ties", 1, 2), ("equal", 3, 3), ("none", 64, 64), ("last", 129, 127), ("ties", 64, 64), ("wide", 40, 40)]
    small = [("ties", 1, 1), ("none", 1, 1), ("ties", 1, 0), ("ties", 0, 1), ("wide", 1, 1), ("ties", 1, 2), ("ties", 2, 1)]
    step = n_parts // len(larger)
    parts = []
    for k in range(n_parts):
        parts.append(larger[k // step] if k % step == step // 2 and k // step < len(larger) else small[(k * 7 + k // 11) % len(small)])
    return parts
