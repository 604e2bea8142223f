"""Greedy one-to-one assignment (svx_match_greedy_batch) stated once more in plain Python — the
yardstick of tests/test_gpu_match.py: sort the eligible pairs, scan them, nothing else."""
NONE = 0xFFFFFFFF


def match_one(dist, nb, nc):
    """dist: nb * nc integers, row-major.  Returns (match_base, match_comp) as lists."""
    pairs = sorted((int(dist[i * nc + j]), i, j) for i in range(nb) for j in range(nc) if int(dist[i * nc + j]) != NONE)
    mb, mc = [NONE] * nb, [NONE] * nc
    for _, i, j in pairs:
        if mb[i] == NONE and mc[j] == NONE:
            mb[i], mc[j] = j, i
    return mb, mc


def match_batch(dist, n_base, n_comp):
    """Partitions back to back, as the entry point takes and returns them."""
    mb, mc, at = [], [], 0
    for nb, nc in zip(n_base, n_comp):
        nb, nc = int(nb), int(nc)
        b, c = match_one(dist[at:at + nb * nc], nb, nc)
        mb += b
        mc += c
        at += nb * nc
    return mb, mc
