"""Cohorts with cohort-sized partitions for the merge tests (tests/test_merge_host.py where there is no GPU,
tests/test_gpu_merge.py on the device): seeded builders of per-sample candidate lists on the config-1 reference, the
expected answer of each from the restatement (tests/merge_restatement.py with the oracle's compiled full DP as its edit
distance), and the comparison both test modules make — records, genotype matrix and the condensed distance vectors the
product hands to its linkage call.

PAIR never clusters more than ten members; the merge sends all pairs of up to 1024 distinct alleles through the same
window / recipe / distance code and clusters them on the workgroup kernel.  The sizes here sit on the switches of that
path: 11 (first size PAIR never had; the lane kernel on HBM scratch), 17 (k_linkage_group at the default threshold),
33 and 65 (its second one-wave class, the four-wave LDS class), 129 (matrix in the workspace; 8256 jobs, which takes the
threaded branch of svx_pair_recipes) and 128 (8128 jobs: the other side of that switch).  Alleles lie 2-3 bp apart so
that the haplotype strings stay under about 700 bytes and the expected answer costs seconds, not minutes."""
import functools

import numpy as np

from tests import merge_restatement as R

SIZES = (11, 17, 33, 65, 129)
TYPES = ("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND")
GTS = ("1/1", "1/0", "0/1")
N_SAMPLES = 4


def _host():
    from tests import test_merge_host
    return test_merge_host


def _candidates():
    from svim_asm_amd import SVCandidate
    return SVCandidate


# ------------------------------------------------------------------------------ distinct alleles of one partition
# Every builder returns one callable per distinct allele: genotype -> a fresh Candidate object.
def dels(n, at=90000, seed=1, step=None, sizes=(40, 80)):
    """Deletions 2-3 bp apart (or `step`), lengths varied."""
    rng = np.random.default_rng(seed)
    size = rng.integers(sizes[0], sizes[1], n).tolist()
    start = [at + (k * step if step else (5 * k) // 2) for k in range(n)]
    return [lambda gt, s=s, z=z: _host().DEL(s, z, gt) for s, z in zip(start, size)]


def inss(n, at=30000, seed=2):
    """Insertions at a few positions within 5 bp: one 60-base seed with 0-5 substitutions and a homopolymer tail of 0-8
    bases, lower-case letters and N included; distinct in (position, bytes)."""
    rng = np.random.default_rng(seed)
    letters = "ACGTacgtN"
    base = "".join(rng.choice(list("ACGT"), 60).tolist())
    seen, out = set(), []
    while len(out) < n:
        seq = list(base)
        for p in rng.integers(0, 60, int(rng.integers(0, 6))).tolist():
            seq[p] = letters[int(rng.integers(0, len(letters)))]
        seq = "".join(seq) + letters[int(rng.integers(0, len(letters)))] * int(rng.integers(0, 9))
        pos = at + int(rng.integers(0, 5))
        if (pos, seq) not in seen:
            seen.add((pos, seq))
            out.append(lambda gt, pos=pos, seq=seq: _host().INS(pos, seq, gt))
    return out


def invs(n, at=20000, contig="chr10", length=300):
    """Inversions whose ends vary by 0-4 bp, both `complete` values (equal coordinates, different flag: distance 0)."""
    out = []
    for k in range(n):
        s = at + 5 * (k // 50) + (k // 2) % 5
        e = at + length + 5 * (k // 50) + (k // 10) % 5
        out.append(lambda gt, s=s, e=e, c=bool(k % 2): _candidates().CandidateInversion(contig, s, e, ["r"], c, _host().BAM, gt))
    return out


def dup_tans(n, at=40000, contig="chr2"):
    """Tandem duplications of 1-3 additional copies."""
    out = []
    for k in range(n):
        s = at + 2 * (k // 3)
        e = s + 100 + k % 4
        out.append(lambda gt, s=s, e=e, c=1 + k % 3, f=bool(k % 7): _candidates().CandidateDuplicationTandem(
            contig, s, e, c, f, ["r"], _host().BAM, gt))
    return out


def dup_ints(n, at=120000, seed=5):
    """Interspersed duplications into chr1 whose source intervals on chr2 vary in start and length."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        ss = 50000 + int(rng.integers(0, 40))
        ln = 150 + int(rng.integers(0, 30))
        d = at + 2 * k
        out.append(lambda gt, ss=ss, ln=ln, d=d: _candidates().CandidateDuplicationInterspersed(
            "chr2", ss, ss + ln, "chr1", d, d + ln, ["r"], _host().BAM, False, gt))
    return out


def bnds(n, at=60000, seed=6):
    """Breakends 3 bp apart with both direction pairs; destinations spread over 1200 bp, so that the span-position
    distances (|source difference| + |destination difference|) / 3000 fall on either side of 0.3."""
    rng = np.random.default_rng(seed)
    dest = (7000 + rng.integers(0, 1200, n)).tolist()
    return [lambda gt, p=at + 3 * k, d=d, sd=("fwd", "rev")[k % 2]: _host().BND(p, d, sd, "fwd", gt) for k, d in enumerate(dest)]


BUILDERS = {"DEL": dels, "INS": inss, "INV": invs, "DUP_TAN": dup_tans, "DUP_INT": dup_ints, "BND": bnds}


def spread(makers, samples=None):
    """The distinct alleles dealt over four samples, genotypes cycling through 1/1, 1/0, 0/1; every fifth allele appears
    again, byte for byte, in one or two other samples (collapse and carrier counts are in play)."""
    samples = samples if samples is not None else [[] for _ in range(N_SAMPLES)]
    for k, make in enumerate(makers):
        samples[k % N_SAMPLES].append(make(GTS[k % 3]))
        if k % 5 == 0:
            for extra in range(1, 2 + k % 2):
                samples[(k + extra) % N_SAMPLES].append(make(GTS[(k + extra) % 3]))
    return samples


# ------------------------------------------------------------------------------ the cases
# max_edit_distance per case: where the restatement clusters the partition non-trivially (1 < records < distinct
# alleles, a cluster of three or more) — a condition on the inputs above, asserted by tests/test_merge_host.py.
# Breakends are cut at 0.3 whatever the option says.
CUTS = {"DEL": 30, "INS": 8, "INV": 6, "DUP_TAN": 60, "DUP_INT": 25, "BND": 200}
EVERYTHING_CUT = 25
WIDE_CUT = 110
CHUNKS_CUT = 8
# partition sizes of the "everything" cohort: every type in one call; its non-breakend linkage call mixes the lane kernel
# (1-10 members), the lane kernel on HBM scratch (11, 15) and the group classes of 16-32, 33-64, 65-128 and 129-512 members
EVERYTHING = (("DEL", (65, 2, 15)), ("INS", (129, 1, 11)), ("INV", (17, 3)), ("DUP_TAN", (33, 10)), ("DUP_INT", (16, 1)),
              ("BND", (3, 2)))
_BASE = {"DEL": 90000, "INS": 30000, "INV": 20000, "DUP_TAN": 40000, "DUP_INT": 120000, "BND": 60000}


def sized(typ, n):
    """Four samples, one partition of n distinct alleles of one type."""
    return spread(BUILDERS[typ](n))


def everything():
    samples = [[] for _ in range(N_SAMPLES)]
    for typ, sizes in EVERYTHING:
        for i, n in enumerate(sizes):
            spread(BUILDERS[typ](n, at=_BASE[typ] + 4000 * i), samples)
    return samples


def wide():
    """17 deletions 600 bp apart: one partition, a window of about 10 kb — pairs of the length PAIR's ten members never
    exceeded.  (Expected distances by the oracle's band-doubling DP: the full matrix of 136 such pairs takes minutes.)"""
    return spread(dels(17, at=100000, seed=7, step=600, sizes=(40, 75)))


def chunks():
    """One partition of 33 insertions between a dozen partitions of 2-3 alleles, insertions on either side of it: with
    the jobs cut into chunks of whole partitions (SVIM_COMBINE._job_distances) the large partition fills one chunk and
    the chunks before and after each append their own stretch of the sequence pool."""
    samples = [[] for _ in range(N_SAMPLES)]
    small = (("DEL", 90000, 2), ("DEL", 94000, 3), ("DEL", 98000, 2), ("INV", 20000, 3), ("INV", 24000, 2),
             ("INS", 22000, 3), ("INS", 26000, 2), ("INS", 38000, 2), ("INS", 42000, 3), ("DUP_TAN", 40000, 3),
             ("DUP_TAN", 44000, 2), ("DUP_INT", 120000, 2))
    for typ, at, n in small:
        spread(BUILDERS[typ](n, at=at), samples)
    spread(inss(33, at=30000, seed=8), samples)
    return samples


def build(case):
    """case: (type, n), "everything", "wide" or "chunks" -> (samples, max_edit_distance)."""
    if case == "everything":
        return everything(), EVERYTHING_CUT
    if case == "wide":
        return wide(), WIDE_CUT
    if case == "chunks":
        return chunks(), CHUNKS_CUT
    typ, n = case
    return sized(typ, n), CUTS[typ]


def _oracle_distance(case):
    from oracle import orc
    return orc.edit_distance_banded if case == "wide" else orc.edit_distance


@functools.lru_cache(maxsize=None)
def expected(case):
    """(records, [(type, allele keys, condensed vector)] per clustered partition) of the restatement; computed once per
    process and shared by the tests, which leave it unchanged."""
    samples, cut = build(case)
    recorded = []
    records, unclustered = R.merge(samples, _host().SEQS, 1000, cut, 1024, edit_distance=_oracle_distance(case), record=recorded)
    assert unclustered == 0
    return records, recorded


def cut_of(typ, cut):
    return 0.3 if typ == "BND" else float(cut)


def cluster_sizes(case):
    """Members per flat cluster of every clustered partition of the expected answer (scipy on the recorded vectors)."""
    from scipy.cluster.hierarchy import fcluster, linkage
    _, cut = build(case)
    out = []
    for typ, keys, cond in expected(case)[1]:
        labels = fcluster(linkage(np.array(cond), method="complete"), cut_of(typ, cut), criterion="distance")
        out.extend(np.bincount(labels)[1:].tolist())
    return out


def is_non_trivial(case):
    """1 < records < distinct alleles, and a cluster of three or more members."""
    samples, _ = build(case)
    distinct = len({R.allele_key(c) for s in samples for c in s})
    return 1 < len(expected(case)[0]) < distinct and max(cluster_sizes(case)) >= 3


# ------------------------------------------------------------------------------ the comparison
class Recording(object):
    """A context that delegates everything and keeps the arguments of its linkage and distance calls."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.linkage = []  # (dist, n_members, cutoff) per linkage_cut_batch call
        self.distance_jobs = []  # pairs per haplotype_distance_batch_mixed call

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def linkage_cut_batch(self, dist, n_members, cutoff):
        self.linkage.append((np.array(dist, np.float64), np.array(n_members, np.int64), float(cutoff)))
        return self._ctx.linkage_cut_batch(dist, n_members, cutoff)

    def haplotype_distance_batch_mixed(self, pool, pieces, k_max):
        self.distance_jobs.append(len(k_max))
        return self._ctx.haplotype_distance_batch_mixed(pool, pieces, k_max)

    def vectors(self):
        """[(condensed vector, cut-off)] per clustered partition, in the order of the calls."""
        out = []
        for dist, n_members, cutoff in self.linkage:
            at = 0
            for n in n_members.tolist():
                m = n * (n - 1) // 2
                out.append((dist[at:at + m].tolist(), cutoff))
                at += m
            assert at == len(dist)
        return out


def merged(case, ctx):
    """merge_tables on `ctx` through the recording proxy -> (merged table, genotype matrix, options, recording)."""
    from svim_asm_amd import SVIM_MERGE
    from svim_asm_amd.fasta import FastaFile
    from svim_asm_amd.table import CandidateTable
    from tests import helpers
    host = _host()
    samples, cut = build(case)
    proxy = Recording(ctx)
    options = helpers.options(max_edit_distance=cut)
    tables = [CandidateTable.from_objects(s, host.BAM) for s in samples]
    table, G = SVIM_MERGE.merge_tables(tables, host.SAMPLES, FastaFile(host.REF), options, ctx=proxy)
    assert G.shape == (len(table), N_SAMPLES)
    return table, G, options, proxy


def run(case, ctx):
    """merge_tables on `ctx` -> (records as the restatement writes them, recording)."""
    from svim_asm_amd import SVIM_MERGE
    table, G, _, proxy = merged(case, ctx)
    got = [(R.allele_key(c), [SVIM_MERGE.GT_TEXT[g] for g in row]) for c, row in zip(table.objects(), G.tolist())]
    return got, proxy


def check(case, ctx):
    """Records and genotype matrix equal the restatement's, and so does every condensed vector handed to the linkage
    call, element for element in partition order: a wrong exact distance that leaves the flat clusters in place still
    fails here.  One rule for two-member partitions: the product only asks "within the threshold?" there and answers
    "no" with threshold + 1, so a value over the cut on one side must be over the cut on the other, and a value within
    it must be equal."""
    got, proxy = run(case, ctx)
    exp_records, exp_vectors = expected(case)
    _, cut = build(case)
    vectors = proxy.vectors()
    assert len(vectors) == len(exp_vectors)
    for (vec, cutoff), (typ, keys, exp) in zip(vectors, exp_vectors):
        assert cutoff == cut_of(typ, cut)
        assert len(vec) == len(exp) == len(keys) * (len(keys) - 1) // 2
        if len(keys) == 2 and exp[0] > cutoff:
            assert vec[0] > cutoff, (typ, keys)
        else:
            assert vec == exp, (typ, keys[0], len(keys))
    assert got == exp_records
    return got, proxy
