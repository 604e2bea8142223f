"""tests/segments_restatement.py and the case table of tests/segments_cases.py (no GPU): the restatement agrees with
the C oracle (orc.segments_classify) and the Python oracle (svim_oracle.postpass_records), both of which are pinned to
recorded vectors of the real reference by tests/test_oracle_pins.py; every case reaches the leaf it names; the table
reaches both sides of every comparison and -1 | 0 | +1 around every threshold; and a comparison evaluated wrongly
(strictness flipped, another tolerance, min_sv_size for max_sv_size) changes the record of at least one case.
tests/test_gpu_segments_cases.py holds the device forms to the same table."""
import numpy as np
import pytest

from oracle import orc, svim_oracle
from tests import segments_cases as SC, segments_restatement as R
from tests.test_gpu_segments import _random_raw_read, random_reads

TABLES = {name: SC.tree_cases(prm) for name, prm in SC.PARAM_SETS.items()}

# What one parameter set cannot show, and why.  Over the three sets together nothing of the tree is left out.
ONLY_WITH_AN_EMPTY_WINDOW = {
    # :131 `deviation < -max_sv_size` is looked at behind a failed `-max_sv_size <= deviation <= -min_sv_size` (:123) and a
    # failed `deviation >= min_sv_size` (:113).  With min_sv_size <= max_sv_size, deviation = -max_sv_size and -max_sv_size + 1
    # are inside the window of :123, so lhs - rhs = 0 and +1 never get here; ZERO (min 50 > max 20) shows both.  For
    # the same reason flipping `<` to `<=` or reading min_sv_size changes nothing unless the window is empty.
    "same.bnd.max": {0, 1},
}
# The post-passes: what the reference itself rules out (two ids).
POST_UNREACHABLE = {
    # :28 `start1 >= end2`: the pairs come from a list sorted by start (:323), so start1 <= start2, and start2 < end2
    # because an inversion's end is its start plus a size of at least min_sv_size > 0.  Never true; lhs - rhs <= -1.
    "dist.apart2": {"True", 0, 1},
    # :31 `start2 >= start1`: the same sort.  Never false; lhs - rhs >= 0.
    "dist.left": {"False", -1},
}
# Mutants that compute the same function (so no case can tell them apart).
POST_EQUIVALENT = {
    ("dist.apart2", "flip_strict"),  # never true either way (above)
    ("dist.left", "flip_strict"),    # start2 == start1: both branches subtract the same start
    ("dist.apart1", "flip_strict"),  # start2 == end1: the overlap is 0 and the distance 1 - 0 / ... = 1, what :27 returns
}


def observations(trace):
    seen = {}
    for cid, outcome, diff in trace:
        s = seen.setdefault(cid, set())
        s.add(str(outcome))
        if R.COMPARISONS[cid][0] != "==":
            s.add(diff)
    return seen


def needed(cid):
    return {"True", "False"} | ({-1, 0, 1} if R.COMPARISONS[cid][0] != "==" else set())


def tree_trace(name):
    trace = []
    for rd in SC.pairs(TABLES[name]):
        R.classify_read(rd["segs"], rd["read_len"], SC.PARAM_SETS[name], trace)
    return observations(trace)


def shapes(name):
    cases = TABLES[name]
    return dict(pairs=SC.pairs(cases), packed=SC.packed(cases, 33), chains=SC.chains(cases), ties=SC.ties(cases),
                mirrored=SC.mirrored())


@pytest.mark.parametrize("name", list(SC.PARAM_SETS))
def test_restatement_equals_the_c_oracle_on_every_table(name):
    prm = SC.PARAM_SETS[name]
    for shape, reads in shapes(name).items():
        segs, off, rl = SC.to_arrays(reads, orc.SEG_DTYPE)
        assert segs["ref_start"].min() >= 0 and (segs["ref_end"] - segs["ref_start"] == segs["q_end"] - segs["q_start"]).all()
        exp = orc.segments_classify(segs, off, rl, prm).view(np.int32).reshape(-1, 8)
        got = SC.expected_raw(reads, prm)
        assert np.array_equal(got, exp), (shape, np.nonzero((got != exp).any(axis=1))[0][:5])
        lens = [rd["read_len"] for rd in reads]  # a lane with the length of another read of its workgroup shows
        assert all(lens[i] not in lens[max(0, i - 32):i] for i in range(len(lens))), shape


@pytest.mark.parametrize("seed", range(5))
def test_restatement_equals_the_c_oracle_on_random_reads(seed):
    rng = np.random.default_rng(seed)
    segs, off, rl = random_reads(rng, n_reads=300, max_k=int(rng.choice([2, 6, 40, 90])))
    for prm in list(SC.PARAM_SETS.values()) + [(1, 100000, 500, 500, 500, 500)]:
        exp = orc.segments_classify(segs, off, rl, prm).view(np.int32).reshape(-1, 8)
        reads = [dict(segs=[R.Seg(*(int(v) for v in s)) for s in segs[off[r]:off[r + 1]]], read_len=int(rl[r]))
                 for r in range(len(rl))]
        assert np.array_equal(SC.expected_raw(reads, prm), exp)


@pytest.mark.parametrize("name", list(SC.PARAM_SETS))
def test_every_case_reaches_its_leaf(name):
    """Alone and inside a chain, where the segments arrive shuffled and the sort has to restore the order of
    construction (no gap or short segment may have turned two segments round)."""
    prm, cases = SC.PARAM_SETS[name], TABLES[name]
    for c, rd in zip(cases, SC.pairs(cases)):
        leaves = []
        R.classify_read(rd["segs"], rd["read_len"], prm, leaves=leaves)
        assert leaves == [c.leaf], (c.name, leaves)
    for rd in SC.chains(cases):
        leaves = []
        R.classify_read(rd["segs"], rd["read_len"], prm, leaves=leaves)
        assert leaves == [cases[i].leaf for i in rd["steps"]], [cases[i].name for i in rd["steps"]]
    assert {c.leaf for c in cases} >= set(["none", "ins.fwd", "ins.rev", "bnd.fwd", "bnd.rev", "dup_full.fwd", "dup_full.rev",
                                           "dup_bnd.fwd", "dup_bnd.rev", "inv1_bnd", "inv2_bnd", "inv3_bnd", "inv4_bnd",
                                           "other.ff", "other.fr", "other.rf", "other.rr"])
    if name != "ZERO":
        assert {c.leaf for c in cases} >= set(["del.fwd", "del.rev", "dup_part.fwd", "dup_part.rev", "inv1", "inv2", "inv3", "inv4"])


def test_chains_use_every_case_on_either_path():
    for name, cases in TABLES.items():
        used = {"shuffle": set(), "serial": set()}
        sizes = {"shuffle": set(), "serial": set()}
        for rd in SC.chains(cases):
            path = "shuffle" if len(rd["segs"]) <= 8 else "serial"
            used[path] |= set(rd["steps"])
            sizes[path].add(len(rd["segs"]))
            assert R.sort_segments(rd["segs"]) != rd["segs"] or len(rd["segs"]) < 4  # handed over shuffled
        assert used["shuffle"] == set(range(len(cases))) == used["serial"], name
        assert sizes["shuffle"] == set(SC.SHUFFLE_SIZES) and sizes["serial"] == set(SC.SERIAL_SIZES)


def test_ties_are_decided_by_the_input_order():
    """The same segments in another order give other pairs: the tables hold reads that differ in nothing else."""
    prm = SC.DEFAULT
    reads = SC.ties(TABLES["DEFAULT"])
    by_content = {}
    for rd in reads:
        by_content.setdefault(tuple(sorted(rd["segs"])), set()).add(tuple(R.classify_read(rd["segs"], 10 ** 6, prm)))
    assert len(by_content) == 9 and all(len(v) >= 2 for v in by_content.values())
    tied = {max(sum(1 for s in rd["segs"] if (s.q_start, s.q_end) == (t.q_start, t.q_end)) for t in rd["segs"]) for rd in reads}
    assert tied == {2, 3, 8}
    assert {len(rd["segs"]) <= 8 for rd in reads} == {True, False}


def test_mirrored_reads_give_interspersed_duplications():
    for name, prm in SC.PARAM_SETS.items():
        n = [len([t for t in R.postpass_read(R.classify_read(rd["segs"], rd["read_len"], prm), SC.CONTIG_RANK, prm[0], prm[1])
                  if t[0] == "DUP_INT"]) for rd in SC.mirrored()]
        assert n == ([0, 1, 1, 1, 0] * 2 if name != "ZERO" else [0] * 10), name


@pytest.mark.parametrize("name", ["DEFAULT", "DISTINCT"])
def test_tree_coverage_of_one_parameter_set(name):
    seen = tree_trace(name)
    for cid in R.TREE_IDS:
        missing = needed(cid) - seen.get(cid, set())
        assert missing == ONLY_WITH_AN_EMPTY_WINDOW.get(cid, set()), (cid, missing)


def test_tree_coverage_has_no_exemption():
    seen = {}
    for name in SC.PARAM_SETS:
        for cid, s in tree_trace(name).items():
            seen.setdefault(cid, set()).update(s)
    assert sorted(seen) == sorted(R.TREE_IDS)
    for cid in R.TREE_IDS:
        assert needed(cid) <= seen[cid], (cid, needed(cid) - seen[cid])


def tree_mutants(name, hows):
    """(killed, survivors) among the mutants of the tree whose `how` starts with one of `hows`, on the `pairs` of `name`."""
    prm = SC.PARAM_SETS[name]
    reads = SC.pairs(TABLES[name])
    base, touched = [], []
    for rd in reads:
        trace = []
        base.append(R.classify_read(rd["segs"], rd["read_len"], prm, trace))
        touched.append({t[0] for t in trace})
    killed, survivors = [], []
    for cid in R.TREE_IDS:
        for m in R.mutants_of(cid):
            if not m[1].startswith(hows):
                continue
            dead = any(cid in t and R.classify_read(rd["segs"], rd["read_len"], prm, None, m) != b
                       for rd, b, t in zip(reads, base, touched))
            (killed if dead else survivors).append(m)
    return killed, survivors


def test_tree_mutation_adequacy():
    empty_window_only = {(cid, how) for cid in ONLY_WITH_AN_EMPTY_WINDOW for how in ("flip_strict", "min_max")}
    killed, survivors = tree_mutants("DISTINCT", ("flip_strict", "other_tolerance", "min_max"))
    print("DISTINCT: %d of %d mutants killed" % (len(killed), len(killed) + len(survivors)))
    assert set(survivors) == empty_window_only, survivors
    assert any(m[1].startswith("other_tolerance") for m in killed) and len(killed) >= 100
    killed, survivors = tree_mutants("DEFAULT", ("flip_strict", "min_max"))
    print("DEFAULT: %d of %d mutants killed" % (len(killed), len(killed) + len(survivors)))
    assert set(survivors) == empty_window_only, survivors
    # the equal tolerances of DEFAULT are why DISTINCT exists: there not one of these mutants shows
    assert tree_mutants("DEFAULT", ("other_tolerance",))[0] == []
    killed, survivors = tree_mutants("ZERO", ("flip_strict", "min_max"))
    print("ZERO: %d of %d mutants killed" % (len(killed), len(killed) + len(survivors)))
    assert empty_window_only <= set(killed)


# ------------------------------------------------------------------------------------------ post-passes
@pytest.mark.parametrize("prm", SC.POST_PARAMS)
def test_postpass_restatement_equals_the_python_oracle_on_the_table(prm):
    kinds = set()
    for name, raw in SC.postpass_cases(*prm):
        got = R.postpass_read(raw, SC.POST_RANK, *prm)
        assert got == svim_oracle.postpass_records(raw, SC.POST_RANK, *prm), name
        kinds |= {t[0] for t in got}
    assert kinds == {"TANDEM", "DUP_INT", "INV"}


def test_postpass_table_says_what_the_issue_lists():
    """A few of the table's answers by hand, so that the table cannot drift into cases that no longer bite."""
    cases = dict(SC.postpass_cases(40, 100000))
    post = lambda name: R.postpass_read(cases[name], SC.POST_RANK, 40, 100000)
    assert len(post("tandem.second+19+0")) == 1 and len(post("tandem.second+20+0")) == 2
    assert len(post("tandem.second+0-19")) == 1 and len(post("tandem.second+0-20")) == 2
    assert len(post("tandem.count2.start[0, 1]+20")) == 1 and len(post("tandem.count2.start[0, 1]+21")) == 2  # 19.5 | 20.5
    assert len(post("tandem.count3.end[0, 1, 1]-19")) == 1 and len(post("tandem.count3.end[0, 1, 1]-20")) == 2
    assert [t[4] for t in post("tandem.stale_direction.joins")] == [1, 2]
    assert [t[4] for t in post("tandem.stale_direction.splits")] == [1, 1, 1]
    assert [t[5] for t in post("tandem.fully.third")] == [True, False]
    assert post("tandem.truncate")[0][2:4] == (10000, 10100) and post("tandem.truncate")[1][2:4] == (10500, 10100)
    assert len(post("mirror.fwd.near+19")) == 1 and post("mirror.fwd.near+20") == []
    assert len(post("mirror.rev.near-19")) == 1 and post("mirror.rev.near-20") == []
    for name in ("fwd", "rev"):
        assert [len(post("mirror.%s.length%d" % (name, n))) for n in (39, 40, 100000, 100001)] == [0, 1, 1, 0]
        for broken in ("dir1", "dir2", "chrom", "origin", "same_dir"):
            assert post("mirror.%s.%s" % (name, broken)) == []
        assert len(post("mirror.%s.two_before" % name)) == 2
    assert post("inv.overlap+0") == post("inv.overlap+1") != post("inv.overlap-1")  # 199 joins; 200 and 201 close, and are dropped
    assert post("inv.dropped_then_new") == [("INV", 0, 100, 200, False), ("INV", 0, 260, 340, True)]
    assert post("inv.dropped_last") == [("INV", 0, 120, 200, True)]
    # chr10 in front of chr2; the change of contig closes the group, so contig 1's first breakpoint is dropped too
    assert post("inv.str_rank") == [("INV", 9, 120, 200, True), ("INV", 1, 110, 210, False)]
    assert post("inv.ratio.7/10") == [("INV", 0, 1000, 1010, False), ("INV", 0, 1003, 1013, False)]
    assert len(post("inv.ratio.70/100")) == 2 and post("inv.ratio.3/4") == [("INV", 0, 1001, 1004, True)]
    assert all(t[4] is False for t in post("inv.same_side")) and len(post("inv.same_side")) == 4
    assert 1 - 7 / float(10) == 0.30000000000000004 == 1 - 70 / float(100) and 1 - 3 / float(4) == 0.25


@pytest.mark.parametrize("seed", range(4))
def test_postpass_restatement_equals_the_python_oracle_on_random_records(seed):
    rng = np.random.default_rng(40 + seed)
    for _ in range(300):
        raw = _random_raw_read(rng, int(rng.integers(0, 14)), SC.POST_CONTIGS, bool(rng.random() < 0.7))
        for prm in SC.POST_PARAMS:
            assert R.postpass_read(raw, SC.POST_RANK, *prm) == svim_oracle.postpass_records(raw, SC.POST_RANK, *prm)


def post_trace():
    trace = []
    for prm in SC.POST_PARAMS:
        for _, raw in SC.postpass_cases(*prm):
            R.postpass_read(raw, SC.POST_RANK, prm[0], prm[1], trace)
    return observations(trace)


def test_postpass_coverage():
    seen = post_trace()
    for cid in R.POST_IDS:
        missing = needed(cid) - seen.get(cid, set())
        assert missing == POST_UNREACHABLE.get(cid, set()), (cid, missing)
    assert len(POST_UNREACHABLE) <= 3  # (and the tree has none: test_tree_coverage_has_no_exemption)


def test_postpass_mutation_adequacy():
    killed, survivors = [], []
    for cid in R.POST_IDS:
        for m in R.mutants_of(cid):
            dead = False
            for prm in SC.POST_PARAMS:
                for _, raw in SC.postpass_cases(*prm):
                    if R.postpass_read(raw, SC.POST_RANK, prm[0], prm[1], None, m) != R.postpass_read(raw, SC.POST_RANK, *prm):
                        dead = True
            (killed if dead else survivors).append(m)
    print("post-passes: %d of %d mutants killed" % (len(killed), len(killed) + len(survivors)))
    assert set(survivors) == POST_EQUIVALENT, survivors


def test_the_figures_the_table_stands_for():
    """Counts that the pull request states: a change of the table shows here."""
    print("comparison ids: %d in the tree, %d in the post-passes" % (len(R.TREE_IDS), len(R.POST_IDS)))
    for name, cases in TABLES.items():
        sh = shapes(name)
        print(name, "cases", len(cases), {k: len(v) for k, v in sh.items()})
    for prm in SC.POST_PARAMS:
        print("post-pass cases", prm, len(SC.postpass_cases(*prm)))
    assert len(R.TREE_IDS) == 47 and len(R.POST_IDS) == 24
    assert [len(c) for c in TABLES.values()] == [144, 144, 126]
