"""svx_cover_single on the device (svim_asm_amd/csrc/svx_cover.hip) against the plain loops of
tests/callable_restatement.py, element for element and seg_off included, on the cases of tests/callable_cases.py: the wave,
workgroup and pass edges and the carry across two and four passes in one call of fourteen lists; disjoint, duplicated,
abutting, equal-start and nested entries; both carried maxima; a segment in the open last slot alone; contig borders, contig
2^16 and position 2^31 - 1; an empty list between full ones; poisoned scratch; refused inputs — then `svim-asm diploid
--callable_bed` and `svim-asm-merge --callable_bed` end to end, held to the expectation of tests/test_callable_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from svim_asm_amd import _lib
from tests import callable_cases as K, callable_restatement as R, cover_cases, test_callable_host as host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arrays(lists):
    start = np.array([s for ivs in lists for s, _ in ivs], dtype=np.uint64)
    end = np.array([e for ivs in lists for _, e in ivs], dtype=np.uint64)
    off = np.zeros(len(lists) + 1, np.uint64)
    np.cumsum([len(ivs) for ivs in lists], out=off[1:])
    return start, end, off


def on_device(ctx, lists):
    lo, hi, off = ctx.cover_single(*arrays(lists))
    assert lo.dtype == hi.dtype == off.dtype == np.uint64 and len(off) == len(lists) + 1 and len(lo) == len(hi) == int(off[-1])
    return lo.tolist(), hi.tolist(), off.tolist()


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_case_equals_the_restatement(svx_ctx, name):
    lists = K.CASES[name]()
    K.check_inputs(lists)
    if name in K.MIXED:
        assert K.is_balanced(name)
    assert on_device(svx_ctx, lists) == K.answers(name)


def test_the_mixed_case_holds_the_edges_of_the_scan():
    assert [len(ivs) for ivs in K.mixed()] == [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097]
    assert K.CHUNK == 1024  # SVX_COVER_SCAN_CHUNK: 256 lanes of four slots


@pytest.mark.parametrize("n", K.MANY_LISTS)
def test_more_lists_than_one_pass_of_the_offsets(svx_ctx, n):
    """seg_off over CHUNK, CHUNK + 1 and 2 * CHUNK + 1 lists: the exclusive sum of the lists' counts carries its running
    count from one pass of CHUNK lists to the next.  By the restatement alone the count is above 0 at every pass border,
    grows from border to border and the lists around a border are not all empty: a carry that is dropped shows."""
    lists = K.many_lists(n)
    K.check_inputs(lists)
    lo, hi, off = K.many_lists_answers(n)
    assert len(lists) == n and [len(ivs) for ivs in lists[K.CHUNK - 1:K.CHUNK + 2]] == [3, 0, 1][:n - K.CHUNK + 1]
    assert sum(len(ivs) for ivs in lists) == len(lo) <= 3100
    borders = list(range(K.CHUNK, n, K.CHUNK))
    assert len(borders) == (n - 1) // K.CHUNK
    for b in borders:
        assert off[b] > off[b - K.CHUNK] and off[b - 1] < off[b]
    assert on_device(svx_ctx, lists) == (lo, hi, off)


def test_no_lists_and_lists_without_entries(svx_ctx):
    none = np.zeros(0, np.uint64)
    assert on_device(svx_ctx, []) == ([], [], [0])
    assert on_device(svx_ctx, [[], [], []]) == ([], [], [0, 0, 0, 0])
    with pytest.raises(_lib.SvxError):
        svx_ctx.cover_single(none, none, none)  # (no offsets at all)
    with pytest.raises(_lib.SvxError):
        svx_ctx.cover_single(np.ones(3, np.uint64), np.ones(2, np.uint64), np.array([0, 3], np.uint64))


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_answers_do_not_depend_on_what_scratch_held(svx_ctx, byte):
    assert on_device(svx_ctx, K.mixed()) == K.answers("mixed")  # (the regions exist from here on)
    for name in sorted(K.CASES):
        svx_ctx.scratch_fill(byte)
        assert on_device(svx_ctx, K.CASES[name]()) == K.answers(name), name


def test_every_case_directly_after_a_cover_query_of_another_size(svx_ctx):
    """The two entries share the workspace: what the prefix maxima of a query left there is not the single sweep's."""
    lists, queries = cover_cases.nested()
    q_lo, q_hi = (np.array([q[k] for q in queries], dtype=np.uint64) for k in (0, 1))
    for name in sorted(K.CASES):
        assert svx_ctx.cover_query(*arrays(lists), q_lo, q_hi).tolist() == cover_cases.answers("nested")
        assert on_device(svx_ctx, K.CASES[name]()) == K.answers(name), name


# what the message has to name
REFUSALS = {
    "list_off[0]": ("list_off[0] is 1",),
    "decreasing offsets": ("list 1",),
    "unsorted list": ("list 2", "entry 401"),
    "entry across contigs": ("list 0", "entry 17"),
    "empty entry": ("list 2", "entry 5"),
    "reversed entry": ("list 0", "entry 299"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_invalid_inputs_are_refused_by_list_and_entry_and_the_context_stays_usable(svx_ctx, what):
    lists = [list(ivs) for ivs in K.empty_between()]
    start, end, off = arrays(lists)
    if what == "list_off[0]":
        # (the binding's own shape check would catch a shifted end: straight to the entry)
        off = off.copy()
        off[0] = 1
    elif what == "decreasing offsets":
        off = off.copy()
        off[2] = off[1] - np.uint64(1)
    elif what == "unsorted list":
        lists[2][400], lists[2][401] = lists[2][401], lists[2][400]
        assert lists[2][400][0] > lists[2][401][0]
        start, end, off = arrays(lists)
    elif what == "entry across contigs":
        s, e = lists[0][17]
        lists[0][17] = (s, e + (1 << 32))
        start, end, off = arrays(lists)
    elif what == "empty entry":
        lists[2][5] = (lists[2][5][0], lists[2][5][0])
        start, end, off = arrays(lists)
    else:
        lists[0][299] = (lists[0][299][0], lists[0][299][0] - 1)
        start, end, off = arrays(lists)
    with pytest.raises(_lib.SvxError) as e:
        svx_ctx.cover_single(start, end, off)
    assert e.value.status == _lib.SVX_E_INVALID
    text = str(e.value)
    assert "svx_cover_single" in text
    for word in REFUSALS[what]:
        assert word in text, text
    assert on_device(svx_ctx, K.empty_between()) == K.answers("empty_between")


# ------------------------------------------------------------------------------ the commands
def _run(argv, timeout=120):
    env = dict(os.environ)
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SVX_NODE_PROCESSES"):
        env.pop(name, None)
    r = subprocess.run([sys.executable] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


@pytest.mark.spawns_gpu_children
def test_commands_end_to_end_write_the_restatements_files(tmp_path, svx_ctx):
    """s1 = (hap1, hap2) and s2 = (hap2, hap1) through `svim-asm diploid`, s3 = `svim-asm haploid` on hap1, then the merges —
    one in this process on its default context, one as the command: callable.bed of every sample and cohort.callable.bed,
    file for file."""
    from svim_asm_amd import merge_cli
    dirs = [str(tmp_path / n) for n in ("s1", "s2", "s3")]
    keep = ["--keep_candidates", "--keep_coverage", "--callable_bed"]
    _run([os.path.join(ROOT, "bin", "svim-asm"), "diploid", dirs[0], host.HAP1, host.HAP2, host.REF] + keep)
    _run([os.path.join(ROOT, "bin", "svim-asm"), "haploid", dirs[2], host.HAP1, host.REF] + keep)
    _run([os.path.join(ROOT, "bin", "svim-asm"), "diploid", dirs[1], host.HAP2, host.HAP1, host.REF] + keep)
    diploid = R.bed_text(host.CONTIGS, host.expected_set([host.HAP1, host.HAP2]))
    assert host.read(os.path.join(dirs[0], "callable.bed")) == diploid == host.read(os.path.join(dirs[1], "callable.bed"))
    assert host.read(os.path.join(dirs[2], "callable.bed")) == R.bed_text(host.CONTIGS, host.expected_set([host.HAP1]))
    assert diploid.count("\n") > 20
    assert merge_cli.main([str(tmp_path / "plain"), host.REF] + dirs) == 0
    assert merge_cli.main([str(tmp_path / "bed"), host.REF] + dirs + ["--callable_bed"]) == 0
    assert host.read(tmp_path / "bed" / "cohort.callable.bed") == R.bed_text(host.CONTIGS, host.expected_track())
    assert host.undated(tmp_path / "bed" / "cohort.vcf") == host.undated(tmp_path / "plain" / "cohort.vcf")
    n = sorted(e - s for _, s, e in host.python_intervals(host.HAP1))[10] + 1
    _run([os.path.join(ROOT, "bin", "svim-asm-merge"), str(tmp_path / "long"), host.REF] + dirs + ["--callable_bed", "--callable_min_length", str(n)])
    assert host.read(tmp_path / "long" / "cohort.callable.bed") == R.bed_text(host.CONTIGS, host.expected_track(n))
