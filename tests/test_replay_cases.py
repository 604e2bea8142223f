"""The case table of svx_variant_replay (tests/replay_cases.py) where there is no GPU: every case shows what its name
promises; the table's constants are those of the header and the kernels; a constant moved by one makes the preconditions
fail; the restatement's strings are what the header's loop says, held to brute-force splicing on the cases' good jobs;
and no canary byte of the pool appears in an expected string."""
import os
import re

import pytest

from svim_asm_amd import _lib
from tests import replay_cases as T
from tests import replay_restatement as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_preconditions():
    assert T.check_preconditions() >= 80
    assert len(T.CASES) >= 30


def test_constants_are_those_of_the_header_and_the_kernels():
    def one(path, pattern):
        found = re.findall(pattern, open(os.path.join(ROOT, path)).read(), re.M)
        assert len(found) == 1, (pattern, found)
        return found[0]
    assert int(one("include/svx.h", r"^#define SVX_REPLAY_TILE (\d+)$")) == T.K["TILE"] == _lib.REPLAY_TILE
    assert int(one("include/svx.h", r"^#define SVX_REPLAY_MAX_BYTES (0x[0-9A-F]+)ull$"), 16) == _lib.REPLAY_MAX_BYTES
    assert int(one("svim_asm_amd/csrc/svx_scan_dev.h", r"^constexpr int kScanThreads = (\d+);")) == T.K["GROUP"]
    assert int(one("svim_asm_amd/csrc/svx_scan_dev.h", r"^constexpr int kScanPer = (\d+);")) * T.K["GROUP"] == T.K["CHUNK"]
    one("svim_asm_amd/csrc/svx_replay.hip", r"^constexpr int kBytes = SVX_REPLAY_TILE / kThreads;")
    one("svim_asm_amd/csrc/svx_replay.hip", r"^constexpr int kThreads = kScanThreads;")
    assert T.K["TILE"] // T.K["GROUP"] == T.K["LANE"]


@pytest.mark.parametrize("key", sorted(T.K))
@pytest.mark.parametrize("delta", (-1, 1))
def test_a_constant_moved_by_one_fails_the_preconditions(key, delta):
    k = dict(T.K)
    k[key] += delta
    with pytest.raises(AssertionError, match="does not show"):
        T.check_preconditions(k)


def test_the_header_states_the_loop_of_the_restatement():
    """The lines of the definition in include/svx.h, word for word: a change of the rule has to move both."""
    text = open(os.path.join(ROOT, "include", "svx.h")).read()
    for line in ("order  = false unless ed_start[e] >= p, and, for e not the job's first, ed_start[e] > ed_start[e - 1]",
                 "inside = false unless ed_start[e] + ed_ref_len[e] <= win_len[j]",
                 "string += win[p : ed_start[e]] + alt(e)",
                 "p = ed_start[e] + ed_ref_len[e]",
                 "string += win[p : win_len[j]]",
                 "status[j]  = 1 unless order, else 2 unless inside, else 0"):
        assert text.count(line) == 1, line


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_expected_strings_are_brute_force_splices_without_canaries(name):
    args, exp = T.case(name), T.expected(name)
    pool = bytes(bytearray(args[0]))
    assert b"!" not in exp["out"] and b"?" not in exp["out"]
    assert len(exp["out"]) == exp["total"] == sum(exp["out_len"]) and exp["total"] < 1 << 22
    for j, s in enumerate(exp["strings"]):
        if j >= 40 and j % 97:
            continue
        win = pool[int(args[1][j]):int(args[1][j]) + int(args[2][j])]
        edits = [(int(args[4][e]), int(args[5][e]), pool[int(args[6][e]):int(args[6][e]) + int(args[7][e])])
                 for e in range(int(args[3][j]), int(args[3][j + 1]))]
        if s is None:
            assert exp["status"][j] in (1, 2) and exp["out_len"][j] == 0
        else:
            assert s == RR.splice_brute(win, edits), (name, j)
        # every range lies between its canaries
        assert pool[int(args[1][j]) + len(win)] == ord("?") and (int(args[1][j]) == 0 or pool[int(args[1][j]) - 1] == ord("!"))
