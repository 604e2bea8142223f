"""svx_fasta_fetch_oriented (include/svx_text.h) on the host: plain and bgzip-compressed FASTA against a restatement in
five lines of Python — slice, reverse, complement table, BAM round-trip table."""
import numpy as np
import pytest

from tests import paf_writer as pw

_COMP = bytes.maketrans(b"ATCGMKRYVBHDatcgmkryvbhd", b"TAGCKMYRBVDHtagckmyrbvdh")
_BAM = bytes((c if chr(c) in "=ACMGRSVTWYHKDBN" else (c - 32 if chr(c) in "acmgrsvtwyhkdbn" else ord("N"))) for c in range(256))


def restated(seq, start, end, reverse, bam_alphabet):
    s = seq[start:min(end, len(seq))]
    if reverse:
        s = s[::-1].translate(_COMP)
    return s.translate(_BAM) if bam_alphabet else s


def sequences(seed=3):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTacgtNnRYKMSWBDHVrykmswbdhv=XxUu*-.", np.uint8)
    return {"c%d" % k: letters[rng.integers(0, len(letters), n)].tobytes() for k, n in enumerate((1, 59, 60, 61, 1000, 20011))}


def windows(seqs, seed):
    rng = np.random.default_rng(seed)
    names, start, end = [], [], []
    for name, s in seqs.items():
        n = len(s)
        for a, b in [(0, n), (0, 1), (n - 1, n), (n, n), (0, n + 50), (n // 2, n // 2)] + \
                [tuple(sorted(rng.integers(0, n + 1, 2).tolist())) for _ in range(40)]:
            names.append(name); start.append(a); end.append(b)
    return names, np.array(start), np.array(end), rng.integers(0, 2, len(names)).astype(bool)


@pytest.mark.parametrize("line", [1, 60, 0])
@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("bam_alphabet", [True, False])
def test_oriented_fetch_equals_the_restatement(tmp_path, line, compressed, bam_alphabet, monkeypatch):
    from svim_asm_amd import fasta
    monkeypatch.setenv("SVX_FASTA_DEVICE", "0")
    seqs = sequences()
    path = pw.write_fasta(str(tmp_path / "q.fa"), list(seqs), list(seqs.values()), line=line)
    if compressed:
        path = fasta.bgzip_fasta(path, path + ".gz", member_size=777)
    f = fasta.FastaFile(path)
    assert f.compressed == compressed
    names, start, end, rev = windows(seqs, 11)
    out, off = f.fetch_oriented(names, start, end, rev, bam_alphabet=bam_alphabet)
    for i, name in enumerate(names):
        exp = restated(seqs[name], int(start[i]), int(end[i]), bool(rev[i]), bam_alphabet)
        assert out[off[i]:off[i + 1]].tobytes() == exp, (name, int(start[i]), int(end[i]), bool(rev[i]))
    # no window reversed: the same call without the flags
    fwd, _ = f.fetch_oriented(names, start, end, np.zeros(len(names), bool), bam_alphabet=False)
    plain, _ = f.fetch_batch(names, start, end, upper=False)
    assert np.array_equal(fwd, plain)


def test_many_windows_take_the_threads(tmp_path):
    from svim_asm_amd import fasta
    seqs = sequences(5)
    path = pw.write_fasta(str(tmp_path / "q.fa"), list(seqs), list(seqs.values()), line=60)
    f = fasta.FastaFile(path)
    rng = np.random.default_rng(1)
    n = 3000
    start = rng.integers(0, 20000, n)
    end = start + rng.integers(0, 400, n)
    rev = rng.integers(0, 2, n).astype(bool)
    out, off = f.fetch_oriented(["c5"] * n, start, end, rev)
    for i in range(0, n, 7):
        assert out[off[i]:off[i + 1]].tobytes() == restated(seqs["c5"], int(start[i]), int(end[i]), bool(rev[i]), True)


def test_bad_windows_are_refused(tmp_path):
    from svim_asm_amd import fasta
    path = pw.write_fasta(str(tmp_path / "q.fa"), ["a"], [b"ACGT"], line=60)
    f = fasta.FastaFile(path)
    with pytest.raises(ValueError):
        f.fetch_oriented(["a"], [3], [2], [True])
    with pytest.raises(KeyError):
        f.fetch_oriented(["b"], [0], [2], [True])
