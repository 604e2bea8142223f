"""Plain-loop restatement of svx_cigar_mismatch (include/svx.h): the yardstick of
tests/test_gpu_mismatch.py and, through tests/small_restatement.py, of the svim-asm-small tests.  Python integers, lists
and one loop per column; shares no code with the product.

  mismatches(ops, ref_start, ref, qry)   [(ref_pos, qry_pos, R, Q)] of one alignment, R and Q upper-case byte values
  mismatch_batch(...)                    the entry point's arguments -> its five output columns as lists"""

REF_OPS = (0, 2, 3, 7, 8)  # M D N = X
QRY_OPS = (0, 1, 4, 7, 8)  # M I S = X
COLUMN_OPS = (0, 7, 8)     # M = X
ACGT = (0x41, 0x43, 0x47, 0x54)


def mismatches(ops, ref_start, ref, qry):
    """ops: [(code, length)]; ref: the bytes of the reference window from ref_start on, qry: the bytes of SEQ — each as
    long as its length argument says, nothing behind it is looked at."""
    out = []
    r = q = 0
    for code, n in ops:
        if code in COLUMN_OPS:
            # (the columns j with r + j < len(ref) and q + j < len(qry): a 2^27M op over 300 bases is 300 turns)
            for j in range(max(0, min(n, len(ref) - r, len(qry) - q))):
                R, Q = ref[r + j] & 0xDF, qry[q + j] & 0xDF
                if R in ACGT and Q in ACGT and R != Q:
                    out.append((ref_start + r + j, q + j, R, Q))
        if code in REF_OPS:
            r += n
        if code in QRY_OPS:
            q += n
    return out


def mismatch_batch(cigar, aln_off, ref_start, bases, ref_off, ref_len, qry_off, qry_len):
    bases = bytes(bytearray(bases))
    cols = {"aln": [], "ref_pos": [], "qry_pos": [], "ref_base": [], "qry_base": []}
    for a in range(len(aln_off) - 1):
        ops = [(int(w) & 15, int(w) >> 4) for w in cigar[int(aln_off[a]):int(aln_off[a + 1])]]
        ro, rl, qo, ql = int(ref_off[a]), int(ref_len[a]), int(qry_off[a]), int(qry_len[a])
        for ref_pos, qry_pos, R, Q in mismatches(ops, int(ref_start[a]), bases[ro:ro + rl], bases[qo:qo + ql]):
            cols["aln"].append(a)
            cols["ref_pos"].append(ref_pos)
            cols["qry_pos"].append(qry_pos)
            cols["ref_base"].append(R)
            cols["qry_base"].append(Q)
    return cols
