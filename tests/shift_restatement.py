"""Plain-loop restatement of svx_indel_shift (include/svx.h) and of what `svim-asm-small --left_align`
does with it: the yardstick of tests/test_shift_restatement.py, tests/test_gpu_shift.py and the left-align command tests.
Python bytes, tuples and loops; it shares no code with the product."""
from tests import mismatch_restatement as MM

INS, DEL = 0, 1  # svx_cigar_extract's type codes
ACGT = (65, 67, 71, 84)


def shift_of(ref, qry, r, q, length, kind, limit):
    """The loop of include/svx.h on one event: `ref` and `qry` are the alignment's two ranges as bytes."""
    k = 0
    while k < limit:
        i = k + 1
        if not (i <= r and i <= q and r - i < len(ref) and q - i < len(qry)):
            break
        R, Q = ref[r - i] & 0xDF, qry[q - i] & 0xDF
        if R not in ACGT or R != Q:
            break
        if kind == INS:
            if not q + length - i < len(qry):
                break
            X = qry[q + length - i] & 0xDF
        else:
            if not r + length - i < len(ref):
                break
            X = ref[r + length - i] & 0xDF
        if X != R:
            break
        k = i
    return k


def shift_batch(bases, ref_off, ref_len, qry_off, qry_len, ref_start, aln, ref_pos, qry_pos, length, kind, limit):
    """The entry point's arguments, event by event."""
    bases = bytes(bytearray(bases))
    out = []
    for e in range(len(aln)):
        a = int(aln[e])
        ref = bases[int(ref_off[a]):int(ref_off[a]) + int(ref_len[a])]
        qry = bases[int(qry_off[a]):int(qry_off[a]) + int(qry_len[a])]
        out.append(shift_of(ref, qry, int(ref_pos[e]) - int(ref_start[a]), int(qry_pos[e]), int(length[e]), int(kind[e]), int(limit[e])))
    return out


def gaps_of(start, ops):
    """Every I and D op of an alignment in its original placement: (op index, r, q, length, kind, limit) with r and q the
    cursors inside the alignment — the limit keeps one aligned column between a gap and the gap (or the start) in front."""
    out, r, q, prev_end = [], 0, 0, 0
    for j, (op, n) in enumerate(ops):
        if op in (1, 2):
            out.append((j, r, q, n, INS if op == 1 else DEL, max(0, r - prev_end - 1)))
            prev_end = r + (n if op == 2 else 0)
        if op in MM.REF_OPS:
            r += n
        if op in MM.QRY_OPS:
            q += n
    return out


def shifts_of(alignment, ref_seqs, min_sv_size):
    """[(op index, shift)] of the gaps shorter than min_sv_size of a record the command uses ([] for the others)."""
    contig, start, ops, seq = alignment
    if not seq or any(op == 3 for op, _ in ops):
        return []
    window = ref_seqs[contig][start:start + sum(n for op, n in ops if op in MM.REF_OPS)].encode("latin-1")
    qry = seq.encode("latin-1")
    return [(j, shift_of(window, qry, r, q, n, kind, limit)) for j, r, q, n, kind, limit in gaps_of(start, ops) if n < min_sv_size]


def rewrite(alignments, ref_seqs, min_sv_size=40):
    """The same alignments with every small gap moved by its shift in the CIGAR: the aligned run in front shortened, the
    run behind lengthened, SEQ untouched; limits and shifts from the ORIGINAL ops.  Returns (alignments, shifts > 0)."""
    out, moved = [], []
    for alignment in alignments:
        contig, start, ops, seq = alignment
        ops = [list(x) for x in ops]
        for j, k in shifts_of(alignment, ref_seqs, min_sv_size):
            if k == 0:
                continue
            moved.append(k)
            left, i = k, j - 1
            while left:  # (the limit keeps all k columns, and one more, inside aligned ops in front of the gap)
                assert i >= 0 and ops[i][0] in (0, 7, 8)
                take = min(left, ops[i][1])
                ops[i][1] -= take
                left -= take
                i -= 1
            if j + 1 < len(ops) and ops[j + 1][0] in (0, 7):
                ops[j + 1][1] += k
            else:
                ops[j] = [ops[j], [0, k]]  # (a passed column is a match: an M run of its own)
        flat = []
        for x in ops:
            flat += [tuple(y) for y in x] if isinstance(x[0], list) else [tuple(x)]
        out.append((contig, start, [(op, n) for op, n in flat if n > 0], seq))
    return out, moved
