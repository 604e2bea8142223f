"""Read a VCF back (include/svx_vcfin.h, csrc/svx_vcfin.cpp): the deletions and insertions of one sample as a
CandidateTable, everything else counted by class.  The inverse of the VCF writer for DEL and INS, sequence-resolved or
symbolic <DEL>; what the classes are is defined in include/svx_vcfin.h."""
import ctypes as C

import numpy as np

from svim_asm_amd import _lib
from svim_asm_amd.table import CandidateTable, T_DEL, T_INS

CLASSES = ("DEL", "INS", "multiallelic", "complex", "unresolved", "other", "not_carried", "filtered")
# genotype column of the table: the index IS the haplotype bits (bit h: allele h is 1); 0: no genotype in the file
GENOTYPES = ("./.", "1/0", "0/1", "1/1")


class VcfFormatError(ValueError):
    """The file is refused: the message names the file and the 1-based line."""


class VcfRecords(object):
    """What read_vcf returns.
      table      CandidateTable of the DEL and INS rows in file order (contigs: the genome's; gt: haplotype bits)
      line_no    1-based line of every row;  ids: its ID column;  lines: its line, verbatim, without the line end
      header     the header lines, verbatim with their line ends
      counts     {class: data lines}, DEL and INS among them;  n_lines: all data lines"""

    def __init__(self, table, line_no, ids, lines, header, counts, n_lines):
        self.table, self.line_no, self.ids, self.lines = table, line_no, ids, lines
        self.header, self.counts, self.n_lines = header, counts, n_lines

    def __len__(self):
        return len(self.table)


def _column(ptr, n, dtype):
    if not n:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dtype).itemsize,)).view(dtype).copy()


def read_vcf(path, contigs, contig_len, sample=None, passonly=False, threads=0):
    """Read `path` (plain text or BGZF) against the contig dictionary of the genome's .fai.  sample: the sample column
    by name (None: the first).  Raises VcfFormatError with the reader's message."""
    return _read(path, contigs, contig_len, sample, passonly, threads, False)


def read_sites(path, contigs, contig_len, passonly=False, threads=0):
    """read_vcf for a list of SITES (svx_vcfin_open_sites): the sample columns are not looked at — no record is
    not_carried, the table's gt is 0 throughout."""
    return _read(path, contigs, contig_len, None, passonly, threads, True)


ALLELE_CLASSES = ("rows", "multiallelic", "symbolic_or_other", "not_carried", "filtered", "no_change")


class VcfAlleles(object):
    """What read_alleles returns: the sequence-resolved records of one sample as edits, in file order (columns as numpy
    arrays; svx_vcfin_alleles in include/svx_vcfin.h).
      contig, start, ref_len        the reference bytes [start, start + ref_len) of contigs[contig] ...
      alt_off, alt_len, alts        ... become alts[alt_off : alt_off + alt_len] (uint8, upper case)
      pos, ref_off, ref_text_len    POS - 1 and the REF column as written, text[ref_off : ref_off + ref_text_len]
      gt, phased                    haplotype bits (0: unknown) and whether the record's haplotypes are told apart
      line_off, line_len, line_no, id_off, id_len, text, header, counts, n_lines    as for read_vcf"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return len(self.start)

    def line(self, i):
        return self.text[int(self.line_off[i]):int(self.line_off[i]) + int(self.line_len[i])]


def read_alleles(path, contigs, contig_len, sample=None, passonly=False, threads=0):
    """Read `path` as a list of edits (svx_vcfin_open_alleles).  Raises VcfFormatError with the reader's message."""
    lib = _lib.load()
    names = [c.encode() for c in contigs]
    name_arr = (C.c_char_p * len(names))(*names)
    lengths = np.ascontiguousarray(contig_len, dtype=np.int64)
    h, err = C.c_void_p(), C.create_string_buffer(1024)
    rc = lib.svx_vcfin_open_alleles(str(path).encode(), len(names), C.cast(name_arr, C.c_void_p), lengths.ctypes.data,
                                    None if sample is None else str(sample).encode(), 1 if passonly else 0, int(threads), C.byref(h),
                                    err, len(err))
    if rc != _lib.SVX_OK:
        raise VcfFormatError(err.value.decode("utf-8", "replace") or "svx_vcfin_open_alleles failed (%d)" % rc)
    try:
        c = _lib.VcfinAlleles()
        rc = lib.svx_vcfin_get_alleles(h, C.byref(c))
        if rc != _lib.SVX_OK:
            raise VcfFormatError("svx_vcfin_get_alleles failed (%d)" % rc)
        n = int(c.n)
        text = C.string_at(c.text, int(c.text_bytes)) if c.text_bytes else b""
        return VcfAlleles(
            contig=_column(c.contig, n, np.int32), start=_column(c.start, n, np.int64), ref_len=_column(c.ref_len, n, np.uint32),
            alt_off=_column(c.alt_off, n, np.uint64), alt_len=_column(c.alt_len, n, np.uint32),
            alts=_column(c.alts, int(c.alt_bytes), np.uint8), pos=_column(c.pos, n, np.int64), ref_off=_column(c.ref_off, n, np.uint64),
            ref_text_len=_column(c.ref_text_len, n, np.uint32), gt=_column(c.gt, n, np.uint8), phased=_column(c.phased, n, np.uint8),
            line_off=_column(c.line_off, n, np.uint64), line_len=_column(c.line_len, n, np.uint32),
            line_no=_column(c.line_no, n, np.uint32), id_off=_column(c.id_off, n, np.uint64), id_len=_column(c.id_len, n, np.uint32),
            text=text, header=text[:int(c.header_bytes)], counts={name: int(c.counts[k]) for k, name in enumerate(ALLELE_CLASSES)},
            n_lines=int(c.n_lines))
    finally:
        lib.svx_vcfin_close(h)


def _read(path, contigs, contig_len, sample, passonly, threads, sites):
    lib = _lib.load()
    names = [c.encode() for c in contigs]
    name_arr = (C.c_char_p * len(names))(*names)
    lengths = np.ascontiguousarray(contig_len, dtype=np.int64)
    h, err = C.c_void_p(), C.create_string_buffer(1024)
    if sites:
        rc = lib.svx_vcfin_open_sites(str(path).encode(), len(names), C.cast(name_arr, C.c_void_p), lengths.ctypes.data,
                                      1 if passonly else 0, int(threads), C.byref(h), err, len(err))
    else:
        rc = lib.svx_vcfin_open(str(path).encode(), len(names), C.cast(name_arr, C.c_void_p), lengths.ctypes.data,
                                None if sample is None else str(sample).encode(), 1 if passonly else 0, int(threads), C.byref(h),
                                err, len(err))
    if rc != _lib.SVX_OK:
        raise VcfFormatError(err.value.decode("utf-8", "replace") or "svx_vcfin_open failed (%d)" % rc)
    try:
        c = _lib.VcfinColumns()
        rc = lib.svx_vcfin_get_columns(h, C.byref(c))
        if rc != _lib.SVX_OK:
            raise VcfFormatError("svx_vcfin_get_columns failed (%d)" % rc)
        n = int(c.n)
        text = C.string_at(c.text, int(c.text_bytes)) if c.text_bytes else b""
        kind = _column(c.type, n, np.uint8)
        contig = _column(c.contig, n, np.int32)
        start, end = _column(c.start, n, np.int64), _column(c.end, n, np.int64)
        is_ins = kind == 1
        t = CandidateTable(contigs, contig_len, n, seqs=_column(c.seqs, int(c.seq_bytes), np.uint8), genotypes=GENOTYPES)
        t.type[:] = np.where(is_ins, T_INS, T_DEL)
        t.sc[:] = np.where(is_ins, -1, contig)
        t.ss[:] = np.where(is_ins, 0, start)
        t.se[:] = np.where(is_ins, 0, end)
        t.dc[:] = np.where(is_ins, contig, -1)
        t.ds[:] = np.where(is_ins, start, 0)
        t.de[:] = np.where(is_ins, end, 0)
        t.gt[:] = _column(c.gt, n, np.uint8)
        t.q_off[:] = _column(c.seq_off, n, np.uint64).astype(np.int64)
        t.q_len[:] = _column(c.seq_len, n, np.uint32)
        line_off, line_len = _column(c.line_off, n, np.uint64).tolist(), _column(c.line_len, n, np.uint32).tolist()
        id_off, id_len = _column(c.id_off, n, np.uint64).tolist(), _column(c.id_len, n, np.uint32).tolist()
        lines = [text[o:o + l] for o, l in zip(line_off, line_len)]
        ids = [text[o:o + l].decode("utf-8", "surrogateescape") for o, l in zip(id_off, id_len)]
        counts = {name: int(c.counts[k]) for k, name in enumerate(CLASSES)}
        return VcfRecords(t, _column(c.line_no, n, np.uint32), ids, lines, text[:int(c.header_bytes)], counts, int(c.n_lines))
    finally:
        lib.svx_vcfin_close(h)
