"""FASTQ / FASTA in (the north star's "FASTQ-in" surface — the reference itself simulates its reads in
R, lib/GenerateReads.R, and has no file reader on this path).  The reader is libgasm's (csrc/seqio.cpp, C++ with zlib):
it parses and packs 2-bit in one go; this module is its ctypes face."""
import ctypes as C

import numpy as np

from ._lib import INGEST_STATS, QUAL_BINS, IngestParams, check, lib


def _paths(paths):
    arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
    return arr


class IngestStats:
    """What an ingest under options did, per file (= segment): `counters` is the (n_files, len(INGEST_STATS)) uint64 array of
    include/gasm.h's counters, each also an attribute of its name (records, kept, dropped_non_acgt, dropped_short, dropped_mate,
    bases_in, bases_kept, bases_dropped, trimmed5, trimmed3, reads_trimmed: one uint64 per file); `quality_hist` is the
    (n_files, QUAL_BINS) histogram of the base qualities before trimming (zeros unless quality_hist=True, and for FASTA)."""

    def __init__(self, counters, quality_hist):
        self.counters = np.asarray(counters, dtype=np.uint64).reshape(-1, len(INGEST_STATS))
        self.quality_hist = np.asarray(quality_hist, dtype=np.uint64).reshape(-1, QUAL_BINS)
        for i, name in enumerate(INGEST_STATS):
            setattr(self, name, self.counters[:, i])

    def mean_quality(self, file=0):
        """mean base quality of the file (0.0 where the histogram is empty)"""
        h = self.quality_hist[file].astype(np.float64)
        return float((h * np.arange(QUAL_BINS)).sum() / h.sum()) if h.sum() else 0.0

    def suggest_trim_q(self, file=0):
        """a cutoff for trim_q3 / trim_q5 from the file's own histogram, the way kmer_spectrum() serves min_count: the largest q such
        that at most 5 % of the bases have a quality below q, clamped to 2..30.  The 5 % is a convention, not a derivation."""
        h = [int(x) for x in self.quality_hist[file]]
        total, below, best = sum(h), 0, 0
        for q in range(QUAL_BINS + 1):
            if 20 * below <= total:
                best = q
            if q < QUAL_BINS:
                below += h[q]
        return max(2, min(30, best))

    def __eq__(self, other):
        return isinstance(other, IngestStats) and np.array_equal(self.counters, other.counters) and np.array_equal(self.quality_hist, other.quality_hist)

    def __repr__(self):
        return "IngestStats(" + ", ".join(f"{n}={self.counters[:, i].tolist()}" for i, n in enumerate(INGEST_STATS)) + ")"


def _packed_out(h, n_files, with_device, with_stats):
    """the arrays of a gasm_packed handle (freed here)"""
    L = lib()
    try:
        n, S = L.gasm_packed_n_reads(h), L.gasm_packed_n_segments(h)
        off = np.ctypeslib.as_array(C.cast(L.gasm_packed_read_off(h), C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        seg = np.ctypeslib.as_array(C.cast(L.gasm_packed_seg_read_off(h), C.POINTER(C.c_uint64)), shape=(S + 1,)).copy()
        nw = (int(off[-1]) + 31) // 32
        words = np.ctypeslib.as_array(C.cast(L.gasm_packed_words(h), C.POINTER(C.c_uint64)), shape=(nw,)).copy() if nw else np.zeros(0, np.uint64)
        out = [words, off, seg, int(L.gasm_packed_dropped(h))]
        if with_device:
            out.append([bool(L.gasm_packed_parsed_on_device(h, f)) for f in range(n_files)])
        if with_stats:
            st = np.ctypeslib.as_array(C.cast(L.gasm_packed_ingest_stats(h), C.POINTER(C.c_uint64)), shape=(S * len(INGEST_STATS),)).copy()
            qh = np.ctypeslib.as_array(C.cast(L.gasm_packed_quality_hist(h), C.POINTER(C.c_uint64)), shape=(S * QUAL_BINS,)).copy()
            out.append(IngestStats(st, qh))
        return tuple(out)
    finally:
        L.gasm_packed_free(h)


def read_files(paths, non_acgt="drop", **trim):
    """one file per segment -> (words uint64 (2-bit, 32 bases per word, first base most significant, reads back to back),
    read_off uint64[n+1] (base offsets), seg_read_off uint64[S+1], dropped reads).
    trim: the ingest options of include/gasm.h ("Quality trimming at ingest"): trim_q3, trim_q5, min_len, pairs, phred_offset,
    quality_hist.  With any of them set (a phred_offset alone sets nothing) an IngestStats follows as a fifth element."""
    p = IngestParams.make(non_acgt, **trim)
    h = C.c_void_p()
    check(lib().gasm_read_files_params(_paths(paths), len(paths), C.byref(p), C.byref(h)))
    return _packed_out(h, len(paths), False, p.any())


def read_files_device(paths, non_acgt="drop", ctx=None, **trim):
    """the same through the device path (gasm_read_files_device, csrc/ingest.hip: the host inflates, the GPU finds the records
    and packs them) -> (words, read_off, seg_read_off, dropped, parsed_on_device[bool per file]); under options (see read_files) the
    GPU also trims, one wave per record, and an IngestStats follows as a sixth element"""
    from ._lib import default_context
    ctx = ctx or default_context()
    p = IngestParams.make(non_acgt, **trim)
    h = C.c_void_p()
    check(lib().gasm_read_files_device_params(ctx.h, _paths(paths), len(paths), C.byref(p), C.byref(h)))
    return _packed_out(h, len(paths), True, p.any())


def unpack_reads(words, read_off):
    """packed reads -> list of bytes (for inspection and tests)"""
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    n = int(read_off[-1])
    w = np.asarray(words, dtype=np.uint64)
    idx = np.arange(n)
    bases = lut[((w[idx >> 5] >> (62 - 2 * (idx & 31)).astype(np.uint64)) & np.uint64(3)).astype(np.int64)] if n else np.zeros(0, np.uint8)
    return [bases[int(read_off[i]):int(read_off[i + 1])].tobytes() for i in range(len(read_off) - 1)]
