"""SegmentBatch: reads of many independent segments in, contigs + breakage scores out, everything resident in HBM
between the calls (gasm_batch_* in include/gasm.h).  This is the reads-level surface the reference only has in R
(lib/DeNovoAssembler.R:58-68: get_reads -> get_kmers_from_reads -> get_contigs -> calc_breakscore)."""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import qtable, readkmers
from ._lib import CORRECT_FIELDS, INGEST_STATS, QUAL_BINS, IngestParams, MAP_FIELDS, MAP_MAX_GAP, MAP_MAX_MISMATCH, MAP_MAX_PIECES, MAPEND_FIELDS, MAPG_FIELDS, MAPSCORE_FIELDS, MAPSCORE_PARTIAL, MAPSCORE_SOURCES, MAX_TABLES, MAX_BUBBLE_ROUNDS, MAX_COV_ROUNDS, MAX_INSERT, MAX_SPAN_LEN, MAX_TIP_ROUNDS, PAIR_FIELDS, PLAN_FIELDS, BuildParams, check, default_context, lib
from .api import _check_build_opts, unpack_kmers
from .links import ContigLinks
from .pairs import PairPlaces
from .readmap import AlignedReadMap, GappedReadMap, MappedScores, ReadMap


def _arr(p, ctype, n):
    """a copy of the n entries of `ctype` a fetch handed out at pointer p"""
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(n,)).copy() if n else np.zeros(0, ctype)


def weighted_median_half(mult_sum, n_edges):
    """floor(median / 2) of the contigs' mean multiplicities mult_sum / n_edges, each weighted by n_edges: the median is the mean of
    the first contig, in ascending order of mean, at which the running weight reaches half the total.  Exact integers."""
    ms, ns = [int(x) for x in mult_sum], [int(x) for x in n_edges]
    order = sorted(range(len(ns)), key=lambda i: Fraction(ms[i], ns[i]))
    total, run = sum(ns), 0
    for i in order:
        run += ns[i]
        if 2 * run >= total:
            return ms[i] // (2 * ns[i])
    return 0


class SegmentBatch:
    def __init__(self, reads, seg_read_off, fixed_len=0, read_off=None, ctx=None):
        """reads: uint8 array (ASCII ACGT) of all reads of all segments, concatenated segment after segment.
        seg_read_off: n_segments+1 read indices.  Either fixed_len > 0 or read_off (n_reads+1 base offsets)."""
        self.ctx = ctx or default_context()
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        seg = np.ascontiguousarray(seg_read_off, dtype=np.uint64)
        self.n_segments = len(seg) - 1
        self.n_reads = int(seg[-1])
        ro = None
        if read_off is not None:
            ro = np.ascontiguousarray(read_off, dtype=np.uint64)
            fixed_len = 0
        h = C.c_void_p()
        check(lib().gasm_batch_create(self.ctx.h, reads.ctypes.data_as(C.c_void_p),
                                      ro.ctypes.data_as(C.c_void_p) if ro is not None else None, self.n_reads, int(fixed_len),
                                      seg.ctypes.data_as(C.c_void_p), self.n_segments, C.byref(h)))
        self.h = h
        self.k = None
        self._table = None
        self._seg_read_off = seg.copy()
        self._read_len = np.diff(ro.astype(np.int64)) if ro is not None else np.full(self.n_reads, int(fixed_len), np.int64)

    @classmethod
    def from_strings(cls, segments, ctx=None):
        """segments: list (one per segment) of lists of read strings"""
        seg = np.zeros(len(segments) + 1, dtype=np.uint64)
        off, data = [0], []
        for i, rs in enumerate(segments):
            seg[i + 1] = seg[i] + len(rs)
            for r in rs:
                b = r.encode() if isinstance(r, str) else bytes(r)
                data.append(b)
                off.append(off[-1] + len(b))
        buf = np.frombuffer(b"".join(data), dtype=np.uint8) if data else np.zeros(0, dtype=np.uint8)
        return cls(buf, seg, read_off=np.array(off, dtype=np.uint64), ctx=ctx)

    @classmethod
    def from_packed(cls, words, seg_read_off, fixed_len=0, read_off=None, ctx=None):
        """reads that are 2-bit packed already (gasm_batch_create_packed): a quarter of the bytes over PCIe"""
        self = cls.__new__(cls)
        self.ctx = ctx or default_context()
        w = np.ascontiguousarray(words, dtype=np.uint64)
        seg = np.ascontiguousarray(seg_read_off, dtype=np.uint64)
        ro = np.ascontiguousarray(read_off, dtype=np.uint64) if read_off is not None else None
        self.n_segments, self.n_reads = len(seg) - 1, int(seg[-1])
        h = C.c_void_p()
        check(lib().gasm_batch_create_packed(self.ctx.h, w.ctypes.data_as(C.c_void_p), ro.ctypes.data_as(C.c_void_p) if ro is not None else None,
                                             self.n_reads, 0 if ro is not None else int(fixed_len), seg.ctypes.data_as(C.c_void_p),
                                             self.n_segments, C.byref(h)))
        self.h, self.k, self._table = h, None, None
        self._seg_read_off = seg.copy()
        self._read_len = np.diff(ro.astype(np.int64)) if ro is not None else np.full(self.n_reads, int(fixed_len), np.int64)
        return self

    @classmethod
    def simulate(cls, genomes, read_len, coverage, seed, kmer=8, table=None, ctx=None):
        """reads simulated on the device from the segments' genomes (lib/GenerateReads.R:235-313, gasm_batch_simulate):
        genomes = list of str/bytes/uint8 arrays; table = normalised 69 904-row table for probability-weighted starts
        (the reference's ultrasonication model) or None for uniform starts"""
        self = cls.__new__(cls)
        self.ctx = ctx or default_context()
        bs = [g.encode() if isinstance(g, str) else (g.tobytes() if hasattr(g, "tobytes") else bytes(g)) for g in genomes]
        off = np.zeros(len(bs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        t = np.ascontiguousarray(table, dtype=np.float64) if table is not None else None
        h = C.c_void_p()
        check(lib().gasm_batch_simulate(self.ctx.h, b"".join(bs), off.ctypes.data_as(C.c_void_p), len(bs), int(read_len), float(coverage), int(seed),
                                        int(kmer), t.ctypes.data_as(C.c_void_p) if t is not None else None, C.byref(h)))
        self.h, self.k, self._table = h, None, None
        self.n_segments = len(bs)
        self.n_reads = int(lib().gasm_batch_total_reads(h))
        return self

    def read_starts(self):
        """(seg_read_off[n_segments+1], 0-based start of every simulated read in its genome)"""
        so, st = C.c_void_p(), C.c_void_p()
        check(lib().gasm_batch_fetch_read_starts(self.h, C.byref(so), C.byref(st)))
        seg = np.ctypeslib.as_array(C.cast(so, C.POINTER(C.c_uint64)), shape=(self.n_segments + 1,)).copy()
        n = int(seg[-1])
        starts = np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_uint32)), shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        return seg, starts

    @classmethod
    def from_fastq(cls, paths, non_acgt="drop", ctx=None, trim_q3=0, trim_q5=0, min_len=0, pairs=False, phred_offset=33, quality_hist=False):
        """one FASTQ/FASTA file (plain or .gz) per segment, read and packed by libgasm (gasm_batch_from_files_params); reads with a
        base outside ACGT are dropped (count in `.dropped_reads`) or, with non_acgt='error', refused.
        trim_q3 / trim_q5 > 0: FASTQ records are trimmed by base quality at that end (the running-sum rule of include/gasm.h,
        "Quality trimming at ingest"; an N counts as quality 0, so a terminal N goes and the read stays); min_len: shorter spans are
        dropped; pairs: an interleaved file's mates (records 2p, 2p + 1) are kept or dropped together, so place_pairs() still finds
        them; quality_hist: ingest_stats() also holds the histogram suggest_trim_q() reads.  `.dropped_reads` counts every drop."""
        from .seqio import _paths
        self = cls.__new__(cls)
        self.ctx = ctx or default_context()
        p = IngestParams.make(non_acgt, trim_q3=trim_q3, trim_q5=trim_q5, min_len=min_len, pairs=bool(pairs), phred_offset=phred_offset, quality_hist=bool(quality_hist))
        h, dropped = C.c_void_p(), C.c_uint64()
        check(lib().gasm_batch_from_files_params(self.ctx.h, _paths(paths), len(paths), C.byref(p), C.byref(h), C.byref(dropped)))
        self.h, self.k, self._table = h, None, None
        self.n_segments = len(paths)
        self.n_reads = int(lib().gasm_batch_total_reads(h))
        self.dropped_reads = int(dropped.value)
        self.ingest_options = p.any()          # an option besides non_acgt was set: ingest_stats() has something to say
        return self

    def ingest_stats(self):
        """seqio.IngestStats of a batch made by from_fastq() under an option besides non_acgt (else GASM_ERR_STATE)"""
        from .seqio import IngestStats
        a, b = C.c_void_p(), C.c_void_p()
        check(lib().gasm_batch_fetch_ingest_stats(self.h, C.byref(a), C.byref(b)))
        return IngestStats(_arr(a, C.c_uint64, self.n_segments * len(INGEST_STATS)), _arr(b, C.c_uint64, self.n_segments * QUAL_BINS))

    def _build(self, k, genome_len_hint, **opts):
        """every build*() below: check the options, hand them to the library as one gasm_build_params (gasm_batch_build_params).  The
        rounds of a feature that is off are not read, here or there."""
        _check_build_opts(**opts)
        check(lib().gasm_batch_build_params(self.h, C.byref(BuildParams.make(k, genome_len_hint=genome_len_hint, **opts))))
        self.k, self._min_count = int(k), int(opts.get("min_count", 1))
        return self

    def build(self, k, genome_len_hint=0, min_count=1, strands=1):
        """queue a build.  min_count > 1: only the k-mers seen at least min_count times in their segment become edges — the cutoff
        for reads with sequencing errors; everything after the build sees the survivors only.  genome_len_hint then counts the
        distinct k-mers before the cutoff (include/gasm.h).
        strands = 2: the k-mers of every read and of its reverse complement — reads of both strands then meet in one graph,
        multiplicities (and min_count) are sums over both strands, and the contigs come in reverse-complement pairs
        (contig_twins).  Scores are over the reads as they were given, each once.
        Tip clipping: build_tips().  Bubble popping: build_bubbles().  Low-coverage removal: build_simplified()."""
        return self._build(k, genome_len_hint, min_count=min_count, strands=strands)

    def build_tips(self, k, genome_len_hint=0, min_count=1, strands=1, tip_len=0, tip_rounds=1):
        """build() with tip clipping: exactly tip_rounds rounds (1.._lib.MAX_TIP_ROUNDS) behind the cutoff — a contig of at most
        tip_len bases that dead-ends on one side and hangs, on the other, on a node with a strictly stronger sibling edge leaves
        the k-mer set with all its k-mers (the rule: include/gasm.h); 2k - 1 is the intended length.  tip_stats() tells what each
        round removed.  tip_len = 0 is build(k, genome_len_hint, min_count, strands): the same build, and tip_rounds is not read."""
        return self._build(k, genome_len_hint, min_count=min_count, strands=strands, tip_len=tip_len, tip_rounds=tip_rounds)

    def build_bubbles(self, k, genome_len_hint=0, min_count=1, strands=1, tip_len=0, tip_rounds=1, bubble_len=0, bubble_rounds=1):
        """build_tips() with bubble popping: exactly bubble_rounds rounds (1.._lib.MAX_BUBBLE_ROUNDS) behind the tip rounds — a contig
        of at most bubble_len bases (<= _lib.MAX_BUBBLE_LEN) beside which a parallel one (same first and last node, at most
        bubble_len bases too) of strictly higher mean multiplicity runs leaves the k-mer set with all its k-mers (the rule:
        include/gasm.h); 2k - 1 is the intended length.  bubble_stats() tells what each round removed.  bubble_len = 0 is
        build_tips(k, genome_len_hint, min_count, strands, tip_len, tip_rounds), and bubble_rounds is not read."""
        return self._build(k, genome_len_hint, min_count=min_count, strands=strands, tip_len=tip_len, tip_rounds=tip_rounds, bubble_len=bubble_len,
                           bubble_rounds=bubble_rounds)

    def build_simplified(self, k, genome_len_hint=0, *, min_count=1, strands=1, tip_len=0, tip_rounds=1, bubble_len=0, bubble_rounds=1, cov_cutoff=0,
                         cov_len=0, cov_rounds=1):
        """build_bubbles() with low-coverage removal: exactly cov_rounds rounds (1.._lib.MAX_COV_ROUNDS) behind the tip and the bubble
        rounds — a contig of at most cov_len bases (<= _lib.MAX_BUBBLE_LEN) whose mean multiplicity is strictly below cov_cutoff leaves
        the k-mer set with all its k-mers, whatever is attached to it (the rule: include/gasm.h).  The intended setting is
        cov_len = 2k - 1, cov_cutoff = min_count + 1, one round; suggest_cov_cutoff() derives a cutoff from a build's own contigs.
        lowcov_stats() tells what each round removed.  cov_cutoff = 0 or cov_len = 0 is build_bubbles() with the other arguments, and
        cov_rounds is not read.  The knobs are keyword-only: the positional chain ends with build_bubbles()."""
        return self._build(k, genome_len_hint, min_count=min_count, strands=strands, tip_len=tip_len, tip_rounds=tip_rounds, bubble_len=bubble_len,
                           bubble_rounds=bubble_rounds, cov_cutoff=cov_cutoff, cov_len=cov_len, cov_rounds=cov_rounds)

    def solid_stats(self):
        """(distinct k-mers per segment before the last build's cutoff, after it): two uint64 arrays, equal at min_count = 1"""
        a, b = C.c_void_p(), C.c_void_p()
        check(lib().gasm_batch_fetch_solid_stats(self.h, C.byref(a), C.byref(b)))
        n = self.n_segments
        return (np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_uint64)), shape=(n,)).copy(),
                np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_uint64)), shape=(n,)).copy())

    def _round_stats(self, fetch, max_rounds):
        """the two (n_segments, max_rounds) uint32 arrays of one gasm_batch_fetch_*_stats entry"""
        a, b = C.c_void_p(), C.c_void_p()
        check(fetch(self.h, C.byref(a), C.byref(b)))
        n = self.n_segments * max_rounds
        shape = (self.n_segments, max_rounds)
        if not n:
            return np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
        return (np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_uint32)), shape=(n,)).copy().reshape(shape),
                np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_uint32)), shape=(n,)).copy().reshape(shape))

    def tip_stats(self):
        """(contigs clipped, k-mers clipped) by the last build's tip clipping: two (n_segments, MAX_TIP_ROUNDS) uint32 arrays,
        column r = round r, zero for rounds not run.  A non-zero last round run: more rounds would clip more."""
        return self._round_stats(lib().gasm_batch_fetch_tip_stats, MAX_TIP_ROUNDS)

    def bubble_stats(self):
        """(contigs popped, k-mers popped) by the last build's bubble popping: two (n_segments, MAX_BUBBLE_ROUNDS) uint32 arrays,
        column r = round r, zero for rounds not run.  A non-zero last round run: more rounds would pop more."""
        return self._round_stats(lib().gasm_batch_fetch_bubble_stats, MAX_BUBBLE_ROUNDS)

    def lowcov_stats(self):
        """(contigs removed, k-mers removed) by the last build's low-coverage removal: two (n_segments, MAX_COV_ROUNDS) uint32 arrays,
        column r = round r, zero for rounds not run.  A non-zero last round run: more rounds would remove more."""
        return self._round_stats(lib().gasm_batch_fetch_lowcov_stats, MAX_COV_ROUNDS)

    def contig_coverage(self, segment=None):
        """(mult_sum uint64, n_edges uint32) of the last build's contigs (gasm_batch_contig_coverage), one entry per contig in the
        order of contigs(): the sum of the contig's k-mer multiplicities and the number of its k-mers; mult_sum / n_edges is its
        mean multiplicity.  segment = None: the whole batch, segment after segment; else that segment's contigs only."""
        check(lib().gasm_batch_contig_coverage(self.h))
        m, n = C.c_void_p(), C.c_void_p()
        check(lib().gasm_batch_fetch_contig_coverage(self.h, C.byref(m), C.byref(n)))
        so, _, _ = self.contigs_raw()
        total = int(so[-1])
        if not total:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        ms = np.ctypeslib.as_array(C.cast(m, C.POINTER(C.c_uint64)), shape=(total,)).copy()
        ns = np.ctypeslib.as_array(C.cast(n, C.POINTER(C.c_uint32)), shape=(total,)).copy()
        if segment is None:
            return ms, ns
        a, z = int(so[int(segment)]), int(so[int(segment) + 1])
        return ms[a:z], ns[a:z]

    def contig_links(self, span_len=None):
        """the links between the last build's contigs and the reads' support for them (gasm_batch_contig_links; the rule: include/gasm.h
        "Contig links") as a links.ContigLinks: per segment succ / pred (which contig follows / precedes which over which base), link
        support (crossings of every link in the reads), span support (reads that run through a contig of at most span_len bases from an
        in-edge to an out-edge) and the reads too long to thread.  span_len = None: the longest read of the batch (a longer contig cannot
        be spanned), at most _lib.MAX_SPAN_LEN; 0: no span work.  After a strands = 2 build every read and its reverse complement are
        threaded.  Reads the build only: contigs, scores, coverage and twins are what they were."""
        if span_len is None:
            span_len = min(self._longest_read(), MAX_SPAN_LEN)
        if not 0 <= int(span_len) <= MAX_SPAN_LEN:
            raise ValueError(f"span_len must be 0..{MAX_SPAN_LEN} (0: no span support)")
        seg, _, contigs = self._contigs_by_segment()
        total = int(seg[-1])
        check(lib().gasm_batch_contig_links(self.h, int(span_len)))
        ps = [C.c_void_p() for _ in range(5)]
        check(lib().gasm_batch_fetch_contig_links(self.h, *[C.byref(p) for p in ps]))
        succ, pred, lsup = (_arr(p, C.c_uint32, 4 * total) for p in ps[:3])
        ssup, skipped = _arr(ps[3], C.c_uint32, 16 * total), _arr(ps[4], C.c_uint64, self.n_segments)
        ms, _ = self.contig_coverage()
        return ContigLinks(self.k, int(span_len), self.strands(), seg, contigs, succ, pred, lsup, ssup, skipped, ms)

    def _longest_read(self):
        if getattr(self, "_max_read_len", None) is None:
            off = self.reads()[1]
            self._max_read_len = int(np.diff(off).max()) if len(off) > 1 else 0
        return self._max_read_len

    def _read_lengths(self):
        """the reads' lengths, int64: from the offsets the batch was made with; a batch made on the device or from files (simulate,
        from_fastq, correct_reads) asks the library once (gasm_batch_fetch_reads hands out the offsets beside the bases: only the
        offsets are copied here)"""
        if getattr(self, "_read_len", None) is None:
            d, o = C.c_void_p(), C.c_void_p()
            check(lib().gasm_batch_fetch_reads(self.h, C.byref(d), C.byref(o)))
            self._read_len = np.diff(_arr(o, C.c_uint64, self.n_reads + 1).astype(np.int64))
        return self._read_len

    def place_pairs(self, max_insert=None):
        """where the batch's read pairs lie on the last build's contigs (gasm_batch_place_pairs; the rule: include/gasm.h "Read pairs") as
        a pairs.PairPlaces: per segment the records (c1, S, c2, E) of every oriented pair, the insert histogram and the six counters.
        Reads 2p and 2p + 1 of a segment are the mates of pair p, forward-reverse.  max_insert: the histogram's overflow bin, 1 ..
        _lib.MAX_INSERT; None: max(1024, 4 x the longest read), at most _lib.MAX_INSERT.  After a strands = 2 build both orientations of
        every pair are placed.  Reads the build only: contigs, scores, coverage, twins and links are what they were."""
        if max_insert is None:
            max_insert = min(max(1024, 4 * self._longest_read()), MAX_INSERT)
        if not 1 <= int(max_insert) <= MAX_INSERT:
            raise ValueError(f"max_insert must be 1..{MAX_INSERT}")
        max_insert = int(max_insert)
        check(lib().gasm_batch_place_pairs(self.h, max_insert))
        ps, orient = [C.c_void_p() for _ in range(3)], C.c_uint32()
        check(lib().gasm_batch_fetch_pair_places(self.h, *[C.byref(p) for p in ps], C.byref(orient)))
        o, n_pairs = int(orient.value), self.n_reads // 2
        rec = _arr(ps[0], C.c_int32, 4 * o * n_pairs)
        hist, cnt = _arr(ps[1], C.c_uint32, self.n_segments * (max_insert + 1)), _arr(ps[2], C.c_uint64, self.n_segments * len(PAIR_FIELDS))
        return PairPlaces(self.k, self.strands(), max_insert, o, self.contigs(), rec, hist, cnt)

    def map_reads(self, max_mismatch=4):
        """where the batch's reads lie on the last build's contigs within max_mismatch substitutions (gasm_batch_map_reads; the rule:
        include/gasm.h "Read mapping") as a readmap.ReadMap: per read its best place, per contig base the four base counts of the reads
        laid over it, per segment the mismatch histogram and the seven counters.  max_mismatch: 0 .. _lib.MAP_MAX_MISMATCH.  The reads
        are mapped as given, whatever the build's strands.  Reads the build only: contigs, scores, coverage, twins, links and pair
        places are what they were."""
        if not 0 <= int(max_mismatch) <= MAP_MAX_MISMATCH:
            raise ValueError(f"max_mismatch must be 0..{MAP_MAX_MISMATCH}")
        max_mismatch = int(max_mismatch)
        check(lib().gasm_batch_map_reads(self.h, max_mismatch))
        ps = [C.c_void_p() for _ in range(4)]
        check(lib().gasm_batch_fetch_read_map(self.h, *[C.byref(p) for p in ps]))
        seg, o, contigs = self._contigs_by_segment()
        total = int(o[-1]) if int(seg[-1]) else 0
        rec, pile = _arr(ps[0], C.c_int32, 4 * self.n_reads), _arr(ps[1], C.c_uint32, 4 * total)
        hist, cnt = _arr(ps[2], C.c_uint32, self.n_segments * (max_mismatch + 1)), _arr(ps[3], C.c_uint64, self.n_segments * len(MAP_FIELDS))
        strands = self.strands()
        return ReadMap(self.k, strands, max_mismatch, contigs, rec, pile, hist, cnt,
                       [t.tolist() for t in self.contig_twins()] if strands == 2 else None, getattr(self, "_seg_read_off", None))

    def map_reads_gapped(self, max_edits=6, max_gap=3, end_gap=0):
        """map_reads() for reads that carry insertions and deletions as well (gasm_batch_map_reads_gapped; the rule: include/gasm.h "Gapped
        read mapping") as a readmap.GappedReadMap: heads of a read on neighbouring diagonals of one contig, at most max_gap apart, are
        joined into a chain and verified as one alignment of a cost (mismatches + gap lengths) of at most max_edits.  max_edits: 0 ..
        _lib.MAP_MAX_MISMATCH, max_gap: 0 .. _lib.MAP_MAX_GAP (0: the tables of map_reads(max_edits)).  end_gap: 0 .. _lib.MAP_MAX_GAP;
        above 0 one gap of at most end_gap bases is also tried at each end of every chain, between the read's end and the outermost
        seed (gasm_batch_map_reads_gapped_ends; the rule: "End gaps"), and the map has end_records() and end_counters().  A pass of its
        own: what map_reads() returned stays what it was."""
        if not 0 <= int(max_edits) <= MAP_MAX_MISMATCH:
            raise ValueError(f"max_edits must be 0..{MAP_MAX_MISMATCH}")
        if not 0 <= int(max_gap) <= MAP_MAX_GAP:
            raise ValueError(f"max_gap must be 0..{MAP_MAX_GAP}")
        if not 0 <= int(end_gap) <= MAP_MAX_GAP:
            raise ValueError(f"end_gap must be 0..{MAP_MAX_GAP}")
        max_edits, max_gap, end_gap = int(max_edits), int(max_gap), int(end_gap)
        if end_gap:
            check(lib().gasm_batch_map_reads_gapped_ends(self.h, max_edits, max_gap, end_gap))
        else:
            check(lib().gasm_batch_map_reads_gapped(self.h, max_edits, max_gap))
        ps = [C.c_void_p() for _ in range(6)]
        check(lib().gasm_batch_fetch_read_map_gapped(self.h, *[C.byref(p) for p in ps]))
        seg, o, contigs = self._contigs_by_segment()
        total = int(o[-1]) if int(seg[-1]) else 0
        rec, gap = _arr(ps[0], C.c_int32, 4 * self.n_reads), _arr(ps[1], C.c_int32, 4 * self.n_reads)
        pile, gpile = _arr(ps[2], C.c_uint32, 4 * total), _arr(ps[3], C.c_uint32, 2 * total)
        hist, cnt = _arr(ps[4], C.c_uint32, self.n_segments * (max_edits + 1)), _arr(ps[5], C.c_uint64, self.n_segments * len(MAPG_FIELDS))
        strands = self.strands()
        ends = {}
        if end_gap:
            pe = [C.c_void_p() for _ in range(2)]
            check(lib().gasm_batch_fetch_read_map_ends(self.h, *[C.byref(p) for p in pe]))
            ends = dict(end_gap=end_gap, rec_end=_arr(pe[0], C.c_int32, 4 * self.n_reads), end_counters=_arr(pe[1], C.c_uint64, self.n_segments * len(MAPEND_FIELDS)))
        return GappedReadMap(self.k, strands, max_edits, max_gap, contigs, rec, gap, pile, gpile, hist, cnt,
                             [t.tolist() for t in self.contig_twins()] if strands == 2 else None, getattr(self, "_seg_read_off", None), **ends)

    def align_reads(self, max_edits=6, max_gap=3, end_gap=3):
        """map_reads_gapped(max_edits, max_gap, end_gap) that keeps every read's alignment (gasm_batch_map_reads_aligned; include/gasm.h
        "Alignments") as a readmap.AlignedReadMap: GappedReadMap's tables, the same values, and per read the pieces of its best chain
        (pieces(), cigars(), to_sam()) and per contig base the bases of the insertions in front of it (insert_pileup(), insertions(),
        consensus() with the insertions applied).  end_gap = 0 is legal: no end gap is taken and the end tables are zero.  It is the
        batch's gapped mapping: score_mapped(source="gapped") reads it, and a later map_reads_gapped() replaces it."""
        if not 0 <= int(max_edits) <= MAP_MAX_MISMATCH:
            raise ValueError(f"max_edits must be 0..{MAP_MAX_MISMATCH}")
        if not 0 <= int(max_gap) <= MAP_MAX_GAP:
            raise ValueError(f"max_gap must be 0..{MAP_MAX_GAP}")
        if not 0 <= int(end_gap) <= MAP_MAX_GAP:
            raise ValueError(f"end_gap must be 0..{MAP_MAX_GAP}")
        max_edits, max_gap, end_gap = int(max_edits), int(max_gap), int(end_gap)
        check(lib().gasm_batch_map_reads_aligned(self.h, max_edits, max_gap, end_gap))
        ps, pe, pa, cols = [C.c_void_p() for _ in range(6)], [C.c_void_p() for _ in range(2)], [C.c_void_p() for _ in range(2)], C.c_uint32()
        check(lib().gasm_batch_fetch_read_map_gapped(self.h, *[C.byref(p) for p in ps]))
        check(lib().gasm_batch_fetch_read_map_ends(self.h, *[C.byref(p) for p in pe]))
        check(lib().gasm_batch_fetch_read_alignments(self.h, *[C.byref(p) for p in pa], C.byref(cols)))
        seg, o, contigs = self._contigs_by_segment()
        total = int(o[-1]) if int(seg[-1]) else 0
        W = int(cols.value)
        rec, gap = _arr(ps[0], C.c_int32, 4 * self.n_reads), _arr(ps[1], C.c_int32, 4 * self.n_reads)
        pile, gpile = _arr(ps[2], C.c_uint32, 4 * total), _arr(ps[3], C.c_uint32, 2 * total)
        hist, cnt = _arr(ps[4], C.c_uint32, self.n_segments * (max_edits + 1)), _arr(ps[5], C.c_uint64, self.n_segments * len(MAPG_FIELDS))
        strands = self.strands()
        return AlignedReadMap(self.k, strands, max_edits, max_gap, end_gap, contigs, rec, gap, pile, gpile, hist, cnt,
                              _arr(pe[0], C.c_int32, 4 * self.n_reads), _arr(pe[1], C.c_uint64, self.n_segments * len(MAPEND_FIELDS)),
                              _arr(pa[0], C.c_int32, 2 * MAP_MAX_PIECES * self.n_reads), _arr(pa[1], C.c_uint32, 4 * W * total), W,
                              self._read_lengths(), [t.tolist() for t in self.contig_twins()] if strands == 2 else None,
                              getattr(self, "_seg_read_off", None))

    def score_mapped(self, kmer=8, tables=None, source="gapped", partial=False):
        """breakage scores from the records of the last map_reads_gapped() (source="gapped") or map_reads() ("ungapped") over the last
        build (gasm_batch_score_mapped; the rule: include/gasm.h "Mapped scoring") as a readmap.MappedScores: a read scores at the
        contig base under its first base, so reads with errors count too.  tables: None (the normalised query table), one row of
        qtable.ROWS probabilities, or 1 to _lib.MAX_TABLES rows.  partial: reads that start on a contig and run off its end score too.
        A pass of its own: what scores(), score_fixed(), guided() and the mappings returned stays what it was."""
        t = np.ascontiguousarray(qtable.load_normalised() if tables is None else tables, dtype=np.float64)
        if t.ndim == 1:
            t = t.reshape(1, -1)
        if t.ndim != 2 or t.shape[1] != qtable.ROWS:
            raise ValueError(f"tables must be rows of {qtable.ROWS} probabilities")
        if not 1 <= t.shape[0] <= MAX_TABLES:
            raise ValueError(f"tables must hold 1..{MAX_TABLES} rows")
        if source not in MAPSCORE_SOURCES:
            raise ValueError(f"source must be one of {sorted(MAPSCORE_SOURCES)}")
        if int(kmer) < 0:
            raise ValueError("kmer must be >= 0")
        T = int(t.shape[0])
        check(lib().gasm_batch_score_mapped(self.h, MAPSCORE_SOURCES[source], int(kmer), t.ctypes.data_as(C.c_void_p), T, MAPSCORE_PARTIAL if partial else 0))
        seg, o, contigs = self._contigs_by_segment()
        n = int(seg[-1])
        total = int(o[-1]) if n else 0
        per_table = []
        for i in range(T):
            ps, sh = [C.c_void_p() for _ in range(6)], C.c_int()
            check(lib().gasm_batch_fetch_mapped_scores(self.h, i, *[C.byref(p) for p in ps], C.byref(sh)))
            per_table.append((dict(bp_score=_arr(ps[0], C.c_double, n), bp_score_norm_by_break_freqs=_arr(ps[1], C.c_double, n),
                                   bp_score_norm_by_len=_arr(ps[2], C.c_double, n), kmer_breaks=_arr(ps[3], C.c_int32, n),
                                   sequence_len=_arr(ps[4], C.c_int32, n), seg_contig_off=seg), _arr(ps[5], C.c_int64, n), sh.value))
        sp, cp = C.c_void_p(), C.c_void_p()
        check(lib().gasm_batch_fetch_mapped_starts(self.h, C.byref(sp), C.byref(cp)))
        return MappedScores(int(kmer), source, bool(partial), contigs, per_table, _arr(sp, C.c_uint32, total),
                            _arr(cp, C.c_uint64, self.n_segments * len(MAPSCORE_FIELDS)))

    def suggest_cov_cutoff(self, segment):
        """a cov_cutoff for build_simplified() from the last build's own contigs of `segment`: half the length-weighted median of the
        contigs' mean multiplicities (Velvet's -cov_cutoff auto), floored, and at least min_count + 1 of that build (below that the
        rule can match nothing).  The weight of a contig is its number of k-mers.  Host arithmetic over contig_coverage()."""
        floor = getattr(self, "_min_count", 1) + 1
        ms, ns = self.contig_coverage(segment)
        if not len(ns):
            return floor
        return max(floor, weighted_median_half(ms, ns))

    def kmer_spectrum(self):
        """(n_segments, 256) uint64: [s, m] = distinct k-mers of segment s of the last build with multiplicity m (255: that or
        more; column 0 is zero).  Build with min_count = 1, look for the valley, build again with the cutoff there."""
        check(lib().gasm_batch_kmer_spectrum(self.h))
        p = C.c_void_p()
        check(lib().gasm_batch_fetch_kmer_spectrum(self.h, C.byref(p)))
        n = self.n_segments * 256
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(n,)).copy().reshape(self.n_segments, 256)

    def build_plan(self):
        """the path the last build took (gasm_batch_build_plan; finishes a pending build first): a dict of the PLAN_FIELDS of
        the final attempt, and the same row as the one entry of its "blocks" list"""
        rows = lib().gasm_batch_build_plan(self.h, None, 0)
        if rows < 0:
            check(rows)
        out = (C.c_int32 * (rows * len(PLAN_FIELDS)))()
        check(min(0, lib().gasm_batch_build_plan(self.h, out, len(out))))
        blocks = [dict(zip(PLAN_FIELDS, out[j * len(PLAN_FIELDS):(j + 1) * len(PLAN_FIELDS)])) for j in range(rows)]
        return dict(blocks[0], blocks=blocks)

    def score(self, kmer=8, table=None):
        t = np.ascontiguousarray(qtable.load_normalised() if table is None else table, dtype=np.float64)
        if t.size != qtable.ROWS:
            raise ValueError(f"table must hold {qtable.ROWS} probabilities")
        self._table = t
        check(lib().gasm_batch_score(self.h, int(kmer), t.ctypes.data_as(C.c_void_p)))
        return self

    def score_tables(self, kmer, tables):
        """score the last build under 1 to _lib.MAX_TABLES breakage tables at once (gasm_batch_score_tables): the reads are
        matched once, every table gets its own sums — table t's scores(table=t) / score_fixed(table=t) are bit for bit what
        score(kmer, tables[t]) gives.  scores(), score_fixed() and guided() refer to tables[0]."""
        t = np.ascontiguousarray(tables, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != qtable.ROWS:
            raise ValueError(f"tables must be rows of {qtable.ROWS} probabilities")
        self._table = t[0] if len(t) else None
        check(lib().gasm_batch_score_tables(self.h, int(kmer), t.ctypes.data_as(C.c_void_p), t.shape[0]))
        return self

    def count_read_kmers(self):
        """break-k-mer counts of every segment's reads (count_read_kmers, lib/DeNovoAssembler.R:135-168, for k = 2, 4, 6 and 8
        at once): (n_segments, 69 904) uint32 in breakage-table order.  Reads only the packed reads: any build and score of the
        batch are unaffected, before or after."""
        check(lib().gasm_batch_count_read_kmers(self.h))
        p = C.c_void_p()
        check(lib().gasm_batch_fetch_read_kmer_counts(self.h, C.byref(p)))
        n = self.n_segments * qtable.ROWS
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        self._rkc = a.reshape(self.n_segments, qtable.ROWS)
        return self._rkc

    def read_kmer_counts(self, segment, kmer):
        """the 4**kmer counts of one segment and length from the last count_read_kmers() (counted now if there was none)"""
        if getattr(self, "_rkc", None) is None:
            self.count_read_kmers()
        return self._rkc[segment, readkmers.table_slice(kmer)]

    def correct_reads(self):
        """a new SegmentBatch of the same context and layout whose reads are this batch's reads with their substitution errors repaired
        against the distinct k-mers of the last build (gasm_batch_correct_reads; the rule: include/gasm.h "Read correction"): a run of
        weak k-mers that one changed base explains in exactly one way is fixed, everything else is copied.  This batch, its build and
        its scores are untouched; the new batch has no build yet.  correction_stats() of the NEW batch tells what happened."""
        h = C.c_void_p()
        check(lib().gasm_batch_correct_reads(self.h, C.byref(h)))
        new = SegmentBatch.__new__(SegmentBatch)
        new.ctx, new.h, new.k, new._table = self.ctx, h, None, None
        new.n_segments, new.n_reads = self.n_segments, int(lib().gasm_batch_total_reads(h))
        return new

    def correction_stats(self, as_dict=False):
        """of a batch that correct_reads() returned: (n_segments, 6) uint32, the columns in the order of _lib.CORRECT_FIELDS (reads
        without a k-mer, clean, corrected, partly corrected, left; bases changed); as_dict: a dict of the columns by those names"""
        p = C.c_void_p()
        check(lib().gasm_batch_fetch_correct_stats(self.h, C.byref(p)))
        n = self.n_segments * len(CORRECT_FIELDS)
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n,)).copy().reshape(self.n_segments, len(CORRECT_FIELDS))
        return {name: a[:, i] for i, name in enumerate(CORRECT_FIELDS)} if as_dict else a

    def reads(self):
        """(uint8 array of the batch's reads as ASCII, back to back; read_off uint64[n_reads + 1]) (gasm_batch_fetch_reads)"""
        d, o = C.c_void_p(), C.c_void_p()
        check(lib().gasm_batch_fetch_reads(self.h, C.byref(d), C.byref(o)))
        off = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(self.n_reads + 1,)).copy()
        total = int(off[-1])
        data = np.frombuffer(C.string_at(d, total), dtype=np.uint8).copy() if total else np.zeros(0, np.uint8)
        return data, off

    def read_strings(self):
        """the reads as one list of str, in the batch's order (segment after segment)"""
        data, off = self.reads()
        raw = data.tobytes()
        return [raw[int(off[i]):int(off[i + 1])].decode() for i in range(self.n_reads)]

    def total_kmers(self):
        return int(lib().gasm_batch_total_kmers(self.h))

    def distinct(self):
        """(seg_off[n_segments+1], keys uint64, multiplicities uint32, words)"""
        so, ks, ms, w = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
        check(lib().gasm_batch_fetch_distinct(self.h, C.byref(so), C.byref(ks), C.byref(ms), C.byref(w)))
        seg = np.ctypeslib.as_array(C.cast(so, C.POINTER(C.c_uint64)), shape=(self.n_segments + 1,)).copy()
        n = int(seg[-1])
        keys = np.ctypeslib.as_array(C.cast(ks, C.POINTER(C.c_uint64)), shape=(n * w.value,)).copy() if n else np.zeros(0, np.uint64)
        mult = np.ctypeslib.as_array(C.cast(ms, C.POINTER(C.c_uint32)), shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        return seg, keys, mult, w.value

    def distinct_kmers(self, segment):
        seg, keys, mult, w = self.distinct()
        a, b = int(seg[segment]), int(seg[segment + 1])
        return unpack_kmers(keys[a * w:b * w], self.k, w), mult[a:b]

    def graph(self):
        """(edge_flags uint8, edge_next uint32), one entry per distinct k-mer in the order of distinct(): bit 0 of a flag = the
        edge's source node is branching, bit 1 (first out-edge of a node) = the node has two or more in-edges; edge_next =
        the edge the walk continues with, 0xFFFFFFFF at the end of a contig (lib/DeNovoAssembler.cpp:125-189)"""
        seg = self.distinct()[0]
        n = int(seg[-1])
        fl, nx = C.c_void_p(), C.c_void_p()
        check(lib().gasm_batch_fetch_graph(self.h, C.byref(fl), C.byref(nx)))
        if not n:
            return np.zeros(0, np.uint8), np.zeros(0, np.uint32)
        return (np.ctypeslib.as_array(C.cast(fl, C.POINTER(C.c_uint8)), shape=(n,)).copy(),
                np.ctypeslib.as_array(C.cast(nx, C.POINTER(C.c_uint32)), shape=(n,)).copy())

    def contigs_raw(self):
        """(seg_contig_off[n_segments+1], contig base offsets[n_contigs+1], ASCII bytes)"""
        so, off, data = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().gasm_batch_fetch_contigs(self.h, C.byref(so), C.byref(off), C.byref(data)))
        seg = np.ctypeslib.as_array(C.cast(so, C.POINTER(C.c_uint64)), shape=(self.n_segments + 1,)).copy()
        nc = int(seg[-1])
        o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(nc + 1,)).copy()
        raw = C.string_at(data, int(o[-1])) if nc and o[-1] else b""
        return seg, o, raw

    def _contigs_by_segment(self):
        """(seg_contig_off, contig base offsets, the contig strings of every segment)"""
        seg, o, raw = self.contigs_raw()
        return seg, o, [[raw[int(o[c]):int(o[c + 1])].decode() for c in range(int(seg[s]), int(seg[s + 1]))] for s in range(self.n_segments)]

    def contigs(self, segment=None, one_per_pair=False):
        """contig strings per segment (or of one segment).  one_per_pair (after a strands = 2 build): of every contig and its
        reverse-complement twin only the first is kept (c <= twin[c]: self-twins stay)"""
        seg, o, raw = self.contigs_raw()
        rng = range(self.n_segments) if segment is None else [segment]
        tw = self.contig_twins() if one_per_pair else None
        out = [[raw[int(o[c]):int(o[c + 1])].decode() for c in range(int(seg[s]), int(seg[s + 1]))
                if tw is None or c - int(seg[s]) <= int(tw[s][c - int(seg[s])])] for s in rng]
        return out if segment is None else out[0]

    def strands(self):
        """strands of the last build (0 before the first)"""
        return int(lib().gasm_batch_strands(self.h))

    def contig_twins(self, segment=None):
        """after a strands = 2 build: per segment a uint32 array, twin[c] = index in the segment's contig list of the contig
        that is contig c's reverse complement (gasm_batch_fetch_contig_twins); twin[twin[c]] == c"""
        p = C.c_void_p()
        check(lib().gasm_batch_fetch_contig_twins(self.h, C.byref(p)))
        seg = self.contigs_raw()[0]
        n = int(seg[-1])
        tw = _arr(p, C.c_uint32, n)
        out = [tw[int(seg[s]):int(seg[s + 1])] for s in range(self.n_segments)]
        return out if segment is None else out[segment]

    def scores(self, table=0):
        """dict of per-contig arrays, in contigs_raw() order; table: which table of the last score_tables"""
        ps = [C.c_void_p() for _ in range(5)]
        check(lib().gasm_batch_fetch_scores_table(self.h, int(table), *[C.byref(p) for p in ps]))
        seg, _, _ = self.contigs_raw()
        n = int(seg[-1])
        return dict(bp_score=_arr(ps[0], C.c_double, n), bp_score_norm_by_break_freqs=_arr(ps[1], C.c_double, n),
                    bp_score_norm_by_len=_arr(ps[2], C.c_double, n), kmer_breaks=_arr(ps[3], C.c_int32, n),
                    sequence_len=_arr(ps[4], C.c_int32, n), seg_contig_off=seg)

    def score_fixed(self, table=0):
        """(int64 fixed-point breakage sums per contig, shift): bp_score == fx * 2**-shift exactly; table: which table of
        the last score_tables (each has its own shift)"""
        p, sh = C.c_void_p(), C.c_int()
        check(lib().gasm_batch_fetch_score_fixed_table(self.h, int(table), C.byref(p), C.byref(sh)))
        seg, _, _ = self.contigs_raw()
        n = int(seg[-1])
        return _arr(p, C.c_int64, n), sh.value

    def guided(self):
        """breakage-score-guided scaffolds (not in the reference) of a built + scored batch:
        list per segment of dicts(sequence, bp_score, bp_score_norm_by_len, kmer_breaks), longest first"""
        check(lib().gasm_batch_guided(self.h))
        ps = [C.c_void_p() for _ in range(6)]
        check(lib().gasm_batch_fetch_guided(self.h, *[C.byref(p) for p in ps]))
        seg = np.ctypeslib.as_array(C.cast(ps[0], C.POINTER(C.c_uint64)), shape=(self.n_segments + 1,)).copy()
        n = int(seg[-1])
        off = np.ctypeslib.as_array(C.cast(ps[1], C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        raw = C.string_at(ps[2], int(off[-1])) if n and off[-1] else b""
        bp, nl, br = _arr(ps[3], C.c_double, n), _arr(ps[4], C.c_double, n), _arr(ps[5], C.c_int32, n)
        return [[dict(sequence=raw[int(off[i]):int(off[i + 1])].decode(), bp_score=bp[i], bp_score_norm_by_len=nl[i], kmer_breaks=int(br[i]))
                 for i in range(int(seg[s]), int(seg[s + 1]))] for s in range(self.n_segments)]

    def close(self):
        if self.h:
            lib().gasm_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
