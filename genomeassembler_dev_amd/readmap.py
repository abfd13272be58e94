"""ReadMap: what SegmentBatch.map_reads() returns — per read its best place on the contigs within max_mismatch substitutions, per contig
base the four base counts of the reads laid over it, per segment a mismatch histogram and seven counters (the rule and its limits:
include/gasm.h "Read mapping") — and the host arithmetic on top: depth, mapped fraction, error rate, consensus, variants."""
import numpy as np

from ._lib import MAP_FIELDS, MAP_MAX_PIECES, MAPEND_FIELDS, MAPG_FIELDS, MAPSCORE_FIELDS

RECORD = np.dtype([("contig", np.int32), ("diagonal", np.int32), ("mismatches", np.int32), ("blocks", np.int32), ("overlap", np.int32)])
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


class ReadMap:
    def __init__(self, k, strands, max_mismatch, contigs, rec, pile, mismatch_hist, counters, twins=None, seg_read_off=None):
        """contigs: per segment the list of contig strings; rec: 4 int32 per read of the batch; pile: 4 uint32 per contig base of the
        batch; mismatch_hist: max_mismatch + 1 per segment; counters: len(MAP_FIELDS) per segment; twins (strands = 2): per segment
        the twin map; seg_read_off: n_segments + 1 read indices (None, for a batch that does not know them: the segments' read counts
        are then taken from the sums of their first six counters)."""
        self.k, self.strands, self.max_mismatch = int(k), int(strands), int(max_mismatch)
        self._contigs = [list(c) for c in contigs]
        self.n_segments = len(self._contigs)
        self._cnt = np.asarray(counters, dtype=np.uint64).reshape(self.n_segments, len(MAP_FIELDS))
        self._hist = np.asarray(mismatch_hist, dtype=np.uint32).reshape(self.n_segments, self.max_mismatch + 1)
        if seg_read_off is None:
            self._read_off = np.concatenate([[0], np.cumsum(self._cnt[:, :6].sum(axis=1).astype(np.int64))])
        else:
            self._read_off = np.asarray(seg_read_off, dtype=np.int64)
        self._rec = np.asarray(rec, dtype=np.int32).reshape(-1, 4)
        if len(self._read_off) != self.n_segments + 1 or len(self._rec) != int(self._read_off[-1]):
            raise ValueError("the segments' read offsets do not fit the records")
        lens = [len(s) for cs in self._contigs for s in cs]
        self._pile = np.asarray(pile, dtype=np.uint32).reshape(-1, 4)
        if len(self._pile) != sum(lens):
            raise ValueError("the pileup does not have four counts per contig base")
        self._base_off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
        self._seg_c = np.concatenate([[0], np.cumsum([len(cs) for cs in self._contigs])])
        self._twins = twins

    def _seg(self, segment):
        if not 0 <= int(segment) < self.n_segments:
            raise IndexError(f"segment {segment} of {self.n_segments}")
        return int(segment)

    def contigs(self, segment):
        return list(self._contigs[self._seg(segment)])

    def records(self, segment, as_struct=False):
        """(reads, 5) int32: contig inside the segment, diagonal, mismatches, accepted blocks, overlap of every read's best block;
        -1, 0, 0, 0, 0 for a read with no place.  as_struct: the same as a structured array of dtype readmap.RECORD"""
        s = self._seg(segment)
        r = self._rec[int(self._read_off[s]):int(self._read_off[s + 1])]
        out = np.stack([r[:, 0], r[:, 1], r[:, 2] & 0xFFFF, r[:, 2] >> 16, r[:, 3]], axis=1).astype(np.int32) if len(r) else np.zeros((0, 5), np.int32)
        return out.view(RECORD).reshape(-1) if as_struct else out

    def pileup(self, segment, fold_twins=False):
        """one (len(c), 4) uint32 array per contig: the A, C, G, T counts of the reads laid over every base.  fold_twins (after a
        strands = 2 build): contig c gets pile[twin(c)][len - 1 - p][3 - x] added — the reads of the other strand"""
        s = self._seg(segment)
        c0 = int(self._seg_c[s])
        own = [self._pile[int(self._base_off[c0 + c]):int(self._base_off[c0 + c + 1])].copy() for c in range(len(self._contigs[s]))]
        if not fold_twins:
            return own
        if self._twins is None:
            raise ValueError("fold_twins needs a strands = 2 build")
        return [own[c] + own[int(self._twins[s][c])][::-1, ::-1] for c in range(len(own))]

    def mismatch_hist(self, segment):
        return self._hist[self._seg(segment)].copy()

    def counters(self, segment, as_dict=False):
        c = self._cnt[self._seg(segment)].copy()
        return {name: int(v) for name, v in zip(MAP_FIELDS, c)} if as_dict else c

    def depth(self, segment, fold_twins=False):
        """one uint32 array per contig: reads laid over every base"""
        return [p.sum(axis=1, dtype=np.uint32) for p in self.pileup(segment, fold_twins)]

    def mapped_fraction(self, segment):
        """(mapped_one + mapped_multi) / reads; 0.0 for a segment without reads"""
        c = self.counters(segment)
        n = int(c[:6].sum())
        return (int(c[4]) + int(c[5])) / n if n else 0.0

    def error_rate(self, segment):
        """mismatches / overlap over the reads' best blocks; 0.0 if nothing is mapped"""
        r = self.records(segment)
        r = r[r[:, 0] >= 0]
        ov = int(r[:, 4].sum())
        return int(r[:, 2].sum()) / ov if ov else 0.0

    def consensus(self, segment, min_depth=3, fold_twins=False):
        """the contigs with every base replaced where another base holds a strict majority of a depth of at least min_depth"""
        out = []
        for s, p in zip(self._contigs[self._seg(segment)], self.pileup(segment, fold_twins)):
            t = np.frombuffer(s.encode(), dtype=np.uint8).copy()
            if len(t):
                dp, top = p.sum(axis=1, dtype=np.int64), p.argmax(axis=1)
                win = (dp >= int(min_depth)) & (2 * p.max(axis=1).astype(np.int64) > dp) & (_BASES[top] != t)
                t[win] = _BASES[top][win]
            out.append(t.tobytes().decode())
        return out

    def variants(self, segment, min_depth=8, min_frac=0.2, fold_twins=False):
        """sorted [(contig, position, contig base, other base, its count, depth)] for every position of a depth of at least min_depth
        whose strongest other base (the first in ACGT of equals) has a count > 0 that reaches min_frac of the depth"""
        out = []
        for c, (s, p) in enumerate(zip(self._contigs[self._seg(segment)], self.pileup(segment, fold_twins))):
            if not len(s):
                continue
            t = np.frombuffer(s.encode(), dtype=np.uint8)
            other = p.astype(np.int64)
            other[np.arange(len(t)), np.searchsorted(_BASES, t)] = -1
            dp, top = p.sum(axis=1, dtype=np.int64), other.argmax(axis=1)
            n = other[np.arange(len(t)), top]
            for i in np.nonzero((dp >= int(min_depth)) & (n > 0) & (n >= float(min_frac) * dp))[0]:
                out.append((c, int(i), s[i], "ACGT"[int(top[i])], int(n[i]), int(dp[i])))
        return sorted(out)


class GappedReadMap(ReadMap):
    """what SegmentBatch.map_reads_gapped() returns (the rule and its limits: include/gasm.h "Gapped read mapping"): ReadMap's tables
    over chains — the records' third column is the chain's cost (mismatches + gap lengths), the fourth the accepted chains, the
    histogram is over costs — and beside them per read the gap record of its best chain, per contig base the deletions that skip it and
    the insertions in front of it, and an eighth counter, gapped.  A map made with end_gap > 0 ("End gaps": one gap tried at each end
    of every chain) also holds per read the end gaps of its best chain and per segment four counters; its records' diagonal is the
    first piece's, its gap records count the end pieces, and depth, error_rate, indels and consensus take them as they take a join."""

    def __init__(self, k, strands, max_edits, max_gap, contigs, rec, rec_gap, pile, gap_pile, edit_hist, counters, twins=None, seg_read_off=None,
                 end_gap=0, rec_end=None, end_counters=None):
        """as ReadMap, with rec_gap: 4 int32 per read of the batch (pieces, inserted bases, deleted bases, last diagonal); gap_pile: 2
        uint32 per contig base (deletions, insertions); counters: len(MAPG_FIELDS) per segment; end_gap > 0: rec_end, 4 int32 per
        read (front gap, its breakpoint, back gap, its breakpoint), and end_counters, len(MAPEND_FIELDS) per segment"""
        self._cnt8 = np.asarray(counters, dtype=np.uint64).reshape(len(contigs), len(MAPG_FIELDS))
        super().__init__(k, strands, max_edits, contigs, rec, pile, edit_hist, self._cnt8[:, :len(MAP_FIELDS)], twins, seg_read_off)
        self.max_edits, self.max_gap = int(max_edits), int(max_gap)
        self._gap = np.asarray(rec_gap, dtype=np.int32).reshape(-1, 4)
        self._gpile = np.asarray(gap_pile, dtype=np.uint32).reshape(-1, 2)
        if len(self._gap) != len(self._rec) or len(self._gpile) != len(self._pile):
            raise ValueError("the gap tables do not fit the records and the pileup")
        self.end_gap = int(end_gap)
        self._end = self._endcnt = None
        if self.end_gap:
            self._end = np.asarray(rec_end, dtype=np.int32).reshape(-1, 4)
            self._endcnt = np.asarray(end_counters, dtype=np.uint64).reshape(len(contigs), len(MAPEND_FIELDS))
            if len(self._end) != len(self._rec):
                raise ValueError("the end records do not fit the records")

    def counters(self, segment, as_dict=False):
        c = self._cnt8[self._seg(segment)].copy()
        return {name: int(v) for name, v in zip(MAPG_FIELDS, c)} if as_dict else c

    def edit_hist(self, segment):
        return self.mismatch_hist(segment)

    def gap_records(self, segment):
        """(reads, 4) int32: pieces, inserted bases, deleted bases and last diagonal of every read's best chain; zeros for a read with
        no place"""
        s = self._seg(segment)
        return self._gap[int(self._read_off[s]):int(self._read_off[s + 1])].copy()

    def end_records(self, segment):
        """(reads, 4) int32: front gap (> 0 a deletion, < 0 an insertion, 0 none), its breakpoint, back gap, its breakpoint of every
        read's best chain; zeros for a read with no place.  Only for a map made with end_gap > 0"""
        if self._end is None:
            raise ValueError("this map was made without end gaps (map_reads_gapped(end_gap=...))")
        s = self._seg(segment)
        return self._end[int(self._read_off[s]):int(self._read_off[s + 1])].copy()

    def end_counters(self, segment, as_dict=False):
        """the segment's four end counters (_lib.MAPEND_FIELDS): accepted chains with a front gap, with a back gap, accepted chains
        that the end gaps rescued, reads whose start a front gap moved.  Only for a map made with end_gap > 0"""
        if self._endcnt is None:
            raise ValueError("this map was made without end gaps (map_reads_gapped(end_gap=...))")
        c = self._endcnt[self._seg(segment)].copy()
        return {name: int(v) for name, v in zip(MAPEND_FIELDS, c)} if as_dict else c

    def gap_pileup(self, segment, fold_twins=False):
        """one (len(c), 2) uint32 array per contig: the accepted chains whose deletion skips the base, and those with an insertion in
        front of it.  fold_twins (after a strands = 2 build): the twin's deletions of base len - 1 - p and its insertions in front of
        base len - p (the same place seen from the other strand) are added"""
        s = self._seg(segment)
        c0 = int(self._seg_c[s])
        own = [self._gpile[int(self._base_off[c0 + c]):int(self._base_off[c0 + c + 1])].copy() for c in range(len(self._contigs[s]))]
        if not fold_twins:
            return own
        if self._twins is None:
            raise ValueError("fold_twins needs a strands = 2 build")
        out = []
        for c in range(len(own)):
            t = own[int(self._twins[s][c])]
            f = own[c].copy()
            f[:, 0] += t[::-1, 0]
            f[1:, 1] += t[:0:-1, 1]
            out.append(f)
        return out

    def depth(self, segment, fold_twins=False):
        """one uint32 array per contig: the reads laid over every base, those whose deletion skips it included"""
        return [p.sum(axis=1, dtype=np.uint32) + g[:, 0] for p, g in zip(self.pileup(segment, fold_twins), self.gap_pileup(segment, fold_twins))]

    def error_rate(self, segment):
        """cost / (overlap + inserted bases) over the reads' best chains; 0.0 if nothing is mapped"""
        r, g = self.records(segment), self.gap_records(segment)
        keep = r[:, 0] >= 0
        n = int(r[keep, 4].sum()) + int(g[keep, 1].sum())
        return int(r[keep, 2].sum()) / n if n else 0.0

    def indels(self, segment, min_depth=8, min_frac=0.2, fold_twins=False):
        """sorted [(contig, position, 'D' | 'I', count, depth)] for every position of a depth of at least min_depth at which the
        deletions of the base ('D') or the insertions in front of it ('I') have a count > 0 that reaches min_frac of the depth"""
        out = []
        for c, (g, dp) in enumerate(zip(self.gap_pileup(segment, fold_twins), self.depth(segment, fold_twins))):
            for x, kind in ((0, "D"), (1, "I")):
                n = g[:, x].astype(np.int64)
                for i in np.nonzero((dp >= int(min_depth)) & (n > 0) & (n >= float(min_frac) * dp))[0]:
                    out.append((c, int(i), kind, int(n[i]), int(dp[i])))
        return sorted(out)

    def consensus(self, segment, min_depth=3, fold_twins=False):
        """ReadMap.consensus, and in addition every base is dropped where deletions hold a strict majority of a depth of at least
        min_depth.  Insertions are listed (indels()), not applied: their bases are not recorded"""
        out = []
        for s, g, dp in zip(super().consensus(segment, min_depth, fold_twins), self.gap_pileup(segment, fold_twins), self.depth(segment, fold_twins)):
            t = np.frombuffer(s.encode(), dtype=np.uint8)
            keep = ~((dp >= int(min_depth)) & (2 * g[:, 0].astype(np.int64) > dp)) if len(t) else np.zeros(0, bool)
            out.append(t[keep].tobytes().decode())
        return out


def cigar(read_len, pieces):
    """the CIGAR of a read of read_len bases with the pieces [(s, e, d)] (include/gasm.h, "Alignments"): soft clips for the read bases
    in front of the first and behind the last piece, an M run per piece, between two pieces the step of the diagonal as D (> 0) or I;
    "*" without pieces"""
    if not pieces:
        return "*"
    out = [f"{pieces[0][0]}S"] if pieces[0][0] > 0 else []
    for i, (s, e, d) in enumerate(pieces):
        if i:
            g = d - pieces[i - 1][2]
            out.append(f"{g}D" if g > 0 else f"{-g}I")
        out.append(f"{e - s}M")
    if read_len - pieces[-1][1] > 0:
        out.append(f"{read_len - pieces[-1][1]}S")
    return "".join(out)


class AlignedReadMap(GappedReadMap):
    """what SegmentBatch.align_reads() returns (include/gasm.h "Alignments"): GappedReadMap's tables of a mapping with end gaps, and
    beside them per read the pieces of its best chain — its CIGAR and its SAM line follow — and per contig base the bases of the
    insertions in front of it, column by column, so that insertions() names what was inserted and consensus() applies it.  It holds
    the reads' lengths, not the reads.  The insertion columns are indexed from the insertion's first base, without its length: a
    twin's insertion cannot be reversed column by column, so insert_pileup() and insertions() speak of the contig's own strand only."""

    def __init__(self, k, strands, max_edits, max_gap, end_gap, contigs, rec, rec_gap, pile, gap_pile, edit_hist, counters, rec_end, end_counters,
                 rec_piece, ins_pile, ins_cols, read_len, twins=None, seg_read_off=None):
        """as GappedReadMap (the end tables also for end_gap = 0, where they are zero), with rec_piece: 2 * MAP_MAX_PIECES int32 per
        read of the batch (s | e << 16, d); ins_pile: ins_cols columns of 4 uint32 per contig base; read_len: one length per read"""
        super().__init__(k, strands, max_edits, max_gap, contigs, rec, rec_gap, pile, gap_pile, edit_hist, counters, twins, seg_read_off)
        self.end_gap, self.ins_cols = int(end_gap), int(ins_cols)
        self._end = np.asarray(rec_end, dtype=np.int32).reshape(-1, 4)
        self._endcnt = np.asarray(end_counters, dtype=np.uint64).reshape(len(contigs), len(MAPEND_FIELDS))
        self._piece = np.asarray(rec_piece, dtype=np.int32).reshape(-1, MAP_MAX_PIECES, 2)
        flat = np.asarray(ins_pile, dtype=np.uint32).reshape(-1)
        if len(flat) != 4 * self.ins_cols * len(self._pile):
            raise ValueError("the insertion pileup does not have ins_cols columns per contig base")
        self._ipile = flat.reshape(len(self._pile) if self.ins_cols else 0, self.ins_cols, 4)
        self._len = np.asarray(read_len, dtype=np.int64).reshape(-1)
        if not len(self._end) == len(self._piece) == len(self._len) == len(self._rec):
            raise ValueError("the end records, the piece records and the read lengths do not fit the records")

    def read_lengths(self, segment):
        s = self._seg(segment)
        return self._len[int(self._read_off[s]):int(self._read_off[s + 1])].copy()

    def pieces(self, segment):
        """per read the list [(s, e, d)] of its best chain's pieces, in read order: read bases [s, e) on diagonal d (read base x lies on
        contig base d + x).  Empty for a read with no place"""
        s = self._seg(segment)
        a, b = int(self._read_off[s]), int(self._read_off[s + 1])
        q = self._gap[a:b, 0]
        return [[(int(w) & 0xFFFF, (int(w) >> 16) & 0xFFFF, int(d)) for w, d in p[:n]] for p, n in zip(self._piece[a:b].tolist(), q.tolist())]

    def cigars(self, segment):
        """one CIGAR string per read; "*" for a read with no place (readmap.cigar)"""
        return [cigar(int(n), p) for n, p in zip(self.read_lengths(segment), self.pieces(segment))]

    def to_sam(self, segment, reads=None, names=None):
        """the segment's reads as SAM text: @HD, one @SQ per contig (s{segment}_c{contig}; after a both-strand build both twins), one
        line per read in read order.  A placed read: FLAG 0 (the reads are mapped as given), POS the contig base under its first
        aligned base + 1, MAPQ 255 (not available), its CIGAR, NM:i: the record's cost and XC:i: its accepted chains.  A read with
        no place: FLAG 4.  reads: the segment's read strings for SEQ (else "*"); names: their names (else r0, r1, ...)"""
        s = self._seg(segment)
        rec, ps, lens = self.records(s), self.pieces(s), self.read_lengths(s)
        for given, what in ((reads, "reads"), (names, "names")):
            if given is not None and len(given) != len(rec):
                raise ValueError(f"{what} must hold one entry per read of the segment")
        out = ["@HD\tVN:1.6\tSO:unknown"] + [f"@SQ\tSN:s{s}_c{c}\tLN:{len(t)}" for c, t in enumerate(self._contigs[s])]
        for i, (r, p) in enumerate(zip(rec.tolist(), ps)):
            name = names[i] if names is not None else f"r{i}"
            seq = reads[i] if reads is not None and len(reads[i]) else "*"
            if r[0] < 0:
                out.append(f"{name}\t4\t*\t0\t0\t*\t*\t0\t0\t{seq}\t*")
            else:
                out.append(f"{name}\t0\ts{s}_c{r[0]}\t{p[0][2] + p[0][0] + 1}\t255\t{cigar(int(lens[i]), p)}\t*\t0\t0\t{seq}\t*\tNM:i:{r[2]}\tXC:i:{r[3]}")
        return "\n".join(out) + "\n"

    def insert_pileup(self, segment):
        """one (len(c), ins_cols, 4) uint32 array per contig: [p, l, x] = the accepted chains whose insertion in front of base p has
        base x (A, C, G, T) as its l-th base.  The own strand only: there is no fold over twins"""
        s = self._seg(segment)
        c0 = int(self._seg_c[s])
        if not self.ins_cols:
            return [np.zeros((len(t), 0, 4), np.uint32) for t in self._contigs[s]]
        return [self._ipile[int(self._base_off[c0 + c]):int(self._base_off[c0 + c + 1])].copy() for c in range(len(self._contigs[s]))]

    def insertions(self, segment, min_depth=8, min_frac=0.2):
        """sorted [(contig, position, inserted string, count, depth)] for every position of a depth (GappedReadMap.depth) of at least
        min_depth in front of which the insertions' first column has a count > 0 that reaches min_frac of the depth: the count is that
        column's sum; the string takes the strongest base (the first in ACGT of equals) of every leading column whose sum is still
        > 0 and reaches min_frac of the depth"""
        out = []
        for c, (ip, dp) in enumerate(zip(self.insert_pileup(segment), self.depth(segment))):
            if not ip.shape[1]:
                continue
            n = ip.sum(axis=2, dtype=np.int64)
            ok = (n > 0) & (n >= float(min_frac) * dp[:, None])
            for i in np.nonzero((dp >= int(min_depth)) & ok[:, 0])[0]:
                cols = int(np.argmin(ok[i])) if not ok[i].all() else ip.shape[1]
                out.append((c, int(i), "".join("ACGT"[int(x)] for x in ip[i, :cols].argmax(axis=1)), int(n[i, 0]), int(dp[i])))
        return sorted(out)

    def consensus(self, segment, min_depth=3, fold_twins=False, insertions=True):
        """GappedReadMap.consensus with the insertions applied: in front of every base of a depth of at least min_depth the strongest
        base (the first in ACGT of equals) of every leading column whose sum holds a strict majority of that depth is inserted,
        whether or not the base itself is dropped by a deletion majority.  insertions=False: GappedReadMap.consensus.  The insertion
        columns cannot be folded over twins: fold_twins with insertions raises ValueError"""
        if not insertions:
            return super().consensus(segment, min_depth, fold_twins)
        if fold_twins:
            raise ValueError("the insertion columns cannot be folded over twins: consensus(fold_twins=True, insertions=False)")
        out = []
        for s, g, dp, ip in zip(ReadMap.consensus(self, segment, min_depth), self.gap_pileup(segment), self.depth(segment), self.insert_pileup(segment)):
            deep = dp >= int(min_depth)
            drop = deep & (2 * g[:, 0].astype(np.int64) > dp)
            n = ip.sum(axis=2, dtype=np.int64)
            text = []
            for p, x in enumerate(s):
                for l in range(ip.shape[1] if deep[p] else 0):
                    if 2 * n[p, l] <= dp[p]:
                        break
                    text.append("ACGT"[int(ip[p, l].argmax())])
                if not drop[p]:
                    text.append(x)
            out.append("".join(text))
        return out


def break_window(contig, j, kmer=8):
    """the break window of a hit at position j of `contig`, as a string: the scorer's (lib/DeNovoAssembler.cpp:366-386) — the octamer
    from max(0, j - kmer // 2), 2 / 4 / 6 bases wide for j = 1 / 2 / 3 where it starts at the contig's first base, cut at the contig's end"""
    start = max(0, int(j) - int(kmer) // 2)
    width = {1: 2, 2: 4, 3: 6}.get(int(j), 8) if start == 0 else 8
    return contig[start:start + width]


class MappedScores:
    """what SegmentBatch.score_mapped() returns (the rule and its limits: include/gasm.h "Mapped scoring"): per table the scorer's
    per-contig numbers from the reads' mapped starts, per contig base the reads scored with their start there, per segment the four
    class counters — and the host arithmetic on top."""

    def __init__(self, kmer, source, partial, contigs, per_table, start_pile, counters):
        """contigs: per segment the list of contig strings; per_table: per table (the dict of SegmentBatch.scores(), int64 fx per
        contig, shift); start_pile: one uint32 per contig base of the batch; counters: len(MAPSCORE_FIELDS) per segment"""
        self.kmer, self.source, self.partial = int(kmer), source, bool(partial)
        self._contigs = [list(c) for c in contigs]
        self.n_segments = len(self._contigs)
        self._tables = list(per_table)
        self.n_tables = len(self._tables)
        self._cnt = np.asarray(counters, dtype=np.uint64).reshape(self.n_segments, len(MAPSCORE_FIELDS))
        lens = [len(s) for cs in self._contigs for s in cs]
        self._pile = np.asarray(start_pile, dtype=np.uint32).reshape(-1)
        if len(self._pile) != sum(lens):
            raise ValueError("the start pile does not have one count per contig base")
        self._base_off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
        self._seg_c = np.concatenate([[0], np.cumsum([len(cs) for cs in self._contigs])])

    def _seg(self, segment):
        if not 0 <= int(segment) < self.n_segments:
            raise IndexError(f"segment {segment} of {self.n_segments}")
        return int(segment)

    def _table(self, table):
        if not 0 <= int(table) < self.n_tables:
            raise IndexError(f"table {table} of {self.n_tables}")
        return self._tables[int(table)]

    def contigs(self, segment):
        return list(self._contigs[self._seg(segment)])

    def scores(self, table=0):
        """the dict of SegmentBatch.scores(): per-contig arrays in contigs_raw() order, and seg_contig_off"""
        return dict(self._table(table)[0])

    def score_fixed(self, table=0):
        """(int64 fixed-point breakage sums per contig, shift): bp_score == fx * 2**-shift exactly"""
        t = self._table(table)
        return t[1].copy(), t[2]

    def starts(self, segment):
        """one uint32 array per contig: the reads scored with their start on every base"""
        s = self._seg(segment)
        c0 = int(self._seg_c[s])
        return [self._pile[int(self._base_off[c0 + c]):int(self._base_off[c0 + c + 1])].copy() for c in range(len(self._contigs[s]))]

    def counters(self, segment, as_dict=False):
        c = self._cnt[self._seg(segment)].copy()
        return {name: int(v) for name, v in zip(MAPSCORE_FIELDS, c)} if as_dict else c

    def scored_fraction(self, segment):
        """scored reads / reads (whole, with partial also end_clipped); 0.0 for a segment without reads"""
        c = self.counters(segment)
        n = int(c.sum())
        return (int(c[3]) + (int(c[2]) if self.partial else 0)) / n if n else 0.0

    def window_counts(self, segment, contig):
        """{window string: reads scored with that break window} of one contig of the segment, from starts() and the contig's text: the
        numerators of the reference's path_freq"""
        s = self._seg(segment)
        text, pile = self._contigs[s][contig], self.starts(s)[contig]
        out = {}
        for j in np.nonzero(pile)[0]:
            w = break_window(text, int(j), self.kmer)
            out[w] = out.get(w, 0) + int(pile[j])
        return out
