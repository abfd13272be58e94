"""ReadMap: what SegmentBatch.map_reads() returns — per read its best place on the contigs within max_mismatch substitutions, per contig
base the four base counts of the reads laid over it, per segment a mismatch histogram and seven counters (the rule and its limits:
include/gasm.h "Read mapping") — and the host arithmetic on top: depth, mapped fraction, error rate, consensus, variants."""
import numpy as np

from ._lib import MAP_FIELDS, MAPEND_FIELDS, MAPG_FIELDS, MAPSCORE_FIELDS

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
