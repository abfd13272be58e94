"""PairPlaces: where the read pairs of a batch lie on the contigs of its last build (include/gasm.h, "Read pairs"), as
SegmentBatch.place_pairs() fetches it — and what to do with it on the host: the insert size, the links that fragments make between
contigs, and the resolution of repeats that are longer than a read.  The tables come from the GPU (k_pair_place); everything here is
host arithmetic over them."""
import numpy as np

from ._lib import PAIR_FIELDS
from .links import NONE, chain_joins


def quantiles(hist, max_insert):
    """(q01, median, q99) of an insert histogram (max_insert + 1 bins, the last the overflow bin), from bins 1 .. max_insert - 1: q_p is
    the smallest d whose cumulative count is >= ceil(p * total).  ValueError when those bins are empty."""
    h = [int(v) for v in hist[1:max_insert]]
    total = sum(h)
    if total == 0:
        raise ValueError("no pair with both mates on one contig inside the histogram: no insert size")
    want = [-(-total * num // den) for num, den in ((1, 100), (1, 2), (99, 100))]
    out, cum, q = [], 0, 0
    for d, c in enumerate(h, start=1):
        cum += c
        while q < 3 and cum >= want[q]:
            out.append(d)
            q += 1
    return tuple(out)


class PairPlaces:
    """The three tables of gasm_batch_fetch_pair_places with the contigs they speak of, per segment.  Contig indices are the ones inside
    the segment (the order of SegmentBatch.contigs(segment)).  An ORIENTED PAIR is a pair in one orientation: orientation 0 = (mate 1,
    mate 2), and after a strands = 2 build orientation 1 = (mate 2, mate 1) as well."""

    def __init__(self, k, strands, max_insert, orientations, contigs, rec, insert_hist, counters):
        self.k, self.strands, self.max_insert, self.orientations = int(k), int(strands), int(max_insert), int(orientations)
        self._contigs = contigs                                      # list per segment of str
        self.n_segments = len(contigs)
        self._cnt = np.asarray(counters, dtype=np.uint64).reshape(self.n_segments, len(PAIR_FIELDS))
        self._hist = np.asarray(insert_hist, dtype=np.uint32).reshape(self.n_segments, self.max_insert + 1)
        # the six counters of a segment sum to its pairs x orientations
        per_seg = self._cnt.sum(axis=1) // np.uint64(max(self.orientations, 1))
        self.seg_pair_off = np.concatenate([[0], np.cumsum(per_seg)]).astype(np.uint64)
        self.n_pairs = int(self.seg_pair_off[-1])
        self._rec = np.asarray(rec, dtype=np.int32).reshape(self.orientations, self.n_pairs, 4)

    def _seg(self, segment):
        s = int(segment)
        if not 0 <= s < self.n_segments:
            raise IndexError(f"segment {segment} of {self.n_segments}")
        return s

    def contigs(self, segment):
        return self._contigs[self._seg(segment)]

    def records(self, segment):
        """(orientations, pairs, 4) int32: c1, S, c2, E of every oriented pair of the segment; a contig of -1 (position 0) = unplaced"""
        s = self._seg(segment)
        return self._rec[:, int(self.seg_pair_off[s]):int(self.seg_pair_off[s + 1])]

    def insert_hist(self, segment):
        """(max_insert + 1,) uint32: [d] = oriented pairs with both mates on one contig and E - S = d > 0; the last bin: d >= max_insert"""
        return self._hist[self._seg(segment)]

    def counters(self, segment, as_dict=False):
        """(6,) uint64 in the order of _lib.PAIR_FIELDS: skipped, none_placed, one_placed, same_contig, reversed, diff_contig"""
        c = self._cnt[self._seg(segment)]
        return {name: int(c[i]) for i, name in enumerate(PAIR_FIELDS)} if as_dict else c

    def insert_size(self, segment):
        """(q01, median, q99) of the segment's insert sizes (quantiles(): the overflow bin is left out; ValueError without any)"""
        return quantiles(self.insert_hist(segment), self.max_insert)

    def _across(self, segment):
        """{(c1, c2): [(S, E), ...]} over the oriented pairs of the segment with both mates placed"""
        out = {}
        for c1, S, c2, E in self.records(segment).reshape(-1, 4).tolist():
            if c1 >= 0 and c2 >= 0:
                out.setdefault((c1, c2), []).append((S, E))
        return out

    def mate_links(self, segment):
        """the sorted (a, b, n, mean_gap) over the oriented pairs whose mates lie on two contigs, c1 = a != c2 = b: n such pairs, and
        the mean over them of the gap one pair implies, median insert - (len(a) - S) - E: the bases between the end of a and the start
        of b.  Two contigs that overlap by k - 1 bases have gap -(k - 1).  ValueError where the segment has no insert size."""
        cs = self.contigs(segment)
        across = {ab: v for ab, v in self._across(segment).items() if ab[0] != ab[1]}
        if not across:
            return []
        med = self.insert_size(segment)[1]
        return sorted((a, b, len(v), sum(med - (len(cs[a]) - S) - E for S, E in v) / len(v)) for (a, b), v in across.items())

    def resolve_repeats(self, segment, links, min_support=2, insert_range=None):
        """the segment's contigs with the repeats resolved that the read pairs resolve; the sorted unique list of str.  Host code.
        links: the links.ContigLinks of the same build (its succ / pred give the topology).  A contig r of ANY length is a candidate under
        the topological conditions of ContigLinks.resolve_repeats: m >= 2 contigs in and m out; r is the only way on from its
        predecessors a_i and the only way back from its successors b_j; none of them is r itself.  Its matrix is M[i][j] = the oriented
        pairs with c1 = a_i, c2 = b_j and lo <= (len(a_i) - S) + len(r) - 2 (k - 1) + E <= hi: the length the fragment would have if it
        ran from a_i THROUGH r into b_j.  a_i == b_j is included (a same-contig pair counts if it would fit through r).  (lo, hi) =
        insert_range, by default (q01, q99) of insert_size(segment); without an insert size nothing is resolved.  r is RESOLVED if M is a
        permutation matrix with every chosen entry >= min_support and zeros elsewhere; the joins a_i . r . b_sigma(i), their chaining,
        closed chains and the output are those of ContigLinks.resolve_repeats (links.chain_joins).  STATED LIMITS: a mixed matrix stays
        as it is; so does a tandem repeat entered from itself, a repeat longer than the insert (no fragment reaches across it), and an
        insert distribution so wide that the range admits the wrong pairing of flanks."""
        if int(min_support) < 1:
            raise ValueError("min_support must be >= 1")
        cs = self.contigs(segment)
        if list(links.contigs(segment)) != list(cs) or links.k != self.k:
            raise ValueError("links and pair places speak of different builds")
        if insert_range is None:
            try:
                q = self.insert_size(segment)
            except ValueError:
                return sorted(set(cs))
            insert_range = (q[0], q[2])
        lo, hi = int(insert_range[0]), int(insert_range[1])
        if lo > hi:
            raise ValueError("insert_range must be (lo, hi) with lo <= hi")
        k = self.k
        succ = [[int(v) for v in row] for row in links.succ(segment)]
        pred = [[int(v) for v in row] for row in links.pred(segment)]
        across = self._across(segment)
        right, left, resolved = {}, {}, set()
        for r in range(len(cs)):
            ins, outs = [a for a in pred[r] if a != NONE], [b for b in succ[r] if b != NONE]
            m = len(ins)
            if m < 2 or len(outs) != m or r in ins or r in outs:
                continue
            if sum(v != NONE for v in succ[ins[0]]) != 1 or sum(v != NONE for v in pred[outs[0]]) != 1:
                continue
            through = len(cs[r]) - 2 * (k - 1)
            M = [[sum(1 for S, E in across.get((a, b), ()) if lo <= (len(cs[a]) - S) + through + E <= hi) for b in outs] for a in ins]
            sigma = []
            for i in range(m):
                nz = [j for j in range(m) if M[i][j] != 0]
                if len(nz) != 1 or M[i][nz[0]] < int(min_support):
                    break
                sigma.append(nz[0])
            if len(sigma) != m or sorted(sigma) != list(range(m)):
                continue
            resolved.add(r)
            for i in range(m):
                right[ins[i]] = (r, outs[sigma[i]])
                left[outs[sigma[i]]] = (ins[i], r)
        return chain_joins(cs, k, right, left, resolved)
