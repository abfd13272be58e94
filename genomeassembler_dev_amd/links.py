"""ContigLinks: the graph between the contigs of a build and the reads' support for it (include/gasm.h, "Contig links"), as
SegmentBatch.contig_links() fetches it — and what to do with it on the host: the sorted link list, GFA 1 output, and the resolution of
repeats that are shorter than a read.  The tables come from the GPU (k_contig_links, k_read_thread); everything here is host
arithmetic over them."""
import numpy as np

NONE = 0xFFFFFFFF
BASES = "ACGT"


def resolve_segment(contigs, k, span_len, succ, pred, span_support, min_support=2):
    """resolve_repeats() of one segment from its tables: contigs (list of str), succ / pred (n x 4, NONE = 0xFFFFFFFF), span_support
    (n x 4 x 4).  Returns the sorted unique list of resolved contig strings (the rule: ContigLinks.resolve_repeats)."""
    if int(min_support) < 1:
        raise ValueError("min_support must be >= 1")
    n = len(contigs)
    succ = [[int(v) for v in row] for row in succ]
    pred = [[int(v) for v in row] for row in pred]
    right, left, resolved = {}, {}, set()          # flank -> (repeat, next flank); flank -> (previous flank, repeat)
    for r in range(n):
        if len(contigs[r]) > span_len:
            continue
        xs = [x for x in range(4) if pred[r][x] != NONE]
        ys = [y for y in range(4) if succ[r][y] != NONE]
        m = len(xs)
        if m < 2 or len(ys) != m:
            continue
        ins, outs = [pred[r][x] for x in xs], [succ[r][y] for y in ys]
        if r in ins or r in outs:
            continue
        # r is the only way on from its predecessors (out(u(r)) == 1) and the only way back from its successors (in(v(r)) == 1)
        if sum(v != NONE for v in succ[ins[0]]) != 1 or sum(v != NONE for v in pred[outs[0]]) != 1:
            continue
        S = [[int(span_support[r][x][y]) for y in ys] for x in xs]
        sigma = []
        for i in range(m):
            nz = [j for j in range(m) if S[i][j] != 0]
            if len(nz) != 1 or S[i][nz[0]] < int(min_support):
                break
            sigma.append(nz[0])
        if len(sigma) != m or sorted(sigma) != list(range(m)):
            continue
        resolved.add(r)
        for i in range(m):
            a, b = ins[i], outs[sigma[i]]
            assert a not in right and b not in left, "a flank has at most one join on each side"
            right[a] = (r, b)
            left[b] = (a, r)
    return chain_joins(contigs, k, right, left, resolved)


def chain_joins(contigs, k, right, left, resolved):
    """the output of a repeat resolution from its joins a . r . b: right[a] = (r, b), left[b] = (a, r), resolved = the repeats r.  The joins
    form simple chains of flanks with copies of repeats in between, overlapping by k-1 bases: each chain is one contig, a chain that closes
    on itself is cut in front of its smallest flank, contigs in no join come out unchanged, resolved repeats do not come out on their
    own.  Returns the sorted unique list of str (shared by ContigLinks.resolve_repeats and pairs.PairPlaces.resolve_repeats)."""
    n = len(contigs)
    assert not (resolved & (set(right) | set(left))), "a resolved repeat is never the flank of another one"

    def text(chain):
        s = contigs[chain[0]]
        for c in chain[1:]:
            s += contigs[c][k - 1:]
        return s

    out, seen = [], set()
    for a in sorted(set(right) - set(left)):                        # open chains, from their first flank
        chain = [a]
        while chain[-1] in right:
            r, b = right[chain[-1]]
            chain += [r, b]
        seen.update(chain[0::2])
        out.append(text(chain))
    for a in sorted(set(right)):                                     # what is left closes on itself: a is the smallest flank of its cycle
        if a in seen:
            continue
        chain = [a]
        while True:
            r, b = right[chain[-1]]
            chain.append(r)
            if b == a:
                break
            chain.append(b)
        seen.update(chain[0::2])
        out.append(text(chain))
    out += [contigs[c] for c in range(n) if c not in resolved and c not in right and c not in left]
    return sorted(set(out))


class ContigLinks:
    """The five tables of gasm_batch_fetch_contig_links with the contigs they speak of, per segment.  Contig indices are the ones inside
    the segment (the order of SegmentBatch.contigs(segment)); bases A, C, G, T are 0..3."""

    def __init__(self, k, span_len, strands, seg_contig_off, contigs, succ, pred, link_support, span_support, skipped, mult_sum):
        self.k, self.span_len, self.strands = int(k), int(span_len), int(strands)
        self.seg_contig_off = np.asarray(seg_contig_off, dtype=np.uint64)
        self.n_segments = len(self.seg_contig_off) - 1
        self._contigs = contigs                                      # list per segment of str
        self._succ, self._pred, self._lsup = succ.reshape(-1, 4), pred.reshape(-1, 4), link_support.reshape(-1, 4)
        self._ssup = span_support.reshape(-1, 4, 4)
        self.skipped = np.asarray(skipped, dtype=np.uint64)          # per segment: reads of more than THREAD_MAX_KMERS k-mers, not threaded
        self._msum = np.asarray(mult_sum, dtype=np.uint64)

    def _rng(self, segment):
        s = int(segment)
        if not 0 <= s < self.n_segments:
            raise IndexError(f"segment {segment} of {self.n_segments}")
        return int(self.seg_contig_off[s]), int(self.seg_contig_off[s + 1])

    def contigs(self, segment):
        self._rng(segment)
        return self._contigs[int(segment)]

    def succ(self, segment):
        """(n, 4) uint32: [a, x] = the contig whose first k-mer is v(a) + base x, or 0xFFFFFFFF"""
        a, z = self._rng(segment)
        return self._succ[a:z]

    def pred(self, segment):
        """(n, 4) uint32: [b, x] = the contig whose last k-mer is base x + u(b), or 0xFFFFFFFF"""
        a, z = self._rng(segment)
        return self._pred[a:z]

    def link_support(self, segment):
        """(n, 4) uint32: [a, x] = crossings of the link (a, succ[a, x]) in the threaded reads"""
        a, z = self._rng(segment)
        return self._lsup[a:z]

    def span_support(self, segment):
        """(n, 4, 4) uint32: [r, x, y] = reads that enter r over the in-edge x + u(r), run through it and leave over v(r) + y"""
        a, z = self._rng(segment)
        return self._ssup[a:z]

    def mult_sum(self, segment):
        a, z = self._rng(segment)
        return self._msum[a:z]

    def links(self, segment):
        """the sorted (a, b, support) triples of the segment's links"""
        su, ls = self.succ(segment), self.link_support(segment)
        return sorted((a, int(su[a, x]), int(ls[a, x])) for a in range(len(su)) for x in range(4) if int(su[a, x]) != NONE)

    def to_gfa(self, segment):
        """the segment's graph as GFA 1 text: one S line per contig (named by its index, KC:i: = the sum of its k-mers' multiplicities,
        m(c) of contig_coverage()) and one `L a + b + {k-1}M RC:i:{support}` line per link.  After a strands = 2 build a contig and its
        reverse-complement twin are SEPARATE S records, each with its own links (contig_twins() pairs them): the two orientations are
        not folded into one segment with +/- ends."""
        cs, ms = self.contigs(segment), self.mult_sum(segment)
        lines = ["H\tVN:Z:1.0"]
        lines += [f"S\t{c}\t{cs[c]}\tKC:i:{int(ms[c])}" for c in range(len(cs))]
        lines += [f"L\t{a}\t+\t{b}\t+\t{self.k - 1}M\tRC:i:{n}" for a, b, n in self.links(segment)]
        return "\n".join(lines) + "\n"

    def resolve_repeats(self, segment, min_support=2):
        """the segment's contigs with the repeats resolved that the threaded reads resolve; the sorted unique list of str.  Host code.
        r is a RESOLVED REPEAT if len(r) <= span_len; in(u(r)) == out(v(r)) == m >= 2; out(u(r)) == 1 and in(v(r)) == 1 (r is the only way
        on from its predecessors and the only way back from its successors); no predecessor or successor is r itself; and the m x m
        span-support matrix over the existing in- and out-bases has a permutation sigma with S[i][sigma(i)] >= min_support for every i
        while every other entry is exactly 0.  Each resolved repeat gives the joins a_i . r . b_sigma(i), overlapping by k-1 bases.  A
        flank has at most one join on each side, so the joins form simple chains of flanks with copies of repeats in between: each chain
        is one output contig; a chain that closes on itself is cut in front of its smallest contig index (of its flanks: a repeat may
        occur in it twice) and ends with the repeat copy that leads back there; contigs in no join come out unchanged; resolved repeats
        do not come out on their own.  STATED LIMITS: anything else stays as it is — a mixed matrix, a tandem repeat entered from
        itself, a repeat longer than the reads."""
        return resolve_segment(self.contigs(segment), self.k, self.span_len, self.succ(segment), self.pred(segment), self.span_support(segment),
                               min_support)
