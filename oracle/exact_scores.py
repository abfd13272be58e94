"""Exact reference of calc_breakscore's scores (TEST INFRASTRUCTURE ONLY).

A second restatement of lib/DeNovoAssembler.cpp:325-426, independent of liborc: for each path, every distinct read's
first occurrence (str.find; "" hits at 0) gives a break window (:366-386); the window's table row collects the read's
multiplicity.  A window the table does not hold has probability 0 but still counts in the total (:386-390, operator[]).
From the integer row counts the three scores follow as exact rationals:
    bp_score                      = sum_w p(w) * c(w)
    bp_score_norm_by_break_freqs  = bp_score / total            (0 when there are no hits)
    bp_score_norm_by_len          = bp_score / len(path)        (NaN for an empty path: 0/0 in the reference)
Non-finite table entries follow IEEE double semantics over the rows that are hit (c != 0 is skipped, so 0 * NaN is never
formed): NaN if a NaN row is hit or both +inf and -inf are, +-inf otherwise.

The numeric contract the GPU scorers are held to is written out in check_fp64 and check_fixed below;
u = 2^-53, m = the path's hit count (kmer_breaks), S = sum |p * c|."""
import math
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)


def window(path, pos, kmer):
    """the break window of a hit at `pos` (lib/DeNovoAssembler.cpp:366-386), cut short by the end of the path"""
    start = max(0, pos - kmer // 2)
    width = 8
    if start == 0 and pos in (1, 2, 3):
        width = 2 * pos
    return path[start:start + width]


class PathExact:
    """exact scores of one path; `counts` maps each hit window to its integer count (missing windows included)"""

    def __init__(self, length, counts, table):
        self.length = length
        self.counts = counts
        self.kmer_breaks = sum(counts.values())
        self.m = self.kmer_breaks
        probs = [(table.get(w, 0.0), c) for w, c in counts.items() if c]
        nan = any(math.isnan(p) for p, _ in probs)
        pinf = any(p == math.inf for p, _ in probs)
        ninf = any(p == -math.inf for p, _ in probs)
        self.finite = not (nan or pinf or ninf)
        if self.finite:
            # every double is n / 2^e: the sums are integers over the largest of those powers of two
            self._probs = [(p.as_integer_ratio(), c) for p, c in probs]
            d = max((r[1] for r, _ in self._probs), default=1)
            self.bp = Fraction(sum(n * (d // dn) * c for (n, dn), c in self._probs), d)
            self.S = Fraction(sum(abs(n) * (d // dn) * c for (n, dn), c in self._probs), d)
            self.nf = self.bp / self.kmer_breaks if self.kmer_breaks else Fraction(0)
            self.nl = self.bp / length if length else None
        else:
            v = math.nan if nan or (pinf and ninf) else (math.inf if pinf else -math.inf)
            self.bp = self.nf = v
            self.nl = v if length else math.nan
            self.S = None

    def fixed_sum(self, shift):
        """sum over the hits of round(p * 2^shift) * c, rounding half to even (llrint): the batch scorer's integer sum"""
        assert self.finite
        tot = 0
        for (n, d), c in self._probs:
            q, r = divmod(n << shift, d)
            if 2 * r > d or (2 * r == d and q & 1):
                q += 1
            tot += q * c
        return tot

    def row_freq(self, keys):
        """path_freq in the order of `keys` (np.float64): the correctly rounded c / total (NaN for every row when total is 0)"""
        ix = _key_index(keys)
        c = np.zeros(len(keys), dtype=np.float64)
        for w, n in self.counts.items():
            for j in ix.get(w, ()):
                c[j] = n
        with np.errstate(all="ignore"):
            return c / np.float64(self.kmer_breaks)


_INDEX = {}


def _key_index(keys):
    """{key: positions in keys}, kept per keys object (the 69 904-row key list is asked for once per path)"""
    hit = _INDEX.get(id(keys))
    if hit is None or hit[0] is not keys:
        ix = {}
        for j, k in enumerate(keys):
            ix.setdefault(k, []).append(j)
        hit = _INDEX[id(keys)] = (keys, ix)
    return hit[1]


def _first_hits(path, by_len):
    """{read: first position} for the reads that occur in `path`; by_len: {length: {read: multiplicity}}"""
    hits = {}
    n = len(path)
    for L, group in by_len.items():
        if L > n:
            continue
        if L == 0 or len(group) < 8:
            for r in group:
                p = path.find(r)
                if p >= 0:
                    hits[r] = p
        else:           # index the path's L-long substrings once: one pass instead of a find() per read
            left = len(group)
            for j in range(n - L + 1):
                s = path[j:j + L]
                if s in group and s not in hits:
                    hits[s] = j
                    left -= 1
                    if not left:
                        break
    return hits


def score_paths(paths, reads, table, kmer):
    """exact scores of every path against the reads; `table`: dict window -> probability"""
    mult = {}
    for r in reads:
        mult[r] = mult.get(r, 0) + 1
    by_len = {}
    for r, c in mult.items():
        by_len.setdefault(len(r), {})[r] = c
    out = []
    for path in paths:
        counts = {}
        for r, p in _first_hits(path, by_len).items():
            w = window(path, p, kmer)
            counts[w] = counts.get(w, 0) + mult[r]
        out.append(PathExact(len(path), counts, table))
    return out


def fixed_shift(table_values, max_reads):
    """the batch scorer's fixed-point shift, restated: the shift with max|p| * max(1, max_reads) * 2^shift in (2^60, 2^61],
    None where the table holds NaN / infinity or that shift lies outside [0, 1000] (FP64 scoring); 62 for a table of zeros"""
    v = np.asarray(table_values, dtype=np.float64)
    if not np.isfinite(v).all():
        return None
    mx = Fraction(float(np.abs(v).max(initial=0.0)))
    if mx == 0:
        return 62
    x = mx * max(1, int(max_reads))
    c = 0                                   # ceil(log2 x)
    while Fraction(2) ** c < x:
        c += 1
    while c > -1100 and Fraction(2) ** (c - 1) >= x:
        c -= 1
    shift = 61 - c
    return shift if 0 <= shift <= 1000 else None


# ---------------------------------------------------------------------------------------------------------------- checks
def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def same(a, b):
    """bit-for-bit equality of two doubles (NaN equals NaN)"""
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (math.isnan(a) and math.isnan(b))


def same_array(a, b):
    """bit-for-bit equality of two double arrays (NaN equals NaN)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


REL = 2.0 ** -36


def rel_close(a, b):
    """|a - b| <= 2^-36 |b| elementwise (so exactly 0 where b is 0): the relative bound every comparison of GPU scores with
    the oracle's hash-order doubles meets for the standard table"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) <= REL * np.abs(b)


def _near(got, exact, bound):
    if not isinstance(exact, Fraction):            # non-finite exact value: IEEE semantics
        return same(got, exact) or (math.isnan(got) and math.isnan(exact))
    return math.isfinite(got) and abs(Fraction(got) - exact) <= bound


def check_fp64(ex, bp, nf, nl, breaks=None, tag=""):
    """FP64 position path: |got - exact| <= (m+2) u S for bp_score and (m+2) u S / total for norm_by_break_freqs (any
    summation order, FMA or not); norm_by_len == bp_score / len bit for bit"""
    if breaks is not None:
        assert int(breaks) == ex.kmer_breaks, (tag, "kmer_breaks", int(breaks), ex.kmer_breaks)
    if ex.finite:
        b = (ex.m + 2) * U * ex.S
        assert _near(bp, ex.bp, b), (tag, "bp_score", bp, float(ex.bp), float(b))
        assert _near(nf, ex.nf, b / ex.kmer_breaks if ex.kmer_breaks else 0), (tag, "norm_by_break_freqs", nf, float(ex.nf))
    else:
        assert same(bp, ex.bp) and same(nf, ex.nf), (tag, "non-finite", bp, nf, ex.bp)
    assert same(nl, _div(bp, ex.length)), (tag, "norm_by_len", nl, bp, ex.length)


def check_fixed(ex, bp, nf, nl, fx, shift, breaks=None, tag=""):
    """fixed-point path: fx is the exact integer sum; bp == float(fx) 2^-shift, nf == bp / kmer_breaks (0 without hits) and
    nl == bp / len bit for bit; |bp - exact| <= m 2^-(shift+1) + u |exact|"""
    assert ex.finite, (tag, "a non-finite table reached the fixed-point path")
    if breaks is not None:
        assert int(breaks) == ex.kmer_breaks, (tag, "kmer_breaks", int(breaks), ex.kmer_breaks)
    want_fx = ex.fixed_sum(shift)
    assert int(fx) == want_fx, (tag, "fx", int(fx), want_fx, shift)
    want = float(int(fx)) * 2.0 ** -shift
    assert same(bp, want), (tag, "bp_score != fx 2^-shift", bp, want)
    assert same(nf, _div(bp, ex.kmer_breaks) if ex.kmer_breaks else 0.0), (tag, "norm_by_break_freqs", nf)
    assert same(nl, _div(bp, ex.length)), (tag, "norm_by_len", nl)
    assert _near(bp, ex.bp, ex.m * Fraction(1, 2 ** (shift + 1)) + U * abs(ex.bp)), (tag, "bp_score bound", bp, float(ex.bp), shift)
