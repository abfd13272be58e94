"""table_read_kmer_prob of the reference's only_kmers_from_reads mode (lib/DeNovoAssembler.R:135-168) and the number
scripts/01_Real_vs_rand_prob_break_vs_kmers.R reports from it.  The counts come from libgasm (api.count_read_kmers,
SegmentBatch.count_read_kmers); this module only slices, joins and correlates them on the host."""
import itertools

import numpy as np

from . import qtable

KMERS = (2, 4, 6, 8)
ROW = {2: 0, 4: 16, 6: 272, 8: 4368}       # first row of each length in the 69 904-row breakage table


def table_slice(kmer):
    """rows of the kmer-long table inside the 69 904-row breakage table"""
    if kmer not in ROW:
        raise ValueError(f"kmer must be one of {KMERS} (got {kmer})")
    return slice(ROW[kmer], ROW[kmer] + 4 ** kmer)


def table_read_kmer_prob(counts, kmer, prob=None):
    """dict(kmer, prob, count) of one length: the table's k-mers in its (lexicographic) order, their breakage probabilities
    (prob: the 69 904-row table or the 4**kmer rows of this length; default the normalised table the reference loads into
    df_prob) and their read counts, 0 where a k-mer never occurs.  counts: 4**kmer counts in table order, or a 69 904-row
    vector of all lengths (SegmentBatch.count_read_kmers()[segment])."""
    sl = table_slice(kmer)
    n = 4 ** kmer
    c = np.asarray(counts)
    c = c[sl] if c.size == qtable.ROWS else c
    p = qtable.load_normalised() if prob is None else np.asarray(prob, dtype=np.float64)
    p = p[sl] if p.size == qtable.ROWS else p
    if c.size != n or p.size != n:
        raise ValueError(f"kmer={kmer}: need {n} counts and probabilities (or {qtable.ROWS}-row tables)")
    keys = ["".join(t) for t in itertools.product("ACGT", repeat=kmer)]
    return dict(kmer=keys, prob=p.copy(), count=c.astype(np.int64))


def r_squared(prob, count):
    """cor(prob, count)^2 of script 01, unrounded (R applies signif(, 2) only for the plot label); NaN where either
    column is constant"""
    p = np.asarray(prob, dtype=np.float64)
    c = np.asarray(count, dtype=np.float64)
    if p.size < 2 or p.std() == 0 or c.std() == 0:
        return float("nan")
    return float(np.corrcoef(p, c)[0, 1] ** 2)
