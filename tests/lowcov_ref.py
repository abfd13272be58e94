"""CPU restatement of the low-coverage rule (include/gasm.h, "Low-coverage removal"), by composition with tests/bubbles_ref.py,
tests/tips_ref.py and the oracle (TEST INFRASTRUCTURE: imported by the lowcov tests only).  Per segment:
    kept = tips_ref.solid_kmers(...), tips_ref.clip(...), bubbles_ref.pop(...)              (tips, then bubbles, go first)
    per round:  contigs = orc.get_contigs(kept, k, 1, rows=1)["contigs"]
                a contig of at most cov_len bases with sum(mult) < cov_cutoff * n loses all its k-mers
                (n = its k-mers; exact integers; a mean equal to the cutoff stays; nothing is asked about its ends)
and, for the coverage fetch, (m, n) of every contig of a k-mer multiset.
"""
import collections

import bubbles_ref as br
import tips_ref as tr

MAX_COV_ROUNDS = 8
MAX_COV_LEN = 65535


def coverage_of(contigs, mult, k):
    """[(m, n)] per contig: the sum of its k-mers' multiplicities and the number of its k-mers.  mult: dict k-mer -> multiplicity"""
    return [(sum(mult[c[i:i + k]] for i in range(len(c) - k + 1)), len(c) - k + 1) for c in contigs]


def lowcov_of(contigs, mult, k, cov_cutoff, cov_len):
    """the rule on one graph: the contigs to remove"""
    return [c for c, (m, n) in zip(contigs, coverage_of(contigs, mult, k)) if len(c) <= cov_len and m < cov_cutoff * n]


def remove(kept, k, cov_cutoff, cov_len, cov_rounds):
    """exactly cov_rounds rounds on the multiset `kept`.  Returns (remaining multiset, contigs per round, k-mers per round, contigs
    before every round, removed contigs per round), the stats padded with zeros to MAX_COV_ROUNDS"""
    cov_n, kmers_n, before, removed = [0] * MAX_COV_ROUNDS, [0] * MAX_COV_ROUNDS, [], []
    if cov_cutoff <= 0 or cov_len <= 0:
        return kept, cov_n, kmers_n, before, removed
    for r in range(cov_rounds):
        contigs = tr.contigs_of(kept, k)["contigs"]
        before.append(contigs)
        low = lowcov_of(contigs, collections.Counter(kept), k, cov_cutoff, cov_len)
        gone = {c[i:i + k] for c in low for i in range(len(c) - k + 1)}
        cov_n[r], kmers_n[r] = len(low), len(gone)
        removed.append(low)
        kept = [x for x in kept if x not in gone]
    return kept, cov_n, kmers_n, before, removed


def expected(rs, k, min_count=1, strands=1, tip_len=0, tip_rounds=1, bubble_len=0, bubble_rounds=1, cov_cutoff=0, cov_len=0, cov_rounds=1):
    """the oracle composition for one segment: bubbles_ref.expected's dict (ref = get_contigs of what is left, tips, kmers, bubbles,
    bubble_kmers, after_tips, cnt, solid) plus after_bubbles (the contigs of the popped set), lowcov, lowcov_kmers (per round),
    before (the contigs before every low-coverage round), removed (the contigs removed in every round) and coverage ([(m, n)] of
    ref's contigs, in their order)"""
    kept, cnt = tr.solid_kmers(rs, k, min_count, strands)
    solid = len(set(kept))
    kept, tips_n, kmers_n, _ = tr.clip(kept, k, tip_len, tip_rounds)
    after_tips = tr.contigs_of(kept, k)["contigs"]
    kept, bub_n, bk_n, _, _ = br.pop(kept, k, bubble_len, bubble_rounds)
    after_bubbles = tr.contigs_of(kept, k)["contigs"]
    kept, cov_n, ck_n, before, removed = remove(kept, k, cov_cutoff, cov_len, cov_rounds)
    ref = tr.contigs_of(kept, k)
    return dict(ref=ref, tips=tips_n, kmers=kmers_n, bubbles=bub_n, bubble_kmers=bk_n, lowcov=cov_n, lowcov_kmers=ck_n, before=before,
                removed=removed, after_tips=after_tips, after_bubbles=after_bubbles, cnt=cnt, solid=solid,
                coverage=coverage_of(ref["contigs"], collections.Counter(kept), k))


_CACHE = {}


def expected_cached(rs, k, min_count=1, strands=1, tip_len=0, tip_rounds=1, bubble_len=0, bubble_rounds=1, cov_cutoff=0, cov_len=0, cov_rounds=1):
    """expected(...), computed once per process for the same reads and arguments (rounds that are not read count as 0).  Read-only."""
    on = cov_cutoff > 0 and cov_len > 0
    key = (len(rs), hash(tuple(rs)), k, min_count, strands, tip_len, tip_rounds if tip_len else 0, bubble_len, bubble_rounds if bubble_len else 0,
           cov_cutoff if on else 0, cov_len if on else 0, cov_rounds if on else 0)
    if key not in _CACHE:
        _CACHE[key] = expected(rs, k, min_count, strands, tip_len, tip_rounds, bubble_len, bubble_rounds, cov_cutoff, cov_len, cov_rounds)
    return _CACHE[key]


def weighted_median_half(cov):
    """floor(median / 2) of the means m / n of cov = [(m, n)], each weighted by n (the first contig, in ascending order of mean, at
    which the running weight reaches half the total): what suggest_cov_cutoff starts from"""
    from fractions import Fraction
    total, run = sum(n for _, n in cov), 0
    for m, n in sorted(cov, key=lambda x: Fraction(x[0], x[1])):
        run += n
        if 2 * run >= total:
            return m // (2 * n)
    return 0


def _backbone(rng, n=300, times=4):
    """G (n random bases) and its windows of 60 bases, each given `times` times: every k-mer of G (k <= 60) is seen at least `times`"""
    G = br._rnd(rng, n)
    return G, [G[i:i + 60] for i in range(n - 60 + 1)] * times


def island_case(seed=3):
    """a backbone covered 4x and an island I (41 random bases, k = 21: a contig of 21 edges with nothing attached) given twice: mean
    multiplicity exactly 2.  Removed at cutoff 3, stays at cutoff 2 (equality).  Returns (reads, G, I)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    G, reads = _backbone(rng)
    I = br._rnd(rng, 41)
    return reads + [I, I], G, I


def link_case(extra=0, seed=4):
    """two backbones G1, G2 covered 4x and a chimeric link of 21 + extra edges of multiplicity 1 that leaves G1 at G1[130:150] and enters
    G2 at G2[150:170] (k = 21): X = G1[130:150] + (1 + extra) bases that differ from both backbones + G2[150:170], given once.  As a contig the link has
    21 + extra edges = 41 + extra bases.  With extra = 0 it goes at cov_len = 41, cutoff 2, and both backbones heal to one contig each;
    with extra = 1 it is one base longer than cov_len and stays.  Returns (reads, G1, G2, X)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    G1, r1 = _backbone(rng)
    G2, r2 = _backbone(rng)
    mid = [x for x in "ACGT" if x not in (G1[150], G2[149])][0] * (1 + extra)      # (neither end of the link runs along a backbone)
    X = G1[130:150] + mid + G2[150:170]
    return r1 + r2 + [X], G1, G2, X
