"""CPU restatement of the bubble-popping rule (include/gasm.h, "Bubble popping"), by composition with tests/tips_ref.py and the
oracle (TEST INFRASTRUCTURE: imported by the bubbles tests only).  Per segment:
    kept = tips_ref.solid_kmers(...), then tips_ref.clip(kept, k, tip_len, tip_rounds)       (tips go first)
    per round:  contigs = orc.get_contigs(kept, k, 1, rows=1)["contigs"]
                those of at most bubble_len bases, grouped by (first k-1 bases, last k-1 bases)
                in a group, a contig loses all its k-mers if another one has a STRICTLY higher mean multiplicity
                (m(d) * n(c) > m(c) * n(d), exact integers; no tie-break)
"""
import collections

import numpy as np

import tips_ref as tr

MAX_BUBBLE_ROUNDS = 8
MAX_BUBBLE_LEN = 65535


def bubbles_of(contigs, mult, k, bubble_len):
    """the rule on one graph: the contigs to pop.  mult: dict k-mer -> multiplicity of the current set"""
    groups = collections.defaultdict(list)
    for c in contigs:
        if len(c) <= bubble_len:
            n = len(c) - k + 1
            groups[(c[:k - 1], c[-(k - 1):])].append((c, n, sum(mult[c[i:i + k]] for i in range(n))))
    popped = []
    for g in groups.values():
        for c, n, m in g:
            if any(d != c and md * n > m * nd for d, nd, md in g):
                popped.append(c)
    return popped


def pop(kept, k, bubble_len, bubble_rounds):
    """exactly bubble_rounds rounds on the multiset `kept`.  Returns (remaining multiset, bubbles per round, k-mers per round,
    contigs before every round, popped contigs per round), the stats padded with zeros to MAX_BUBBLE_ROUNDS"""
    bub_n, kmers_n, before, popped = [0] * MAX_BUBBLE_ROUNDS, [0] * MAX_BUBBLE_ROUNDS, [], []
    if bubble_len <= 0:
        return kept, bub_n, kmers_n, before, popped
    for r in range(bubble_rounds):
        contigs = tr.contigs_of(kept, k)["contigs"]
        before.append(contigs)
        bub = bubbles_of(contigs, collections.Counter(kept), k, bubble_len)
        gone = {c[i:i + k] for c in bub for i in range(len(c) - k + 1)}
        bub_n[r], kmers_n[r] = len(bub), len(gone)
        popped.append(bub)
        kept = [x for x in kept if x not in gone]
    return kept, bub_n, kmers_n, before, popped


def expected(rs, k, min_count=1, strands=1, tip_len=0, tip_rounds=1, bubble_len=0, bubble_rounds=1):
    """the oracle composition for one segment: tips_ref.expected's dict (ref = get_contigs of what is left, tips, kmers per
    tip round, cnt, solid) plus after_tips (the contigs of the clipped set), bubbles, bubble_kmers (per bubble round),
    before (the contigs before every bubble round) and popped (the contigs popped in every round)"""
    kept, cnt = tr.solid_kmers(rs, k, min_count, strands)
    solid = len(set(kept))
    kept, tips_n, kmers_n, _ = tr.clip(kept, k, tip_len, tip_rounds)
    after_tips = tr.contigs_of(kept, k)["contigs"]
    kept, bub_n, bk_n, before, popped = pop(kept, k, bubble_len, bubble_rounds)
    return dict(ref=tr.contigs_of(kept, k), tips=tips_n, kmers=kmers_n, bubbles=bub_n, bubble_kmers=bk_n, before=before, popped=popped,
                after_tips=after_tips, cnt=cnt, solid=solid)


def _rnd(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def nested_case(seed=3):
    """the hand-built case of two rounds (k = 21): G (300 random bases) covered 4x by its 241 windows of 60 bases; a branch
    B = G[100:120] + X + G[150:170] (X: 80 random bases, drawn after G) given 3 times, which leaves the backbone and rejoins it
    around a backbone stretch of another length; B2 = B with base 60 cycled A->C->G->T->A, given once: a bubble inside B.
    Returns (reads, G)."""
    rng = np.random.default_rng(seed)
    G = _rnd(rng, 300)
    X = _rnd(rng, 80)
    B = G[100:120] + X + G[150:170]
    B2 = B[:60] + "ACGTA"["ACGT".index(B[60]) + 1] + B[61:]
    return [G[i:i + 60] for i in range(241)] * 4 + [B] * 3 + [B2], G


P = "ACGTTGCATGCCGATTACGGATCCAGT"
Q = "TTGACCGTAGGCTAACGTCAGGATCAA"


def tie_case(first_twice=False):
    """two parallel paths P+A+Q and P+C+Q of mean multiplicity 1 (nobody is popped); the first read twice: the C branch goes"""
    return [P + "A" + Q] * (2 if first_twice else 1) + [P + "C" + Q]


_CACHE = {}


def noisy_segments(L, rl, cov, seed, strands, n_seg=1, rate=0.01):
    """the tests' noisy input: synth.make_batch(n_seg, L, rl, cov, seed0=seed), tips_ref.noisy(reads, rate, seed + 1) and, for
    strands = 2, tips_ref.flip_half(reads, seed).  Returns (reads array, seg_off, the reads of every segment as strings)"""
    from genomeassembler_dev_amd import synth
    reads, seg_off, _ = synth.make_batch(n_seg, L, rl, cov, seed0=seed)
    if rate:
        reads = tr.noisy(reads, rate, seed + 1)
    if strands == 2:
        reads = tr.flip_half(reads, seed)
    return reads, seg_off, [tr.strs(reads[int(seg_off[s]):int(seg_off[s + 1])]) for s in range(n_seg)]


def expected_cached(rs, k, min_count=1, strands=1, tip_len=0, tip_rounds=1, bubble_len=0, bubble_rounds=1):
    """expected(...), computed once per process for the same reads and arguments (rounds that are not read count as 0): the host
    and the GPU tests of one run, and the tests of one module, share the references they have in common.  Read-only."""
    key = (len(rs), hash(tuple(rs)), k, min_count, strands, tip_len, tip_rounds if tip_len else 0, bubble_len, bubble_rounds if bubble_len else 0)
    if key not in _CACHE:
        _CACHE[key] = expected(rs, k, min_count, strands, tip_len, tip_rounds, bubble_len, bubble_rounds)
    return _CACHE[key]
