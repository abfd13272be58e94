"""CPU restatement of the tip-clipping rule (include/gasm.h, "Tip clipping"), by composition with the oracle (TEST
INFRASTRUCTURE: imported by the tips tests only).  Per segment:
    km   = orc.kmers_from_reads(rs [+ their reverse complements], k)
    kept = the k-mers of km seen at least min_count times               (a multiset: multiplicities stay true)
    per round:  contigs = orc.get_contigs(kept, k, 1, rows=1)["contigs"]
                in / out lists of every (k-1)-mer from the distinct k-mers of kept
                a contig of at most tip_len bases that is a forward or a backward tip loses all its k-mers
"""
import collections

import numpy as np

from oracle import orc

MAX_TIP_ROUNDS = 8
_COMP = str.maketrans("ACGT", "TGCA")
_COMP_LUT = np.zeros(256, dtype=np.uint8)
_COMP_LUT[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)
EMPTY = dict(contigs=[], distinct=[], counts=np.zeros(0, np.int64))


def rc(s):
    return s[::-1].translate(_COMP)


def strs(a):
    return [r.tobytes().decode() for r in a]


def flip_half(reads, seed):
    """reverse-complement a random half of the rows of a (n, read_len) uint8 array: default_rng(seed).random(n) < 0.5"""
    m = np.random.default_rng(seed).random(reads.shape[0]) < 0.5
    out = reads.copy()
    out[m] = _COMP_LUT[reads[m][:, ::-1]]
    return out


def noisy(reads, rate, seed):
    """substitute each base with probability `rate`: a mask, then a shift of 1..3 mod 4 in ACGT"""
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    code = np.zeros(256, dtype=np.uint8)
    code[lut] = np.arange(4, dtype=np.uint8)
    mask = rng.random(reads.shape) < rate
    shift = rng.integers(1, 4, reads.shape).astype(np.uint8)
    c = code[reads]
    return np.where(mask, lut[(c + shift) & 3], reads).astype(np.uint8)


def solid_kmers(rs, k, min_count=1, strands=1):
    """(the k-mer multiset that survives the cutoff, Counter of all k-mers)"""
    km = orc.kmers_from_reads(rs + [rc(r) for r in rs] if strands == 2 else rs, k)
    cnt = collections.Counter(km)
    return [x for x in km if cnt[x] >= min_count], cnt


def contigs_of(kept, k):
    return orc.get_contigs(kept, k, 1, rows=1) if kept else EMPTY


def tips_of(contigs, mult, k, tip_len):
    """rules 2-4 on one graph: the contigs to clip.  mult: dict k-mer -> multiplicity of the current set"""
    out_e, in_e = collections.defaultdict(list), collections.defaultdict(list)
    for e in mult:
        out_e[e[:-1]].append(e)
        in_e[e[1:]].append(e)
    tips = []
    for c in contigs:
        if len(c) > tip_len:
            continue
        u, v, e_first, e_last = c[:k - 1], c[-(k - 1):], c[:k], c[-k:]
        forward = not out_e.get(v) and any(f != e_first and mult[f] > mult[e_first] for f in out_e.get(u, ()))
        backward = not in_e.get(u) and any(f != e_last and mult[f] > mult[e_last] for f in in_e.get(v, ()))
        if forward or backward:
            tips.append(c)
    return tips


def clip(kept, k, tip_len, tip_rounds):
    """exactly tip_rounds rounds on the multiset `kept`.  Returns (remaining multiset, tips per round, k-mers per round,
    contigs before every round), the stats padded with zeros to MAX_TIP_ROUNDS"""
    tips_n, kmers_n, before = [0] * MAX_TIP_ROUNDS, [0] * MAX_TIP_ROUNDS, []
    if tip_len <= 0:
        return kept, tips_n, kmers_n, before
    for r in range(tip_rounds):
        contigs = contigs_of(kept, k)["contigs"]
        before.append(contigs)
        tips = tips_of(contigs, collections.Counter(kept), k, tip_len)
        gone = {c[i:i + k] for c in tips for i in range(len(c) - k + 1)}
        tips_n[r], kmers_n[r] = len(tips), len(gone)
        kept = [x for x in kept if x not in gone]
    return kept, tips_n, kmers_n, before


def expected(rs, k, min_count=1, strands=1, tip_len=0, tip_rounds=1):
    """the oracle composition for one segment: dict(ref = get_contigs of the clipped set, tips, kmers (per round), before =
    the contigs before every round, cnt = Counter of all k-mers, solid = distinct k-mers that survived the cutoff)"""
    kept, cnt = solid_kmers(rs, k, min_count, strands)
    solid = len(set(kept))
    kept, tips_n, kmers_n, before = clip(kept, k, tip_len, tip_rounds)
    return dict(ref=contigs_of(kept, k), tips=tips_n, kmers=kmers_n, before=before, cnt=cnt, solid=solid)


def two_round_case(strands=1, equal=False, seed=3):
    """the hand-built case of two rounds (k = 21, tip_len = 41): a 300-base random backbone G covered 4x by 60-base windows at
    every offset, a branch T = G[130:150] + 12 random bases given 3 times, a sub-branch S = T[-27:-7] + 4 random bases given
    once.  Round 0 clips S (T is no dead end yet: S hangs on it), round 1 the re-joined T.  equal: T is given as often as the
    competing backbone edge is covered (both strands double both alike), so T stays.  Returns (reads, G)."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)

    def rnd(n):
        return letters[rng.integers(0, 4, n)].tobytes().decode()
    G = rnd(300)
    T = G[130:150] + rnd(12)
    S = T[-27:-7] + rnd(4)
    windows = [G[i:i + 60] for i in range(len(G) - 60 + 1)]
    reads = windows * 4
    if equal:
        # the backbone edge that competes with T's first edge is G[130:151]: every window that holds it, times 4
        n_back = 4 * sum(1 for w in windows if G[130:151] in w)
        reads = reads + [T] * n_back
    else:
        reads = reads + [T] * 3
    reads = reads + [S]
    return reads, G
