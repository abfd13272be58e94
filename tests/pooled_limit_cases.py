"""Inputs that take the pooled exchange past its plan-scan and merge-table limits (plain module: builders only, numpy only —
no test functions, no libgasm).

The plan kernels scan their run-length tables 8 192 entries per pass with a carry between passes; `k_bucket_merge` holds at
most LIMIT distinct keys per bucket; `k_repack_reads` / `k_piece_positions` move read pieces that need not start on a word
boundary.  Every case here is built from seeds alone so that one of those edges is reached;
tests/test_pooled_limit_cases_host.py proves the properties with the CPU oracle, tests/test_pooled_limits_gpu.py runs the
kernels.

A case builds to a dict: reads ([n, rl] uint8 ASCII, segment after segment), seg_off (uint64, n_segments + 1), rl, k, bbits,
worlds, and deal(world) -> one (reads, seg_off) per rank.  `reads` is what a single-GPU build of the same input takes: the
ranks' shares concatenated (a read dealt to two ranks is there twice)."""
import collections
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "genomeassembler_dev_amd", "csrc")
PASS_ENTRIES = 8192

Case = collections.namedtuple("Case", "name build")


def merge_limit(words):
    """distinct keys one bucket of `k_bucket_merge` may hold for keys of `words` 64-bit words, read off the sources: the kernel's
    own expression with the table size of its instantiation, which must agree with what the host passes the plan kernels"""
    src = open(os.path.join(CSRC, "kernels_pool.hip")).read()
    tbl = {m.group(1): int(m.group(2)) for m in re.finditer(r"template __global__ void k_bucket_merge<(\w+), (\d+)>", src)}
    expr = re.search(r"constexpr int LIMIT = (TBL / \d+ \* \d+);", src).group(1)
    a, b = (int(v) for v in re.match(r"TBL / (\d+) \* (\d+)", expr).groups())
    limit = tbl["u64" if words == 1 else "K128"] // a * b
    hdr = open(os.path.join(CSRC, "kernels.h")).read()
    base = int(re.search(r"#define GASM_TBL_LIMIT (\d+)", hdr).group(1))
    host = re.search(r"const u32 limit = words == 1 \? GASM_TBL_LIMIT : GASM_TBL_LIMIT / (\d+);", open(os.path.join(CSRC, "exchange.hip")).read())
    assert limit == (base if words == 1 else base // int(host.group(1))), (limit, base)
    return limit


def strs(a):
    return [r.tobytes().decode() for r in a]


def shard_reads(reads, seg_off, rank, world):
    """rank's share of the reads of every segment (every world-th read), with its own seg_read_off"""
    parts, off = [], [0]
    for s in range(len(seg_off) - 1):
        r = reads[int(seg_off[s]):int(seg_off[s + 1])][rank::world]
        parts.append(r)
        off.append(off[-1] + r.shape[0])
    return np.concatenate(parts, axis=0), np.array(off, dtype=np.uint64)


def _genome(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]


def _reads_at(g, starts, rl):
    return np.stack([g[a:a + rl] for a in starts]) if len(starts) else np.zeros((0, rl), np.uint8)


def _batch(parts, rl):
    off = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.uint64)
    return np.concatenate(parts, axis=0).reshape(-1, rl), off


# ------------------------------------------------------------------------------------------------ A: more than one scan pass
def _scan_case(seed, n_seg, bbits, k, rl, worlds):
    """tiny segments (200-400 random bases, reads at 6-10x); segment 1 has no reads, segment 2 a single one"""
    def build():
        rng = np.random.default_rng(seed)
        parts = []
        for s in range(n_seg):
            L, cov = int(rng.integers(200, 401)), int(rng.integers(6, 11))
            g = _genome(rng, L)
            n = 0 if s == 1 else 1 if s == 2 else L * cov // rl
            parts.append(_reads_at(g, rng.integers(0, L - rl + 1, n), rl))
        reads, seg_off = _batch(parts, rl)
        return dict(reads=reads, seg_off=seg_off, rl=rl, k=k, bbits=bbits, worlds=worlds,
                    deal=lambda world: [shard_reads(reads, seg_off, r, world) for r in range(world)])
    return build


# World 1 is there because only the send-side scan of plan 1 runs over all n_segments << bbits entries at every world size: the
# receive-side and capacity scans run over a rank's own buckets, and at world 1 those are all of them.
SCAN_CASES = [
    Case("A1", _scan_case(9101, 33, 8, 9, 20, (1, 3, 5, 8))),        # 8 448 entries: one past the first pass
    Case("A2", _scan_case(9102, 17, 10, 13, 30, (5,))),          # 17 408 entries: a third pass
    Case("A3", _scan_case(9103, 9, 10, 33, 40, (1, 2, 7))),      # 9 216 entries, 128-bit keys
]
SCAN_ENTRIES_ABOVE = {"A1": PASS_ENTRIES, "A2": 2 * PASS_ENTRIES, "A3": PASS_ENTRIES}


# ------------------------------------------------------------------------------------------------ B: the merge table at its limit
def _limit_case(seed, k, extra):
    """One segment, one bucket, three ranks.  A random sequence with exactly LIMIT + extra k-mers is cut into reads that
    overlap by k - 1 bases (consecutive reads share no k-mer, together they hold every k-mer once); read i goes to rank i % 3, and
    every fourth read to the next rank as well, so the ranks' runs overlap partly and each is far below the limit."""
    def build():
        rl, world = 60, 3
        limit = merge_limit(1 if k <= 31 else 2)
        rng = np.random.default_rng(seed)
        L = limit + extra + k - 1
        g = _genome(rng, L)
        starts = list(range(0, L - rl, rl - k + 1)) + [L - rl]
        per_rank = [[] for _ in range(world)]
        for i, a in enumerate(starts):
            per_rank[i % world].append(a)
            if i % 4 == 0:
                per_rank[(i + 1) % world].append(a)
        dealt = [_reads_at(g, st, rl) for st in per_rank]
        reads = np.concatenate(dealt, axis=0)
        seg_off = np.array([0, reads.shape[0]], dtype=np.uint64)
        return dict(reads=reads, seg_off=seg_off, rl=rl, k=k, bbits=0, worlds=(world,), limit=limit, union=limit + extra,
                    deal=lambda w: [(d, np.array([0, d.shape[0]], dtype=np.uint64)) for d in dealt])
    return build


LIMIT_CASES = [Case(f"B-k{k}-limit{'+1' if extra else ''}", _limit_case(9200 + k + extra, k, extra)) for k in (21, 35) for extra in (0, 1)]


# ------------------------------------------------------------------------------------------------ C: read pieces
def _piece_case(seed, rl, k, worlds):
    """5 segments whose base counts are no multiple of 32.  Of segment s's reads rank s % W gets none, rank (s + 1) % W exactly
    one, the others share the rest in turn: every owner puts its segments together from several pieces, some of them shorter
    than one 32-base word, most of them starting inside a word of the sender's read stream."""
    def build():
        rng = np.random.default_rng(seed)
        gens, parts = [], []
        for s in range(5):
            L = int(rng.integers(200, 401))
            g = _genome(rng, L)
            n = L * 8 // rl
            while (n * rl) % 32 == 0 or n < 12:
                n += 1
            gens.append(g)
            parts.append(_reads_at(g, rng.integers(0, L - rl + 1, n), rl))
        reads, seg_off = _batch(parts, rl)

        def deal(world):
            mine = [[[] for _ in range(5)] for _ in range(world)]
            for s in range(5):
                others = [r for r in range(world) if r not in (s % world, (s + 1) % world)]
                for i in range(parts[s].shape[0]):
                    mine[(s + 1) % world if i == 0 else others[i % len(others)]][s].append(i)
            out = []
            for r in range(world):
                out.append(_batch([parts[s][mine[r][s]].reshape(-1, rl) for s in range(5)], rl))
            return out
        return dict(reads=reads, seg_off=seg_off, rl=rl, k=k, bbits=2, worlds=worlds, deal=deal)
    return build


PIECE_CASES = [Case("C-rl20", _piece_case(9301, 20, 9, (4, 6))), Case("C-rl33", _piece_case(9302, 33, 13, (4, 6)))]


# ------------------------------------------------------------------------------------------------ host-side views of a case
def bucket_of(kmers, k, bbits):
    """bucket prefix of k-mer strings: the top bbits bits of the 2k-bit key (base 0 most significant, A=0 C=1 G=2 T=3)"""
    if bbits == 0 or not len(kmers):
        return np.zeros(len(kmers), dtype=np.int64)
    m = (bbits + 1) // 2
    a = np.frombuffer("".join(km[:m] for km in kmers).encode(), dtype=np.uint8).reshape(-1, m)
    code = np.zeros(256, dtype=np.int64)
    code[[ord(c) for c in "ACGT"]] = np.arange(4)
    v = np.zeros(a.shape[0], dtype=np.int64)
    for j in range(m):
        v = v * 4 + code[a[:, j]]
    return v >> (2 * m - bbits)


def run_lengths(reads, seg_off, k, bbits):
    """distinct k-mers per (segment, bucket) of a read set: what gasm_pool_local_runs reports, from string sets"""
    n_seg = len(seg_off) - 1
    out = np.zeros(n_seg << bbits, dtype=np.int64)
    for s in range(n_seg):
        kmers = set()
        for r in strs(reads[int(seg_off[s]):int(seg_off[s + 1])]):
            kmers.update(r[i:i + k] for i in range(len(r) - k + 1))
        if kmers:
            out[s << bbits:(s + 1) << bbits] = np.bincount(bucket_of(sorted(kmers), k, bbits), minlength=1 << bbits)
    return out
