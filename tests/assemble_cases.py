"""Inputs of assemble_contigs at the sizes the product runs (plain module: builders only, no test functions).

The device route of assemble_contigs (k_asm_match, k_asm_merge, k_chain_expand, k_str_bitonic*, k_str_adjacent_eq) has
paths that only larger inputs reach: more than 64 / 128 chains in a permutation (a second ballot chunk in the backwards scan
and in the compaction), more than 512 distinct chains (the global bitonic step), overlaps above 32 bases (the second window of
the suffix/prefix test), chains that spell another contig exactly (the full-string test), contigs exactly k-1 long (elements
that contribute no base).  Every case here is built from seeds alone; `claims` names the properties that make a case reach
its path — tests/test_assemble_cases_host.py proves them with the CPU oracle, tests/test_assemble_gpu.py runs the kernels.

A case builds to a dict: form ("graph": contigs + the shuffle matrix as indices; "velvet": contigs + seed, the matrix is
drawn by the call), contigs, perm or None, seed, rows, k, and for graph cases the reads and the genome they came from."""
import collections

import numpy as np

from genomeassembler_dev_amd import synth
from oracle import orc

Case = collections.namedtuple("Case", "name build claims")
# claims (all optional; tests/test_assemble_cases_host.py asserts each one that a case makes):
#   n_exact           the number of contigs, exactly
#   n_above           more contigs than this
#   scaffolds_above   more distinct scaffolds than this (distinct chains are at least as many)
#   spelled           some contig equals a + b[k-1:] for two other contigs a, b whose ends match at k-1
#   has_k1            a contig exactly k-1 long is present, and it is the last k-1 bases of another contig
#   merged_above_32   k-1 > 32, two distinct contigs match at overlap k-1, and the longest scaffold is longer than every contig
#   decoy_above_32    k-1 > 32, and two contigs agree on the first 32 bases of the k-1 suffix/prefix window but not on all of it
#   duplicate         the contig list holds one string twice
#   differential      (no property) the GPU test also runs it with the plain sort and with the host merge
#   score             (no property) the GPU test scores the handle of this one
#   large             the one case beyond 32 768 distinct scaffolds

def _strs(a):
    return [r.tobytes().decode() for r in a]


# ------------------------------------------------------------------------------------------------ graph contigs from reads
def _graph(seed, L, rl, cov, k, rows, **segment):
    def build():
        g = synth.make_segment(seed, L, planted=True, **segment)
        reads = _strs(synth.simulate_reads(g, rl, cov, seed + 1))
        ref = orc.get_contigs(orc.kmers_from_reads(reads, k), k, 1234, rows=rows)
        return dict(form="graph", contigs=ref["contigs"], perm=ref["perm"], seed=None, rows=rows, k=k, reads=reads, truth=g.tobytes().decode())
    return build


# ------------------------------------------------------------------------------------------------ windows of a random genome
def _rnd(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def windows(gseed, L, k, n_cuts, n_extra=4, n_spelled=0, n_k1=0, n_decoy=0, n_target=None):
    """Velvet-form contigs: windows of one random genome that overlap by k-1 (the recipe of
    test_assemble_index_merge_randomised_against_oracle, scaled up), plus
      n_extra    random strings k-1 to 30 long,
      n_spelled  strings from cut i to cut i+2: each equals the chain of two neighbouring windows,
      n_k1       pieces of the genome exactly k-1 long, each the overlap two neighbouring windows share (glued at overlap
                 k-1 such a contig contributes no base),
      n_decoy    (k-1 > 32) strings whose first 32 to k-2 bases continue a window's last k-1 bases and then differ.
    n_target: the sorted distinct list is cut (seeded choice of what goes; spelled, k-1 and decoy strings stay) or
    filled up with random strings of distinct lengths to exactly that many."""
    rng = np.random.default_rng(gseed)
    g = _rnd(rng, L)
    cuts = sorted(set(rng.integers(0, L - k, n_cuts).tolist() + [0]))
    ends = cuts[1:] + [L]
    contigs = [g[a:min(L, b + k - 1)] for a, b in zip(cuts, ends)]
    extras = [_rnd(rng, int(rng.integers(k - 1, 31))) for _ in range(n_extra)]
    keep = []
    for i in rng.choice(len(cuts) - 2, n_spelled, replace=False).tolist() if n_spelled else []:
        keep.append(g[cuts[i]:min(L, cuts[i + 2] + k - 1)])
    for i in rng.choice(np.arange(1, len(cuts)), n_k1, replace=False).tolist() if n_k1 else []:
        keep.append(g[cuts[i]:cuts[i] + k - 1])
    for i in rng.choice(np.arange(1, len(cuts)), n_decoy, replace=False).tolist() if n_decoy else []:
        same = int(rng.integers(32, k - 1))              # bases shared with the window that ends at cut i + k-1
        head = g[cuts[i]:cuts[i] + same]
        wrong = "ACGT"[("ACGT".index(g[cuts[i] + same]) + 1 + int(rng.integers(0, 3))) % 4]
        keep.append(head + wrong + _rnd(rng, int(rng.integers(k, 60))))
    rest = sorted(set(c for c in contigs + extras if len(c) >= k - 1) - set(keep))
    keep = sorted(set(keep))
    if n_target is not None:
        room = n_target - len(keep)
        assert room >= 0
        if len(rest) > room:
            rest = [rest[i] for i in sorted(rng.permutation(len(rest))[:room].tolist())]
        fill = 61
        while len(rest) < room:                          # (longer than every extra: a new string each time)
            s = _rnd(rng, fill)
            fill += 1
            if s not in rest and s not in keep:
                rest.append(s)
    return sorted(set(rest) | set(keep))


def _velvet(k, seed, rows, **recipe):
    def build():
        return dict(form="velvet", contigs=windows(k=k, **recipe), perm=None, seed=seed, rows=rows, k=k, reads=None, truth=None)
    return build


def _fixed(contigs, k, seed, rows):
    def build():
        return dict(form="velvet", contigs=list(contigs), perm=None, seed=seed, rows=rows, k=k, reads=None, truth=None)
    return build


CASES = [
    # ---- graph contigs: the product's own shape and beyond
    Case("graph_k15_73", _graph(72, 12000, 50, 40, 15, 3000, n_short=30, short_len=60, n_long=6, long_len=200, tandem_len=80),
         dict(n_above=64, scaffolds_above=512, differential=True)),
    Case("graph_k15_73_rows120", _graph(72, 12000, 50, 40, 15, 120, n_short=30, short_len=60, n_long=6, long_len=200, tandem_len=80),
         dict(n_above=64, scaffolds_above=512, score=True)),              # (the oracle scores 820 scaffolds in seconds, 11 183 in minutes)
    Case("graph_k9_175", _graph(74, 4000, 30, 40, 9, 3000, n_short=6, short_len=40, n_long=2, long_len=100, tandem_len=40),
         dict(n_above=128, scaffolds_above=512, differential=True)),
    Case("graph_k17_large", _graph(73, 20000, 60, 30, 17, 10000, n_short=40, short_len=80, n_long=8, long_len=250, tandem_len=100),
         dict(n_above=64, scaffolds_above=32768, large=True)),
    Case("graph_k41", _graph(75, 6000, 90, 30, 41, 600, n_short=8, short_len=120, n_long=3, long_len=300, tandem_len=60),
         dict(merged_above_32=True, differential=True)),
    # ---- windows of a random genome, velvet form: n on both sides of 64 and of 128
    Case("windows_k4_63", _velvet(4, 11, 600, gseed=101, L=900, n_cuts=60, n_extra=6, n_spelled=6, n_k1=3, n_target=63),
         dict(n_exact=63, spelled=True, has_k1=True, scaffolds_above=512, differential=True)),
    Case("windows_k5_64", _velvet(5, 12, 600, gseed=102, L=1000, n_cuts=60, n_extra=6, n_spelled=6, n_k1=3, n_target=64),
         dict(n_exact=64, spelled=True, has_k1=True, scaffolds_above=512, differential=True)),
    Case("windows_k5_65", _velvet(5, 13, 600, gseed=103, L=1000, n_cuts=62, n_extra=6, n_spelled=6, n_k1=3, n_target=65),
         dict(n_exact=65, n_above=64, spelled=True, has_k1=True, scaffolds_above=512, differential=True)),
    Case("windows_k6_128", _velvet(6, 14, 600, gseed=104, L=2200, n_cuts=120, n_extra=8, n_spelled=10, n_k1=4, n_target=128),
         dict(n_exact=128, n_above=64, spelled=True, has_k1=True, scaffolds_above=512, differential=True)),
    Case("windows_k4_129", _velvet(4, 15, 600, gseed=105, L=2000, n_cuts=124, n_extra=8, n_spelled=10, n_k1=4, n_target=129),
         dict(n_exact=129, n_above=128, spelled=True, has_k1=True, scaffolds_above=512, differential=True)),
    Case("windows_k5_172", _velvet(5, 16, 600, gseed=106, L=2600, n_cuts=150, n_extra=10, n_spelled=12, n_k1=5),
         dict(n_above=128, spelled=True, has_k1=True, scaffolds_above=512, differential=True)),
    # ---- overlaps above 32 with contigs that agree on the first window only
    Case("windows_k41_decoys", _velvet(41, 17, 400, gseed=107, L=4000, n_cuts=40, n_extra=0, n_spelled=4, n_k1=2, n_decoy=12),
         dict(merged_above_32=True, decoy_above_32=True, spelled=True, has_k1=True, differential=True)),
    # ---- the size gate of the device merge: 2 048 contigs go to the GPU, 2 049 to the host routine
    Case("gate_2048", _velvet(5, 18, 6, gseed=108, L=60000, n_cuts=2100, n_extra=8, n_spelled=8, n_k1=4, n_target=2048),
         dict(n_exact=2048, n_above=128, spelled=True, has_k1=True)),
    Case("gate_2049", _velvet(5, 18, 6, gseed=108, L=60000, n_cuts=2100, n_extra=8, n_spelled=8, n_k1=4, n_target=2049),
         dict(n_exact=2049, n_above=128, spelled=True, has_k1=True)),
    # ---- small fixed cases
    *[Case(f"spelled_fixed_seed{s}", _fixed(["ACGT", "ACGTAC", "GTAC", "TTGA"], 3, s, 20), dict(n_exact=4, spelled=True))
      for s in range(6)],
    Case("duplicate_string", _fixed(["ACGTAC", "CCGGA", "ACGTAC", "GTACCG", "TTGACG", "ACGGT"], 4, 3, 40),
         dict(n_exact=6, duplicate=True)),
    Case("one_contig", _fixed(["ACGTTGCA"], 4, 1, 10), dict(n_exact=1)),
    Case("two_apart", _fixed(["AAAAAAAC", "GGGGGGGT"], 4, 2, 10), dict(n_exact=2)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def reference(b):
    """the oracle's scaffolds of a built case"""
    if b["form"] == "graph":
        return orc.assemble_contigs(b["contigs"], b["perm"], b["k"])
    return orc.assemble_contigs_velvet(b["contigs"], b["k"], b["seed"], rows=b["rows"])
