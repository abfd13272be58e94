"""k_bucket_partition carries the unfinished line of every bucket from one tile of a workgroup to its next one.

A small batch has fewer tiles than the partition has workgroups, so every workgroup gets one tile and nothing is ever
carried.  GASM_DBG_PART_GRID caps the grid (read at every build): with one workgroup every tile of every segment goes
through it — a carry across every tile of a segment and the filler line at every segment change.  The expected result of
every case is an exact Python count of the reads' k-mers: the distinct k-mers of every segment in order, and how often
each occurs.  Two cases also compare contigs and kmer_breaks with the oracle."""
import collections

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
from genomeassembler_dev_amd import synth
from genomeassembler_dev_amd.api import unpack_kmers
from oracle import orc

pytestmark = pytest.mark.gpu


def _strs(a):
    return [r.tobytes().decode() for r in a]


def _segment(seed, L, rl, cov):
    return _strs(synth.simulate_reads(synth.make_segment(seed, L, planted=False), rl, cov, seed + 7919))


def _count(segs, k):
    """per segment: (distinct k-mers in order, their multiplicities)"""
    out = []
    for rs in segs:
        c = collections.Counter(r[i:i + k] for r in rs for i in range(len(r) - k + 1))
        ks = sorted(c)
        out.append((ks, [c[x] for x in ks]))
    return out


def _check_counts(b, segs, k, tag):
    want = _count(segs, k)
    seg, keys, mult, w = b.distinct()
    assert [int(seg[s + 1] - seg[s]) for s in range(len(segs))] == [len(x[0]) for x in want], (tag, "distinct k-mers per segment")
    for s in range(len(segs)):
        a, e = int(seg[s]), int(seg[s + 1])
        assert unpack_kmers(keys[a * w:e * w], k, w) == want[s][0], (tag, s, "distinct k-mers, or their order")
        assert mult[a:e].tolist() == want[s][1], (tag, s, "multiplicities")


def _built(segs, k, hint=0):
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, genome_len_hint=hint)
    return b


@pytest.fixture(scope="module")
def base():
    """3 segments of 2 kb, 100-base reads at 30x: ten tiles per segment at k = 31"""
    reads, seg_off, genomes = synth.make_batch(3, 2000, 100, 30, seed0=4100, planted=False)
    segs = [_strs(reads[int(seg_off[s]):int(seg_off[s + 1])]) for s in range(3)]
    return segs, [g.tobytes().decode() for g in genomes]


# ---- the grid: one workgroup takes every tile of every segment; two and three split them inside a segment; uncapped
@pytest.mark.parametrize("grid", [1, 2, 3, None])
def test_grid_caps(base, qtable, monkeypatch, grid):
    segs, genomes = base
    k = 31
    if grid is not None:
        monkeypatch.setenv("GASM_DBG_PART_GRID", str(grid))
    b = _built(segs, k)
    try:
        plan = b.build_plan()
        assert plan["single_pass"] == 1 and plan["distinct_attempts"] == 1, plan
        _check_counts(b, segs, k, ("grid", grid))
        if grid in (1, None):
            keys, prob = qtable
            b.score(8, prob)
            contigs, sc = b.contigs(), b.scores()
            for s, rs in enumerate(segs):
                ref = orc.get_contigs(orc.kmers_from_reads(rs, k), k, 1, rows=1)
                assert contigs[s] == ref["contigs"], (grid, s, "contigs")
                o = orc.calc_breakscore(contigs[s], rs, genomes[s], 8, keys, prob, with_lev=False, with_freq=False)
                a, e = int(sc["seg_contig_off"][s]), int(sc["seg_contig_off"][s + 1])
                assert sc["kmer_breaks"][a:e].tolist() == o["kmer_breaks"].tolist(), (grid, s, "kmer_breaks")
    finally:
        b.close()


# ---- key width and line: 16 keys of 64 bits (k = 15, 31), 8 keys of 128 bits (k = 32, 63)
@pytest.mark.parametrize("k", [15, 31, 32, 63])
@pytest.mark.parametrize("grid", [1, 2])
def test_key_widths(base, monkeypatch, k, grid):
    segs, _ = base
    monkeypatch.setenv("GASM_DBG_PART_GRID", str(grid))
    b = _built(segs, k)
    try:
        plan = b.build_plan()
        assert plan["key_words"] == (1 if k <= 31 else 2) and plan["single_pass"] == 1 and plan["distinct_attempts"] == 1, plan
        _check_counts(b, segs, k, ("k", k, grid))
    finally:
        b.close()


# ---- bucket counts
def _one_bucket_batch():
    """1024 segments and a small hint: the host adds no bucket bits -> one bucket.  Three segments hold 40 reads of 300
    bases over 800 (two tiles each at k = 15: 16 reads per tile); the others one read of 20 bases"""
    rng = np.random.default_rng(77)
    segs = [["".join("ACGT"[i] for i in rng.integers(0, 4, 20))] for _ in range(1024)]
    for n, s in enumerate((0, 500, 501)):
        segs[s] = _segment(4200 + n, 800, 300, 12)
    return segs


@pytest.mark.parametrize("case", ["nb1", "default_64", "default_128", "nb64", "nb128", "nb128_k33", "nb512", "nb512_k33"])
@pytest.mark.parametrize("grid", [1, 3])
def test_bucket_counts(monkeypatch, case, grid):
    # (segments, k, hint, bucket bits the plan must show).  Many buckets and small tiles (64 reads of 60 bases: ~2000 k-mers
    # over 64 .. 512 buckets): most tiles flush nothing for most buckets and the carry persists over several tiles
    if case == "nb1":
        segs, k, hint, bits = _one_bucket_batch(), 15, 800, 0
    elif case.startswith("default"):
        segs, k, hint, bits = [_segment(4300 + s, 1500, 60, 20) for s in range(3)], 31 if case.endswith("64") else 41, 0, None
    else:
        nseg, hint, bits = {"nb64": (16, 50_000, 6), "nb128": (8, 100_000, 7), "nb512": (3, 400_000, 9)}[case.split("_")[0]]
        segs, k = [_segment(4400 + s, 1000, 60, 12) for s in range(nseg)], 33 if case.endswith("k33") else 29
    monkeypatch.setenv("GASM_DBG_PART_GRID", str(grid))
    b = _built(segs, k, hint)
    try:
        plan = b.build_plan()
        assert plan["single_pass"] == 1 and plan["distinct_attempts"] == 1, plan
        assert bits is None or plan["bucket_bits"] == bits, plan
        _check_counts(b, segs, k, (case, grid))
    finally:
        b.close()


# ---- full tiles: 64 reads of 128 k-mers (64-bit keys) over 64 buckets leave the staging area 1024 keys for the carried keys
# and the unfinished lines, which take 960 on average: about one tile in ten has to stage on 16-byte units instead of lines
@pytest.mark.parametrize("k", [31, 33])
def test_full_tiles(monkeypatch, k):
    segs = [_segment(4600 + s, 2000, k + 127, 25) for s in range(16)]
    monkeypatch.setenv("GASM_DBG_PART_GRID", "1")
    b = _built(segs, k, 50_000)
    try:
        plan = b.build_plan()
        assert plan["single_pass"] == 1 and plan["distinct_attempts"] == 1 and plan["bucket_bits"] == 6, plan
        _check_counts(b, segs, k, ("full tiles", k))
    finally:
        b.close()


# ---- empty and thin buckets
def _thin_batch():
    rng = np.random.default_rng(5)
    g = synth.make_segment(4500, 3000, planted=False).tobytes().decode()
    ragged = [g[a:a + int(rng.integers(10, 140))] for a in rng.integers(0, 2860, 700)]      # some shorter than k
    short = [g[a:a + 20] for a in range(0, 2000, 9)]                                          # all shorter than k: no k-mer
    tandem = [("AC" * 80)[i % 2:i % 2 + 120] for i in range(300)]                              # two distinct k-mers, two buckets
    return [_segment(4501, 2000, 100, 20), short, ragged, tandem, _segment(4502, 2000, 100, 20)]


@pytest.mark.parametrize("k", [31, 45])
@pytest.mark.parametrize("grid", [1, 2])
def test_empty_and_thin_buckets(monkeypatch, k, grid):
    segs = _thin_batch()
    monkeypatch.setenv("GASM_DBG_PART_GRID", str(grid))
    # (the tandem segment's two buckets hold 16 times the mean the regions are sized from: room for them, or the build
    # comes back through the two-pass kernels and the carry's result is never looked at)
    monkeypatch.setenv("GASM_PART_SLACK", "4000")
    b = _built(segs, k)
    try:
        assert b.build_plan()["single_pass"] == 1
        _check_counts(b, segs, k, ("thin", k, grid))
        assert len(b.distinct_kmers(1)[0]) == 0 and len(b.distinct_kmers(3)[0]) == 2
    finally:
        b.close()


# ---- a region overflows while other buckets' keys are carried: the build comes back through count + scan + scatter
@pytest.mark.parametrize("k", [31, 45])
def test_region_overflow_with_pending_carry(base, monkeypatch, k):
    segs, _ = base
    monkeypatch.setenv("GASM_DBG_PART_GRID", "1")
    # ~42 000 k-mers per segment over 16 buckets; regions of 1024 keys overflow after a few tiles, the carry long pending
    monkeypatch.setenv("GASM_DBG_PART_CAP", "1024")
    b = _built(segs, k)
    try:
        plan = b.build_plan()
        assert plan["single_pass"] == 0 and plan["distinct_attempts"] == 2 and plan["multi_pass"] == 0, plan
        _check_counts(b, segs, k, ("overflow", k))
    finally:
        b.close()


# ---- step slots: consecutive builds of one batch with other k, other tile shapes
def test_consecutive_builds(base, monkeypatch):
    segs, _ = base
    monkeypatch.setenv("GASM_DBG_PART_GRID", "2")
    single = {}
    for k in (21, 31):
        b = _built(segs, k)
        try:
            _check_counts(b, segs, k, ("single", k))
            single[k] = tuple(x.tobytes() if hasattr(x, "tobytes") else x for x in b.distinct())
        finally:
            b.close()
    b = ga.SegmentBatch.from_strings(segs)
    try:
        for k in (21, 31, 21, 31):           # fetched after every build
            b.build(k)
            assert tuple(x.tobytes() if hasattr(x, "tobytes") else x for x in b.distinct()) == single[k], k
        for k in (21, 31, 21, 31):           # queued, fetched once
            b.build(k)
        assert tuple(x.tobytes() if hasattr(x, "tobytes") else x for x in b.distinct()) == single[31]
    finally:
        b.close()
