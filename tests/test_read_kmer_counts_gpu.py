"""count_read_kmers on the GPU (gasm_count_read_kmers, gasm_batch_count_read_kmers; kernels_count.hip) against the oracle's
restatement of lib/DeNovoAssembler.R:135-168 (orc.count_windows).  Counts are exact integers: every comparison is equality."""
import ctypes as C
import gzip
import itertools

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
from genomeassembler_dev_amd import _lib, qtable, readkmers, synth
from oracle import orc

pytestmark = pytest.mark.gpu
KEYS = qtable.keys()


def _strs(a):
    return [r.tobytes().decode() for r in a]


def _oracle_rows(reads):
    """the 69 904 counts of one segment: orc.count_windows of each length against the whole key list (a key of another
    length never matches, so the four calls add up to the table)"""
    out = np.zeros(qtable.ROWS, dtype=np.int64)
    for k in readkmers.KMERS:
        out += orc.count_windows(reads, k, KEYS)
    return out


def _ragged_reads(seed, n=600):
    rng = np.random.default_rng(seed)
    lens = [0, 0, 1, 2, 3, 5, 6, 7, 8, 9, 4, 10, 31, 32, 33, 64, 150] + list(rng.integers(0, 200, n))
    g = synth.make_segment(seed, 4000, planted=False).tobytes().decode()
    out = []
    for L in lens:
        a = int(rng.integers(0, len(g) - 200))
        out.append(g[a:a + int(L)])
    return out


# ------------------------------------------------------------------------------------------------ string API
@pytest.mark.parametrize("kmer", [2, 4, 6, 8])
def test_string_api_default_order_and_key_lists(kmer):
    reads = _ragged_reads(11 + kmer)
    keys = ["".join(t) for t in itertools.product("ACGT", repeat=kmer)]
    ref = orc.count_windows(reads, kmer, keys)
    got = ga.count_read_kmers(reads, kmer)
    assert got.dtype == np.uint32 and got.shape == (4 ** kmer,)
    assert got.tolist() == ref.tolist()
    # a shuffled key list with duplicates
    rng = np.random.default_rng(kmer)
    pick = [keys[i] for i in rng.integers(0, len(keys), 3 * len(keys) // 2)] + [keys[0], keys[0], keys[-1]]
    assert ga.count_read_kmers(reads, kmer, bp_kmer=pick).tolist() == orc.count_windows(reads, kmer, pick).tolist()
    # reads of exactly kmer, kmer +- 1 and shorter: one window, two windows, none
    short = ["A" * kmer, "C" * (kmer - 1), "G" * (kmer + 1), "T" * 1, ""]
    assert ga.count_read_kmers(short, kmer).tolist() == orc.count_windows(short, kmer, keys).tolist()


def test_string_api_no_reads_gives_zeros():
    for kmer in (2, 8):
        assert not ga.count_read_kmers([], kmer).any()
        assert ga.count_read_kmers([], kmer).shape == (4 ** kmer,)
    assert not ga.count_read_kmers(["", "A"], 4).any()


# ------------------------------------------------------------------------------------------------ batch API
def test_batch_fixed_length_and_ragged_with_empty_segment():
    reads, seg_off, _ = synth.make_batch(3, 5000, 100, 8, seed0=501, planted=True)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=100)
    c = b.count_read_kmers()
    assert c.shape == (3, qtable.ROWS) and c.dtype == np.uint32
    for s in range(3):
        assert c[s].tolist() == _oracle_rows(_strs(reads[int(seg_off[s]):int(seg_off[s + 1])])).tolist()
        for k in readkmers.KMERS:
            assert b.read_kmer_counts(s, k).tolist() == c[s, readkmers.table_slice(k)].tolist()
    b.close()
    segs = [_ragged_reads(3), [], ["ACGTACGTTGCA", "ACG", "", "AAAAAAAAA"], _ragged_reads(4)[:50], [""]]
    b = ga.SegmentBatch.from_strings(segs)
    c = b.count_read_kmers()
    for s, rs in enumerate(segs):
        assert c[s].tolist() == _oracle_rows(rs).tolist(), s
    b.close()


def test_batch_packed_simulated_and_fastq(tmp_path):
    segs = [_ragged_reads(21), _ragged_reads(22)[:100]]
    flat = [r for rs in segs for r in rs]
    off = np.zeros(len(flat) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in flat])
    words = synth.pack_2bit(np.frombuffer("".join(flat).encode(), dtype=np.uint8))
    seg = np.array([0, len(segs[0]), len(flat)], dtype=np.uint64)
    b = ga.SegmentBatch.from_packed(words, seg, read_off=off)
    c = b.count_read_kmers()
    for s, rs in enumerate(segs):
        assert c[s].tolist() == _oracle_rows(rs).tolist()
    b.close()
    # fixed-length packed
    reads, seg_off, _ = synth.make_batch(2, 3000, 90, 6, seed0=611)
    b = ga.SegmentBatch.from_packed(synth.pack_2bit(reads), seg_off, fixed_len=90)
    c = b.count_read_kmers()
    for s in range(2):
        assert c[s].tolist() == _oracle_rows(_strs(reads[int(seg_off[s]):int(seg_off[s + 1])])).tolist()
    b.close()
    # simulated on the device: the reads are the genomes' substrings at the starts it reports
    genomes = [synth.make_segment(70 + s, 6000, planted=True).tobytes().decode() for s in range(3)]
    b = ga.SegmentBatch.simulate(genomes, 120, 10, seed=9)
    so, st = b.read_starts()
    c = b.count_read_kmers()
    for s in range(3):
        rs = [genomes[s][int(a):int(a) + 120] for a in st[int(so[s]):int(so[s + 1])]]
        assert c[s].tolist() == _oracle_rows(rs).tolist()
    b.close()
    # FASTQ (gzip) and FASTA files, one per segment
    paths = []
    for s, rs in enumerate(segs):
        if s == 0:
            p = str(tmp_path / "s0.fq.gz")
            with gzip.open(p, "wt") as f:
                for i, r in enumerate(r for r in rs if r):
                    f.write(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n")
        else:
            p = str(tmp_path / "s1.fa")
            with open(p, "w") as f:
                for i, r in enumerate(r for r in rs if r):
                    f.write(f">r{i}\n{r}\n")
        paths.append(p)
    b = ga.SegmentBatch.from_fastq(paths)
    c = b.count_read_kmers()
    for s, rs in enumerate(segs):
        assert c[s].tolist() == _oracle_rows([r for r in rs if r]).tolist()
    b.close()


def test_second_batch_gives_identical_arrays():
    reads, seg_off, _ = synth.make_batch(7, 4000, 100, 10, seed0=901)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=100)
    one = b.count_read_kmers().copy()
    b.close()
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=100)
    two = b.count_read_kmers()
    b.close()
    assert np.array_equal(one, two)
    s = 4
    assert one[s].tolist() == _oracle_rows(_strs(reads[int(seg_off[s]):int(seg_off[s + 1])])).tolist()


@pytest.mark.parametrize("split", ["2", "4", "8"])
def test_split_knob_gives_identical_arrays(monkeypatch, split):
    segs = [_ragged_reads(31), ["A" * 150] * 200 + ["ACGGTC" * 25] * 100, [], _ragged_reads(32)[:40]]
    b = ga.SegmentBatch.from_strings(segs)
    base = b.count_read_kmers().copy()
    monkeypatch.setenv("GASM_RKC_SPLIT", split)
    assert np.array_equal(b.count_read_kmers(), base)
    b.close()
    for s, rs in enumerate(segs):
        assert base[s].tolist() == _oracle_rows(rs).tolist()


# ------------------------------------------------------------------------------------------------ skew
def test_skew_poly_a_and_tandem_reads_are_exact():
    polya = ["A" * 150] * 3000
    unit = "ACGGTC"
    g = "TTGACCA" * 30 + unit * 400 + "A" * 300 + "GATTACA" * 50 + "C" * 200 + "ACGT" * 100
    rl = 70
    tandem = [g[i:i + rl] for i in range(0, len(g) - rl + 1, 3)] + [g[500:500 + rl]] * 500
    b = ga.SegmentBatch.from_strings([polya, tandem])
    c = b.count_read_kmers()
    # one bin past 2^16 and 4e5: AAAAAAAA at 143 places per read, AA at 149
    assert int(c[0, readkmers.ROW[8]]) == 3000 * 143 > 4 * 10 ** 5
    assert int(c[0, readkmers.ROW[2]]) == 3000 * 149
    assert c[0].tolist() == _oracle_rows(polya).tolist()
    assert c[1].tolist() == _oracle_rows(tandem).tolist()
    b.close()


# ------------------------------------------------------------------------------------------------ headline shape
def test_headline_shape_configs2():
    n, L, rl, cov = 100, 50000, 150, 50
    reads, seg_off, _ = synth.make_batch(n, L, rl, cov, seed0=1234, planted=True)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=rl)
    c = b.count_read_kmers()
    nr = np.diff(seg_off.astype(np.int64))
    for k in readkmers.KMERS:
        assert c[:, readkmers.table_slice(k)].sum(axis=1, dtype=np.int64).tolist() == (nr * (rl - k + 1)).tolist()
    for s in (0, 37, 63, 99):
        assert c[s].tolist() == _oracle_rows(_strs(reads[int(seg_off[s]):int(seg_off[s + 1])])).tolist(), s
    b.close()


# ------------------------------------------------------------------------------------------------ non-interference
def _results(b):
    seg, keys, mult, _ = b.distinct()
    sc = b.scores()
    return b.contigs_raw(), (seg, keys, mult), sc


def _same(x, y):
    (a1, a2, a3), (d1, d2, d3), s1 = x
    (b1, b2, b3), (e1, e2, e3), s2 = y
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2) and a3 == b3
    assert np.array_equal(d1, e1) and np.array_equal(d2, e2) and np.array_equal(d3, e3)
    for key in s1:
        assert np.array_equal(s1[key], s2[key]), key


def test_counting_does_not_disturb_build_and_score():
    reads, seg_off, _ = synth.make_batch(4, 8000, 100, 20, seed0=321, planted=True)
    flat = reads.reshape(-1)
    tab = qtable.load_normalised()
    b = ga.SegmentBatch(flat, seg_off, fixed_len=100)
    b.build(31).score(8, tab)
    ref = _results(b)
    b.close()
    b = ga.SegmentBatch(flat, seg_off, fixed_len=100)
    before = b.count_read_kmers().copy()                      # before any build
    b.build(31)
    mid = b.count_read_kmers().copy()                         # between a build and its score
    b.score(8, tab)
    _same(ref, _results(b))
    assert np.array_equal(before, mid)
    assert np.array_equal(b.count_read_kmers(), before)       # after both, and a second time
    # queued while two step-slot builds are in flight (no fetch in between)
    b.build(31).score(8, tab)
    b.build(31).score(8, tab)
    assert np.array_equal(b.count_read_kmers(), before)
    _same(ref, _results(b))
    b.close()
    for s in range(4):
        assert before[s].tolist() == _oracle_rows(_strs(reads[int(seg_off[s]):int(seg_off[s + 1])])).tolist()


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    with pytest.raises(ga.GasmError) as e:
        ga.count_read_kmers(["ACGT"], 5)
    assert e.value.status == -1
    with pytest.raises(ga.GasmError) as e:
        ga.count_read_kmers(["ACGTACGT"], 4, bp_kmer=["ACGT", "ACG"])
    assert e.value.status == -1
    with pytest.raises(ga.GasmError) as e:
        ga.count_read_kmers(["ACGTACGT"], 4, bp_kmer=["ACGT", "ACGN"])
    assert e.value.status == -2
    with pytest.raises(ga.GasmError) as e:
        ga.count_read_kmers(["ACGTNACGT"], 2)
    assert e.value.status == -2
    b = ga.SegmentBatch.from_strings([["ACGTACGT"]])
    p = C.c_void_p()
    assert _lib.lib().gasm_batch_fetch_read_kmer_counts(b.h, C.byref(p)) == -7
    b.count_read_kmers()
    assert _lib.lib().gasm_batch_fetch_read_kmer_counts(b.h, C.byref(p)) == 0
    b.close()
