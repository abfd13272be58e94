"""Read correction on the device (gasm_batch_correct_reads, SegmentBatch.correct_reads()) against the CPU restatement of the rule in
tests/correct_ref.py.  Every comparison is exact: every corrected read equals the restatement's string and the six counters of every
segment are equal.  References are computed once per process (correct_ref.expected, lowcov_ref.expected_cached)."""
import ctypes as C

import numpy as np
import pytest

import bubbles_ref as br
import correct_ref as cr
import genomeassembler_dev_amd as ga
import lowcov_ref as lr
from genomeassembler_dev_amd import synth
from genomeassembler_dev_amd._lib import GasmError, lib

pytestmark = pytest.mark.gpu
STATE = -7


def by_segment(flat, segs):
    out, at = [], 0
    for rs in segs:
        out.append(flat[at:at + len(rs)])
        at += len(rs)
    assert at == len(flat)
    return out


def check_correction(b, segs, k, sample=None, **build):
    """correct_reads() of the built batch `b` against the restatement under the same build options, in every (sampled) segment; returns
    (the corrected batch, {segment: the restatement's result})"""
    c = b.correct_reads()
    assert (c.n_segments, c.n_reads) == (len(segs), sum(len(rs) for rs in segs))
    got, stats = by_segment(c.read_strings(), segs), c.correction_stats()
    assert stats.shape == (len(segs), 6) and stats.dtype == np.uint32
    refs = {}
    for s in (range(len(segs)) if sample is None else sample):
        rs = segs[s]
        e = refs[s] = cr.expected(rs, k, **build)
        print(f"segment {s}: k {k} {build}: restatement {e['stats']}, device {stats[s].tolist()}")
        bad = [i for i, (x, y) in enumerate(zip(got[s], e["reads"])) if x != y]
        assert not bad, (s, bad[:5], [(rs[i], got[s][i], e["reads"][i]) for i in bad[:2]])
        assert stats[s].tolist() == e["stats"], s
    d = c.correction_stats(as_dict=True)
    assert list(d) == list(cr.FIELDS) and all(d[f].tolist() == stats[:, i].tolist() for i, f in enumerate(cr.FIELDS))
    return c, refs


@pytest.mark.parametrize("k", [21, 31, 32, 41, 63])
def test_hand_built_cases(k):
    """64-bit and 128-bit keys and the seams between them (31: all 62 bits, 32: the first 128-bit key, the candidates' XOR shifts pass 62
    and 64; 63: 126 bits): a substitution in the middle, at 0, k - 2, k - 1, at the last base and k - 1 bases from the end, two
    k + 1 apart (both fixed), two k - 1 apart (left), reads without a k-mer, a random read, a read of one k-mer, an ambiguous one"""
    segs, cases = cr.hand_cases(k)
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, min_count=2)
    c, refs = check_correction(b, segs, k, min_count=2)
    got = by_segment(c.read_strings(), segs)
    for name, s, i, want, changed, cat in cases:
        assert got[s][i] == want, name
    assert c.correction_stats().tolist() == [[2, len(segs[0]) - 12, 7, 0, 3, 8], [0, len(segs[1]) - 1, 0, 0, 1, 0]]
    c.close()
    b.close()


def test_candidate_rounds_at_k63():
    """runs of 63 k-mers: 189 candidates in three rounds of 64, the candidates' boundaries inside rounds.  Fixed by the first, second and
    third candidate (all three rounds), no candidate left after the second round (the early exit), two candidates fit (left), and
    shorter runs at both ends.  The restatement says so of every case before the device is asked"""
    seg, cases, runs = cr.candidate_round_cases()
    cr.check_candidate_round_cases(seg, cases, runs)
    b = ga.SegmentBatch.from_strings([seg])
    b.build(63, min_count=2)
    c, _ = check_correction(b, [seg], 63, min_count=2)
    got = c.read_strings()
    for name, _, i, want, changed, cat in cases:
        assert got[i] == want, name
    assert c.correction_stats().tolist() == [[0, len(seg) - len(cases), 5, 0, 2, 5]]
    c.close()
    b.close()


def test_more_than_64_kmers_per_read():
    """150-base reads at k = 21 (130 k-mers, three words of weak bits): runs that straddle k-mer starts 63 / 64 and 127 / 128, a clean
    one, and a read of exactly 128 k-mers whose run is the last bit of its last word"""
    seg, cases = cr.long_read_cases()
    b = ga.SegmentBatch.from_strings([seg])
    b.build(21, min_count=2)
    c, _ = check_correction(b, [seg], 21, min_count=2)
    got = c.read_strings()
    for name, _, i, want, changed, cat in cases:
        assert got[i] == want, name
    assert c.correction_stats().tolist() == [[0, len(seg) - 4, 4, 0, 0, 4]]
    c.close()
    b.close()


def _ragged_case():
    """windows of a backbone with lengths 23 .. 97, so that reads start and end inside 64-bit words; two neighbours that share a word
    carry an error each: the first at its last base, the second at its first"""
    rng = np.random.default_rng(12)
    G, reads = lr._backbone(rng)
    lens = [23 + (37 * i) % 75 for i in range(40)]
    rs = [G[(5 * i) % (300 - n):(5 * i) % (300 - n) + n] for i, n in enumerate(lens)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads + rs])])
    first = len(reads)
    i = next(j for j in range(first + 1, first + len(rs) - 1) if off[j + 1] % 32 not in (0, 31))      # reads j and j + 1 meet inside a word
    assert (off[i + 1] - 1) // 32 == off[i + 1] // 32 and len(rs[i - first]) >= 23 and len(rs[i + 1 - first]) >= 23
    clean = list(rs)
    rs[i - first] = cr._sub(rs[i - first], len(rs[i - first]) - 1)
    rs[i + 1 - first] = cr._sub(rs[i + 1 - first], 0)
    return reads + rs, reads + clean, (i, i + 1)


def test_shared_words_and_layouts():
    """ragged reads through from_strings and from_packed; fixed-length reads through the array form and from_packed"""
    seg, clean, (i, j) = _ragged_case()
    e = cr.expected(seg, 21, min_count=2)
    assert e["reads"] == clean and e["stats"] == [0, len(seg) - 2, 2, 0, 0, 2]
    off = np.concatenate([[0], np.cumsum([len(r) for r in seg])]).astype(np.uint64)
    flat = np.frombuffer("".join(seg).encode(), dtype=np.uint8)
    for make in (lambda: ga.SegmentBatch.from_strings([seg]),
                 lambda: ga.SegmentBatch.from_packed(synth.pack_2bit(flat), [0, len(seg)], read_off=off)):
        b = make()
        b.build(21, min_count=2)
        c, _ = check_correction(b, [seg], 21, min_count=2)
        got = c.read_strings()
        assert got[i] == clean[i] and got[j] == clean[j] and got == clean          # both fixes are there and no other base of the word changed
        data, o = c.reads()
        assert o.tolist() == off.tolist() and data.tobytes().decode() == "".join(clean)
        c.close()
        b.close()
    # fixed length: the 60-base reads of the hand-built segment
    segs, _ = cr.hand_cases(21)
    fixed = [r for r in segs[0] if len(r) == 60]
    arr = np.frombuffer("".join(fixed).encode(), dtype=np.uint8)
    for make in (lambda: ga.SegmentBatch(arr, [0, len(fixed)], fixed_len=60),
                 lambda: ga.SegmentBatch.from_packed(synth.pack_2bit(arr), [0, len(fixed)], fixed_len=60)):
        b = make()
        b.build(21, min_count=2)
        c, refs = check_correction(b, [fixed], 21, min_count=2)
        assert refs[0]["stats"][2] == 7 and c.reads()[1].tolist() == [60 * r for r in range(len(fixed) + 1)]
        c.close()
        b.close()


def test_several_segments():
    """three segments of different sizes in one batch; a read that segment 0's k-mers would repair sits in segment 1 and stays"""
    k = 15
    s0 = br.noisy_segments(600, 50, 12, 3, 1)[2][0]
    s1 = br.noisy_segments(400, 40, 15, 9, 1)[2][0]
    s2 = cr.hand_cases(k)[0][0]
    # a clean read of segment 0 (all its k-mers solid there) with one substitution in the middle: repaired in segment 0 ...
    e0 = cr.expected(s0, k, min_count=2)
    src = next(r for r in s0 if not cr.weak_runs(r, e0["trusted"], k))
    planted = cr._sub(src, 25)
    assert cr.correct(planted, e0["trusted"], k) == (src, 1, "corrected")
    segs = [s0 + [planted], s1 + [planted], s2]
    e0, e1 = cr.expected(segs[0], k, min_count=2), cr.expected(segs[1], k, min_count=2)
    # ... and in segment 1 every k-mer of it is weak: it stays as it is
    assert e0["reads"][-1] == src and e1["reads"][-1] == planted and cr.weak_runs(planted, e1["trusted"], k) == [(0, len(planted) - k)]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, min_count=2)
    c, _ = check_correction(b, segs, k, min_count=2)
    got = by_segment(c.read_strings(), segs)
    assert got[0][-1] == src and got[1][-1] == planted
    c.close()
    b.close()


# the issue's table rows 1, 2 and 4: L, read length, coverage, k, seed, strands; clean, corrected, partial, left, bases changed under
# build(k, min_count = 2) (None: not compared, the rows are the 128-bit-key cases, k = 41 and k = 63, under the simplified build only)
ROWS = [((4000, 80, 20, 21, 5, 1), (433, 419, 25, 103, 518)), ((4000, 80, 20, 21, 5, 2), (433, 419, 25, 103, 518)), ((8000, 100, 40, 41, 11, 2), None),
        ((3000, 150, 24, 63, 5, 2), None)]


@pytest.mark.parametrize("row,table", ROWS)
def test_noisy_rows(row, table):
    """the trusted set is what the README's build_simplified options leave; and, for rows 1 and 2, under build(k, min_count = 2) the
    counters are the table's"""
    L, rl, cov, k, seed, strands = row
    reads, seg_off, segs = br.noisy_segments(L, rl, cov, seed, strands)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=rl)
    opts = cr.readme_options(k)
    b.build_simplified(k, strands=strands, **opts)
    c, refs = check_correction(b, segs, k, strands=strands, **opts)
    assert refs[0]["stats"][2] > 0 and refs[0]["stats"][5] > refs[0]["stats"][2]
    c.close()
    if table is not None:
        b.build(k, min_count=2, strands=strands)
        c, refs = check_correction(b, segs, k, min_count=2, strands=strands)
        assert c.correction_stats()[0].tolist() == [0, *table]
        c.close()
    b.close()


def test_end_to_end(qtable):
    """row 1: the corrected batch, built with the README's options, gives the contigs of the restatement's corrected strings, and its
    reads score on its contigs at least as often as the uncorrected batch's on its own"""
    keys, prob = qtable
    k = 21
    reads, seg_off, segs = br.noisy_segments(4000, 80, 20, 5, 1)
    opts = cr.readme_options(k)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80)
    b.build_simplified(k, **opts).score(8, prob)
    before = int(b.scores()["kmer_breaks"].sum())
    c = b.correct_reads()
    c.build_simplified(k, **opts).score(8, prob)
    e = cr.expected(segs[0], k, **opts)
    assert c.contigs() == [lr.expected_cached(e["reads"], k, **opts)["ref"]["contigs"]]
    after = int(c.scores()["kmer_breaks"].sum())
    print(f"reads that score: {before} before correction, {after} after, of {len(segs[0])}")
    assert after >= before
    c.close()
    b.close()


def test_source_untouched_and_state_errors(qtable):
    keys, prob = qtable
    reads, seg_off, segs = br.noisy_segments(4000, 80, 20, 5, 2, n_seg=2)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80)
    h = C.c_void_p()
    assert lib().gasm_batch_correct_reads(b.h, C.byref(h)) == STATE and not h.value          # before a build
    with pytest.raises(GasmError):
        b.correct_reads()
    assert lib().gasm_batch_fetch_correct_stats(b.h, C.byref(h)) == STATE                    # not a batch correction made
    with pytest.raises(GasmError):
        b.correction_stats()
    b.build(21, min_count=2, strands=2).score(8, prob)
    snap = (b.contigs(), b.distinct()[1].tobytes(), {n: v.tobytes() for n, v in b.scores().items()})
    c = b.correct_reads()
    assert c.read_strings() != b.read_strings()
    data, off = b.reads()
    assert data.tobytes() == reads.tobytes() and off.tolist() == [80 * r for r in range(b.n_reads + 1)]
    assert (b.contigs(), b.distinct()[1].tobytes(), {n: v.tobytes() for n, v in b.scores().items()}) == snap
    with pytest.raises(GasmError):
        b.correction_stats()                                                                 # still an ordinary batch
    with pytest.raises(GasmError):
        c.correct_reads()                                                                    # the new batch has no build yet
    assert c.correction_stats()[:, :5].sum(axis=1).tolist() == [len(rs) for rs in segs]
    c.close()
    b.close()


def test_reads_round_trip():
    """reads() gives back ragged, fixed-length and packed input, before any build; and api.correct_reads is build + correct + fetch"""
    rng = np.random.default_rng(2)
    segs = [[br._rnd(rng, n) for n in (0, 1, 31, 32, 33, 64, 97)], [], [br._rnd(rng, 5)]]
    flat = [r for rs in segs for r in rs]
    b = ga.SegmentBatch.from_strings(segs)
    assert b.read_strings() == flat and b.reads()[1].tolist() == np.concatenate([[0], np.cumsum([len(r) for r in flat])]).tolist()
    b.close()
    fixed = [br._rnd(rng, 37) for _ in range(9)]
    arr = np.frombuffer("".join(fixed).encode(), dtype=np.uint8)
    for b in (ga.SegmentBatch(arr, [0, 4, 9], fixed_len=37), ga.SegmentBatch.from_packed(synth.pack_2bit(arr), [0, 4, 9], fixed_len=37)):
        assert b.read_strings() == fixed
        b.close()
    b = ga.SegmentBatch.from_strings([[], []])
    assert b.read_strings() == [] and b.reads()[1].tolist() == [0]
    b.build(21)
    c = b.correct_reads()                                             # nothing at all
    assert c.read_strings() == [] and c.correction_stats().tolist() == [[0] * 6] * 2
    c.close()
    b.close()
    seg, cases = cr.long_read_cases()
    assert ga.correct_reads(seg, 21) == cr.expected(seg, 21, min_count=2)["reads"]
