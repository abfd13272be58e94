"""The launch scheme the three read-driven kernels share (k_read_thread, k_pair_place, k_read_correct: seg_grid / seg_chunk), at a batch
shape no other test gives it: 2051 segments (257 groups of eight, the last one holding three segments and five padding workgroups per
chunk) and three segments with more reads than the grid covers at once, so that every workgroup of theirs goes round its outer loop
three times or more, the last time over a partial slice.  The big segments sit in the first group, a middle one and the padded last one.
Sampled segments are held against the restatements (tests/links_ref.py, pairs_ref.py, correct_ref.py) through the checkers of the links,
pairs and correction tests; every one of the 2051 is held against the sums its counters must make."""
import random

import numpy as np
import pytest
import torch

import correct_ref as cr
import genomeassembler_dev_amd as ga
import links_ref as lr
import pairs_ref as pr
import tips_ref as tr
from genomeassembler_dev_amd import synth
from test_correct_gpu import by_segment, check_correction
from test_links_gpu import check_links
from test_pairs_gpu import check_places

pytestmark = pytest.mark.gpu
K, S, READ_LEN, MIN_COUNT = 21, 2051, 60, 2
BIG = (3, 1029, 2050)
GROUPS = (S + 7) // 8
_MADE = {}
# Substitution rates of the big segments.  The first keeps 1 %: at this depth (3622 reads on 600 bases, about 250 on every k-mer) a given
# wrong base is then seen twice at one position in five, min_count = 2 keeps it, and the graph branches every few bases — contigs shorter
# than a read, every placed pair on two contigs.  The other two are cleaner, so that pairs lie on one contig and the insert histogram
# is written in every pass
RATES = dict(zip(BIG, (0.01, 0.0005, 0.0005)))

def grid_cap(n_cu):
    """workgroups per segment at most, as pipeline.hip takes them for S segments: n_cu * 8 / ceil(S / 8), at least one"""
    return max(1, n_cu * 8 // GROUPS)


def passes(items, per_wg, cap):
    """(workgroups per segment, rounds of a workgroup's outer loop, items of the last round) for the largest segment, by the launch rule of
    pipeline.hip: chunks = min(ceil(most / per_wg), cap), base += chunks * per_wg"""
    chunks = max(1, min(-(-items // per_wg), cap))
    return chunks, -(-items // (chunks * per_wg)), items % (chunks * per_wg)


def make_segments(cap):
    """the 2051 segments as lists of strings (made once per process).  Big: a 600-base genome (the middle one with a 40-base stretch
    planted twice), 2 * (2 * 128 * cap + 19) reads of 60 bases in pairs from both strands, substitutions at RATES, the last two pairs
    with junk mates.  Every 50th other segment is
    empty, every 51st holds two reads shorter than k, the rest one error-free pair from a 90-base genome"""
    if cap in _MADE:
        return _MADE[cap]
    n_pairs = 2 * 128 * cap + 19
    segs = []
    for s in range(S):
        if s in BIG:
            g = synth.make_segment(7000 + s, 600, planted=False)
            if s == BIG[1]:
                g, _, _ = synth.plant_repeat(g, 40, 7000 + s, min_gap=60)
            pairs = synth.simulate_pairs(g, READ_LEN, 2.2 * n_pairs * 2 * READ_LEN / 600, 200, 20, 7000 + s, both_strands=True)
            assert pairs.shape[0] >= 2 * n_pairs
            rs = tr.strs(tr.noisy(pairs[:2 * n_pairs], RATES[s], 8000 + s))
            # two pairs of the last, partial pass: both mates junk (none_placed), and mate 2 junk (one_placed where mate 1 lies on a contig)
            rnd = random.Random(9000 + s)
            junk = ["".join(rnd.choice("ACGT") for _ in range(READ_LEN)) for _ in range(3)]
            rs[-4:] = [junk[0], junk[1], rs[-2], junk[2]]
            segs.append(rs)
        elif s % 50 == 0:
            segs.append([])
        elif s % 51 == 0:
            segs.append(["ACGTACGTAC", "ACGTTGCA"])
        else:
            g = synth.make_segment(100000 + s, 90, planted=False).tobytes().decode()
            segs.append([g[:READ_LEN], pr.rc(g[-READ_LEN:])])
    _MADE[cap] = segs
    return segs


def sampled():
    """the big segments, the seams of the first and the last groups, an empty segment and one of reads shorter than k, and ten others by a
    seeded draw"""
    rnd = random.Random(2051)
    fixed = list(BIG) + [0, 7, 8, 9, 50, 51, 2047, 2048, 2049]
    return sorted(fixed + rnd.sample([s for s in range(S) if s not in fixed], 10))


@pytest.fixture(scope="module")
def shape():
    """(cap, segments) and the test's own precondition.  The restatement of the launch rule here is a PRECONDITION — it makes sure that the
    device that runs the test loops as the test means it to — not a reference: every expected value comes from the restatements of the
    rules"""
    cap = grid_cap(torch.cuda.get_device_properties(0).multi_processor_count)
    segs = make_segments(cap)
    reads = len(segs[BIG[0]])
    assert all(len(segs[s]) == reads for s in BIG) and max(map(len, segs)) == reads
    for items, per_wg in ((reads, 64), (reads // 2, 128), (reads // 2, 64)):       # reads per workgroup; pairs per workgroup, strands 1 and 2
        chunks, rounds, last = passes(items, per_wg, cap)
        assert items > 2 * cap * per_wg and chunks == cap and rounds >= 3 and 0 < last < cap * per_wg, (items, per_wg, cap)
    return cap, segs


def _beyond_first_pass(cap, per_wg, hits):
    """is an item with an index the first pass does not reach among `hits` (indices inside a segment)?"""
    return any(i >= cap * per_wg for i in hits)


def test_links_over_many_segments_and_passes(shape):
    cap, segs = shape
    b = ga.SegmentBatch.from_strings(segs)
    for strands in (1, 2):
        b.build(K, min_count=MIN_COUNT, strands=strands)
        cl, ts = check_links(b, segs, K, strands, 60, sample=sampled())
        assert cl.skipped.tolist() == [0] * S
        so = np.asarray(cl.seg_contig_off, dtype=np.int64)
        for s in range(S):
            if len(segs[s]) < 2 or len(segs[s][0]) < K:                   # empty, or nothing but reads shorter than k: all-zero tables
                assert so[s + 1] == so[s] and cl.links(s) == []
        for s in BIG:
            contigs = b.contigs(s)
            later = next((i for i in range(cap * 64, len(segs[s])) if lr.crossings(contigs, segs[s][i], K)), None)    # behind the first pass
            spans = sum(v for row in ts[s]["span_support"] for m in row for v in m)
            print(f"segment {s}, strands {strands}: {len(contigs)} contigs, {sum(map(sum, ts[s]['link_support']))} crossings, {spans} spans; read {later} crosses")
            assert sum(map(sum, ts[s]["link_support"])) >= 1 and later is not None and (spans >= 1 or s != BIG[1]), s      # (BIG[1] has the repeat)
    b.close()


def test_pairs_over_many_segments_and_passes(shape):
    cap, segs = shape
    b = ga.SegmentBatch.from_strings(segs)
    n_pairs = np.array([len(rs) // 2 for rs in segs])
    for strands in (1, 2):
        b.build(K, min_count=MIN_COUNT, strands=strands)
        pp, ts = check_places(b, segs, K, strands, 512, sample=sampled())
        assert pp.n_pairs == int(n_pairs.sum()) and pp.orientations == strands
        counters = np.stack([pp.counters(s) for s in range(S)]).astype(np.int64)
        hist = np.stack([pp.insert_hist(s) for s in range(S)]).astype(np.int64)
        assert counters.sum(axis=1).tolist() == (n_pairs * strands).tolist()
        assert hist.sum(axis=1).tolist() == counters[:, 3].tolist() and counters[:, 0].tolist() == [0] * S
        n_contigs = [len(c) for c in b.contigs()]
        rows = 0
        for s in range(S):
            rec = pp.records(s)
            rows += rec.shape[0] * rec.shape[1]
            assert rec.shape == (strands, n_pairs[s], 4)
            if rec.size:                                                   # no record names a contig the segment does not have
                assert -1 <= int(rec[:, :, [0, 2]].min()) and int(rec[:, :, [0, 2]].max()) < n_contigs[s], s
            if len(segs[s]) < 2 or len(segs[s][0]) < K:
                assert counters[s].tolist() == [0, n_pairs[s] * strands, 0, 0, 0, 0], s          # none_placed, in every orientation
        assert rows == pp.n_pairs * strands
        per_wg = 128 // strands
        for s in BIG:
            t = ts[s]
            placed = [p for p, r in enumerate(t["records"][strands - 1]) if r[0] >= 0 and r[2] >= 0]
            print(f"segment {s}, strands {strands}: counters {dict(zip(pr.FIELDS, t['counters']))}, {len(placed)} pairs placed in the last orientation")
            assert sum(1 for v in t["counters"] if v) >= 3 and _beyond_first_pass(cap, per_wg, placed), s
            same = [p for p, r in enumerate(t["records"][strands - 1]) if r[0] >= 0 and r[0] == r[2] and r[3] > r[1]]
            assert s == BIG[0] or _beyond_first_pass(cap, per_wg, same), s          # same_contig, and so a histogram bin, in a later pass
            assert t["counters"][1] >= strands and t["counters"][2] >= 1, s          # the junk pairs of the last pass
    b.close()


def test_correction_over_many_segments_and_passes(shape):
    cap, segs = shape
    b = ga.SegmentBatch.from_strings(segs)
    b.build(K, min_count=MIN_COUNT)
    c, refs = check_correction(b, segs, K, sample=sampled(), min_count=MIN_COUNT)
    stats = c.correction_stats().astype(np.int64)
    assert stats[:, :5].sum(axis=1).tolist() == [len(rs) for rs in segs]
    for s in range(S):
        if len(segs[s]) < 2 or len(segs[s][0]) < K:
            assert stats[s].tolist() == [len(segs[s]), 0, 0, 0, 0, 0], s
    got = by_segment(c.read_strings(), segs)
    for s in BIG:
        changed = [i for i, (x, y) in enumerate(zip(segs[s], refs[s]["reads"])) if x != y]
        print(f"segment {s}: restatement {dict(zip(cr.FIELDS, refs[s]['stats']))}, {len(changed)} reads changed")
        assert refs[s]["stats"][2] >= 1 and _beyond_first_pass(cap, 64, changed), s
        assert got[s][changed[-1]] == refs[s]["reads"][changed[-1]] != segs[s][changed[-1]]
    c.close()
    b.close()
