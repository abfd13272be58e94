"""Read pairs on the device (gasm_batch_place_pairs: k_pair_place; SegmentBatch.place_pairs()) against the CPU restatement of the rule in
tests/pairs_ref.py: per segment the records of every oriented pair, the insert histogram and the six counters, all with ==.  The contigs
the restatement starts from are the build's own (other tests hold them against the oracle).  Shapes: segments of at most 4 kb; mates
built so that the first k-mer in the set lies at position 0, inside the first 64-position chunk, behind it, or nowhere."""
import collections
import ctypes as C
import random

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
import links_cases as lc
import links_ref as lr
import pairs_ref as pr
from genomeassembler_dev_amd import synth
from genomeassembler_dev_amd._lib import lib

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -7
_REF = {}


def ref_place(contigs, reads, k, strands, max_insert):
    key = (tuple(contigs), tuple(reads), k, strands, max_insert)
    if key not in _REF:
        _REF[key] = pr.place(contigs, reads, k, strands, max_insert)
    return _REF[key]


def check_places(b, segs, k, strands, max_insert, sample=None):
    """every (sampled) segment's three tables against the restatement; returns (PairPlaces, {segment: the restatement's tables})"""
    pp = b.place_pairs(max_insert)
    assert (pp.k, pp.strands, pp.max_insert, pp.n_segments, pp.orientations) == (k, strands, max_insert, len(segs), strands)
    assert pp.n_pairs == sum(len(rs) for rs in segs) // 2
    contigs = b.contigs()
    out = {}
    for s in (range(len(segs)) if sample is None else sample):
        rs = segs[s]
        assert pp.contigs(s) == contigs[s]
        t = ref_place(contigs[s], rs, k, strands, max_insert)
        print(f"segment {s}: k {k} strands {strands} max_insert {max_insert}: {len(contigs[s])} contigs, {len(rs) // 2} pairs, "
              f"counters {dict(zip(pr.FIELDS, t['counters']))}")
        assert pp.records(s).tolist() == t["records"], (s, "records")
        assert pp.insert_hist(s).tolist() == t["insert_hist"], (s, "insert_hist")
        assert pp.counters(s).tolist() == t["counters"], (s, "counters")
        assert int(pp.counters(s).sum()) == len(rs) // 2 * strands
        assert int(pp.insert_hist(s).sum()) == t["counters"][3], (s, "the histogram holds the same_contig pairs")
        out[s] = t
    return pp, out


def strs(a):
    return [r.tobytes().decode() for r in a]


def example():
    g, p1, p2 = synth.plant_repeat(synth.make_segment(28, 4000, planted=False), 200, 28)
    return g.tobytes().decode(), (p1, p2), synth.simulate_pairs(g, 80, 30, 400, 30, 28, both_strands=True)


def junk(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def test_worked_example_in_two_segments():
    """the README's example beside a second genome without a repeat (fixed-length reads, both strands): the tables against the
    restatement, the twin identity through contig_twins(), and the example's numbers end to end"""
    k = 21
    genome, (p1, p2), pairs0 = example()
    g1 = synth.make_segment(29, 3000, planted=False)
    pairs1 = synth.simulate_pairs(g1, 80, 30, 400, 30, 29, both_strands=True)
    segs = [strs(pairs0), strs(pairs1)]
    assert len(segs[0]) == 2 * 668
    b = ga.SegmentBatch(np.concatenate([pairs0, pairs1]).reshape(-1), [0, len(pairs0), len(pairs0) + len(pairs1)], fixed_len=80)
    b.build(k, strands=2)
    cl = b.contig_links()
    pp, ts = check_places(b, segs, k, 2, 1024)
    for s in range(2):
        contigs, tw, rec = b.contigs(s), b.contig_twins(s).tolist(), pp.records(s).tolist()
        assert tw == pr.twin_of(contigs)
        for (c1, S, c2, E), got in zip(rec[0], rec[1]):
            assert c1 >= 0 and c2 >= 0 and got == [tw[c2], len(contigs[c2]) - E, tw[c1], len(contigs[c1]) - S]
    contigs = b.contigs(0)
    assert sorted(map(len, contigs)) == [200, 200, 653, 653, 1019, 1019, 2008, 2008]
    assert pp.counters(0, as_dict=True) == dict(skipped=0, none_placed=0, one_placed=0, same_contig=936, reversed=0, diff_contig=400)
    q = pp.insert_size(0)
    assert q == (324, 397, 475) == pr.quantiles(ts[0]["insert_hist"], 1024)
    xc, rr, yc, zc = (contigs.index(s) for s in (genome[:p1 + k - 1], genome[p1:p1 + 200], genome[p1 + 200 - (k - 1):p2 + k - 1], genome[p2 + 200 - (k - 1):]))
    rec = pp.records(0).tolist()
    _, _, M = pr.matrix(contigs, k, rec, rr)
    assert (M[(xc, yc)], M[(yc, zc)], M[(yc, yc)], M[(xc, zc)]) == (38, 25, 52, 0)
    _, _, M = pr.matrix(contigs, k, rec, rr, (q[0], q[2]))
    assert (M[(xc, yc)], M[(yc, zc)], M[(yc, yc)], M[(xc, zc)]) == (37, 24, 0, 0)
    want = sorted([genome, pr.rc(genome)])
    assert pp.resolve_repeats(0, cl) == want == pr.resolve(contigs, k, rec, 2, (q[0], q[2]))
    assert pp.resolve_repeats(0, cl, insert_range=(1, 4000)) == sorted(contigs)                       # without the filter Y -> Y blocks
    assert pp.mate_links(0) == pr.mate_links(contigs, rec, q[1])
    assert cl.span_len == 80 and cl.resolve_repeats(0) == sorted(contigs)                             # reads alone: all eight stay
    # the second genome has no repeat: one contig and its twin, nothing to resolve
    q1 = pp.insert_size(1)
    assert len(b.contigs(1)) == 2 and pp.resolve_repeats(1, cl) == pr.resolve(b.contigs(1), k, pp.records(1).tolist(), 2, (q1[0], q1[2]))
    assert pp.mate_links(1) == [] and pp.counters(1, as_dict=True)["diff_contig"] == 0
    # max_insert = 350: the overflow bin holds the rest
    small, _ = check_places(b, segs, k, 2, 350)
    h, full = small.insert_hist(0), pp.insert_hist(0)
    assert h[:350].tolist() == full[:350].tolist() and int(h[350]) == int(full[350:].sum()) > 0 and int(h.sum()) == 936
    b.close()
    assert ga.resolve_repeats_paired(segs[0], k, strands=2) == want


def noisy_pairs(genome, read_len, k, seed):
    """error-free pairs at 30x, then pairs whose mates carry substitutions placed so that the first k-mer without one starts at a
    chosen position (the errors are unique: a build with min_count = 2 drops their k-mers), and a pair of junk"""
    g = np.frombuffer(genome.encode(), dtype=np.uint8)
    rnd = random.Random(seed)
    reads = strs(synth.simulate_pairs(g, read_len, 30, 3 * read_len, 20, seed))

    def spoil(read, first):
        """substitutions at first - 1, first - 1 - k, ...: every k-mer that starts in front of `first` holds one, the one at `first` none"""
        r = list(read)
        for p in range(first - 1, -1, -k):
            r[p] = "ACGT"[("ACGT".index(r[p]) + 1 + rnd.randrange(3)) % 4]
        return "".join(r)
    n = read_len - k + 1
    firsts = []                                                     # n: no k-mer is left
    for first in (1, k, 63, 64, 65, n - 1, n):
        if first not in firsts and first <= n:
            firsts.append(first)
    seen = collections.Counter(r[i:i + k] for r in reads for i in range(n))
    covered = lambda read: all(seen[read[i:i + k]] >= 2 for i in range(n))
    for first in firsts:
        while True:                                                  # (a fragment whose ends the error-free pairs cover twice: its clean k-mers are in the set)
            s = rnd.randrange(len(genome) - 4 * read_len)
            frag = genome[s:s + 3 * read_len]
            if covered(frag[:read_len]) and covered(frag[-read_len:]):
                break
        reads += [spoil(frag[:read_len], first), pr.rc(frag[-read_len:]), frag[:read_len], spoil(pr.rc(frag[-read_len:]), first)]
    reads += [junk(rnd, read_len), junk(rnd, read_len)]
    return reads, firsts


@pytest.mark.parametrize("k,read_len,genome_len", [(31, 100, 2500), (32, 100, 2500), (33, 100, 2500), (63, 150, 3000)])
def test_128_bit_keys_and_two_chunks(k, read_len, genome_len):
    """k = 33, 100-base reads: 68 k-mers, two 64-position chunks.  Mates with substitutions hit first inside the first chunk, at its last
    position, in the second chunk, or nowhere.  The same at the key-width seams: k = 31 (the reverse complement moves down by 2 bits),
    32 (by exactly 64) and 63 (by 2 bits of a 128-bit key; 150-base reads, 88 k-mers)"""
    n = read_len - k + 1
    genome = synth.make_segment(41, genome_len, planted=False).tobytes().decode()
    reads, firsts = noisy_pairs(genome, read_len, k, 41)
    assert firsts == list(dict.fromkeys([1, k, 63, 64, 65, n - 1, n])) and n > 65 and len(firsts) >= 6
    if k == 33:
        assert firsts == [1, 33, 63, 64, 65, 67, 68]
    segs = [reads, reads[:40]]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, min_count=2)
    pp, ts = check_places(b, segs, k, 1, 600)
    c = ts[0]["counters"]
    assert c[2] >= 2 and c[1] >= 1 and c[3] > 100, c                 # one_placed (a mate spoiled to its end), none_placed (the junk)
    # the spoiled mates are placed where the clean ones are: same S resp. E
    rec, base = pp.records(0)[0].tolist(), len(reads) // 2 - 1 - 2 * len(firsts)
    where = pr.where_of(b.contigs(0), k)
    for i, first in enumerate(firsts):
        a, bb = rec[base + 2 * i], rec[base + 2 * i + 1]               # (mate 1 spoiled, mate 2 clean), (clean, spoiled)
        m1, m2 = reads[2 * (base + 2 * i)], reads[2 * (base + 2 * i + 1) + 1]
        assert [j for j in range(n) if m1[j:j + k] in where][:1] == [j for j in range(n) if pr.rc(m2[j:j + k]) in where][:1] == [first][:n - first]
        assert (a[2:] == bb[2:] and bb[:2] == a[:2]) if first < n else (a[:2] == [-1, 0] and bb[2:] == [-1, 0]), (first, a, bb)
        assert bb[0] >= 0 and a[2] >= 0
    b.build(k, min_count=2, strands=2)
    check_places(b, segs, k, 2, 600)
    b.close()


def test_hand_built_pairs_on_the_device():
    """the k = 5 pairs of tests/links_cases.py against the records, counters and histogram written out by hand: the pairs of HAND, then
    three pairs (G, G), built with min_count = 5 — every k-mer of G is then seen 6 times or more, no other k-mer (the junk, the
    reverse-complemented mates) more than 4 times, so the contigs are the hand-built four.  One row differs from the host test's: the
    "skipped" pair has 11 k-mers, far below the device's cap of 4096 (the host test sets max_kmers = 10), so it is placed as its first
    row is — [0, 0, 3, 17], diff_contig.  The added pairs' records come from the restatement"""
    copies, min_count, max_insert = 3, 5, 12
    hand = [(m1, m2, [0, 0, 3, 17] if f == "skipped" else rec, "diff_contig" if f == "skipped" else f) for m1, m2, rec, f in lc.HAND]
    assert sum(1 for h in lc.HAND if h[3] == "skipped") == 1
    added = [lc.G, lc.G] * copies
    reads = [m for m1, m2, _, _ in hand for m in (m1, m2)] + added
    b = ga.SegmentBatch.from_strings([reads])
    b.build(lc.K, min_count=min_count)
    assert b.contigs(0) == lc.CONTIGS
    pp = b.place_pairs(max_insert)
    extra = pr.place(lc.CONTIGS, added, lc.K, 1, max_insert)
    assert pp.records(0).tolist() == [[rec for _, _, rec, _ in hand] + extra["records"][0]]
    by_hand = [sum(1 for h in hand if h[3] == f) for f in pr.FIELDS]
    assert by_hand == [0, 1, 1, 2, 1, 3]
    assert pp.counters(0).tolist() == [x + y for x, y in zip(by_hand, extra["counters"])]
    hist = [0] * (max_insert + 1)
    hist[8], hist[12] = 1, 1                                          # d = 8, and d = 15 in the overflow bin of max_insert = 12
    assert pp.insert_hist(0).tolist() == [x + y for x, y in zip(hist, extra["insert_hist"])]
    b.close()


def test_a_hit_behind_the_first_chunk():
    """70 unique junk bases in front of 80 genome bases, min_count = 2: the first k-mer in the set starts at 70 — once as mate 1, once as
    mate 2"""
    k = 21
    rnd = random.Random(7)
    genome = synth.make_segment(43, 1500, planted=False).tobytes().decode()
    reads = strs(synth.simulate_pairs(np.frombuffer(genome.encode(), dtype=np.uint8), 80, 30, 300, 20, 43))
    f1, f2 = genome[200:560], genome[700:1100]
    reads += [junk(rnd, 70) + f1[:80], pr.rc(f1[-80:]), f2[:80], junk(rnd, 70) + pr.rc(f2[-80:])]
    segs = [reads]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, min_count=2, strands=2)
    pp, ts = check_places(b, segs, k, 2, 1024)
    contigs = b.contigs(0)
    fwd = [c for c, s in enumerate(contigs) if s in genome]
    assert len(contigs) == 2 and len(fwd) == 1 and len(contigs[fwd[0]]) > 1400
    c, off = fwd[0], genome.index(contigs[fwd[0]])
    rec = pp.records(0)[0].tolist()
    assert rec[-2] == [c, 200 - off - 70, c, 560 - off]               # S = o1 - i1 with i1 = 70: 70 bases in front of the fragment
    assert rec[-1] == [c, 700 - off, c, 1100 - off + 70]              # E = o2 + k + i2 with i2 = 70: 70 bases behind it
    where = pr.where_of(contigs, k)
    assert all(reads[-4][i:i + k] not in where for i in range(70)) and reads[-4][70:70 + k] in where
    assert all(pr.rc(reads[-1][i:i + k]) not in where for i in range(70)) and pr.rc(reads[-1][70:70 + k]) in where
    b.close()


def test_ragged_reads_short_long_and_outie_mates():
    """read_off: a mate shorter than k (one_placed), both shorter (none_placed), a 4200-base mate (skipped: 4180 k-mers), a mate of
    exactly 4096 k-mers (placed), an outie pair (reversed), an empty mate"""
    k = 21
    rnd = random.Random(11)
    genome = synth.make_segment(47, 1200, planted=False).tobytes().decode()
    reads = []
    for _ in range(120):
        n1, n2, d = rnd.randint(k, 120), rnd.randint(k, 120), rnd.randint(130, 400)
        s = rnd.randrange(len(genome) - d)
        reads += [genome[s:s + n1], pr.rc(genome[s + d - n2:s + d])]
    reads += [genome[i:i + 150] for i in range(0, 1200, 75)]         # (every base is covered; an even number of reads)
    s = 300
    special = [(genome[s:s + k - 1], pr.rc(genome[s + 300:s + 380])),       # mate 1 shorter than k
               (genome[s:s + 5], genome[s + 7:s + 9]),                     # both shorter
               (genome[s:s + 80] + junk(rnd, 4120), pr.rc(genome[s + 300:s + 380])),   # 4200 bases: skipped
               (genome[s:s + 80], pr.rc(genome[s + 300:s + 380] + junk(rnd, 4116 - 80))),   # 4116 bases = 4096 k-mers: placed
               (genome[s + 300:s + 380], pr.rc(genome[s:s + 80])),         # an outie
               ("", pr.rc(genome[s + 300:s + 380]))]
    reads += [m for pair in special for m in pair]
    assert len(reads) % 2 == 0
    segs = [reads, reads[:60]]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, min_count=2)                                          # (the junk k-mers are seen once: not in the set)
    pp, ts = check_places(b, segs, k, 1, 512)
    rec = pp.records(0)[0].tolist()[-len(special):]
    assert [r[0] < 0 for r in rec] == [True, True, True, False, False, True] and [r[2] < 0 for r in rec] == [False, True, True, False, False, False]
    assert rec[4][0] == rec[4][2] and rec[4][3] - rec[4][1] == -220                  # reversed: E - S = (s + 80) - (s + 300)
    c = dict(zip(pr.FIELDS, ts[0]["counters"]))
    assert c["skipped"] == 1 and c["none_placed"] == 1 and c["one_placed"] >= 2 and c["reversed"] >= 1, c
    b.close()


def test_edge_batches():
    """an empty segment, a segment whose reads are all shorter than k, and a build with no contig at all"""
    k = 21
    genome = synth.make_segment(53, 900, planted=False).tobytes().decode()
    reads = strs(synth.simulate_pairs(np.frombuffer(genome.encode(), dtype=np.uint8), 60, 20, 200, 15, 53))
    short = [genome[i:i + 12] for i in range(0, 80, 4)]
    segs = [[], reads, short, reads[:10], []]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k)
    pp, ts = check_places(b, segs, k, 1, 300)
    assert pp.records(0).shape == (1, 0, 4) and pp.counters(2).tolist() == [0, 10, 0, 0, 0, 0] and pp.records(2).tolist() == [[[-1, 0, -1, 0]] * 10]
    with pytest.raises(ValueError):
        pp.insert_size(2)
    b.build(k, min_count=1000)                                       # nothing survives: no contig at all
    assert b.contigs() == [[]] * 5
    pp, ts = check_places(b, segs, k, 1, 300)
    assert pp.counters(1).tolist() == [0, len(reads) // 2, 0, 0, 0, 0] and not pp.insert_hist(1).any()
    b.close()


def test_one_strand_places_one_orientation():
    k = 21
    _, _, pairs0 = example()
    reads = strs(pairs0)[:400]
    segs = [reads]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k)
    pp, ts = check_places(b, segs, k, 1, 1024)
    assert pp.records(0).shape == (1, 200, 4) and pp.orientations == 1
    c = dict(zip(pr.FIELDS, ts[0]["counters"]))
    # the fragments came from both strands: forward ones read as innies, the others as outies or land on other contigs
    assert c["same_contig"] > 0 and c["reversed"] + c["diff_contig"] + c["one_placed"] + c["none_placed"] > 0, c
    b.close()


def test_status_codes():
    k = 21
    genome = synth.make_segment(59, 600, planted=False).tobytes().decode()
    reads = strs(synth.simulate_pairs(np.frombuffer(genome.encode(), dtype=np.uint8), 60, 20, 200, 15, 59))
    ps, o = [C.c_void_p() for _ in range(3)], C.c_uint32()
    odd = ga.SegmentBatch.from_strings([reads[:4], reads[:3], reads[:1]])
    odd.build(k)
    assert lib().gasm_batch_place_pairs(odd.h, 300) == INVALID                            # an odd segment
    odd.close()
    b = ga.SegmentBatch.from_strings([reads])
    fetch = lambda: lib().gasm_batch_fetch_pair_places(b.h, *[C.byref(p) for p in ps], C.byref(o))
    assert lib().gasm_batch_place_pairs(b.h, 300) == STATE and fetch() == STATE           # before a build
    b.build(k)
    assert fetch() == STATE                                                               # no placement over this build
    assert lib().gasm_batch_place_pairs(b.h, 0) == INVALID and lib().gasm_batch_place_pairs(b.h, 65536) == INVALID and fetch() == STATE
    assert lib().gasm_batch_place_pairs(None, 300) == INVALID
    assert lib().gasm_batch_fetch_pair_places(b.h, None, None, None, None) == INVALID
    assert lib().gasm_batch_place_pairs(b.h, 65535) == 0 and fetch() == 0 and o.value == 1
    b.build(k, min_count=2)
    assert fetch() == STATE                                                               # a build after the placement invalidates it
    with pytest.raises(ValueError):
        b.place_pairs(70000)
    # two builds on different step slots: the placement speaks of the LAST one
    b.build(k)
    b.build(k, min_count=3, strands=2)
    check_places(b, [reads], k, 2, 300)
    assert b.place_pairs().max_insert == 1024                                             # the default: max(1024, 4 x 60)
    b.close()


def _snapshot(b):
    sc = b.scores()
    cl = b.contig_links(100)
    return (b.contigs_raw()[2], tuple(sc[key].tobytes() for key in sorted(sc)), tuple(t.tobytes() for t in b.contig_coverage()),
            tuple(t.tobytes() for t in b.contig_twins()), b.distinct()[1].tobytes(), b.score_fixed()[0].tobytes(),
            tuple(t(s).tobytes() for s in range(cl.n_segments) for t in (cl.succ, cl.pred, cl.link_support, cl.span_support)), cl.skipped.tobytes())


def test_nothing_else_moves(qtable, monkeypatch):
    """contigs, scores, coverage, twins and links before and after a placement are equal; a batch that never places launches what it
    launched before: the placement adds k_pair_place and nothing else"""
    k = 21
    monkeypatch.setenv("GASM_PINGPONG", "0")        # every launch on the batch's own context, where the profiler counts
    _, _, pairs0 = example()
    segs = [strs(pairs0)[:300], strs(pairs0)[300:500]]
    ctx = ga.Context(0)
    try:
        ctx.profile(True)
        b = ga.SegmentBatch.from_strings(segs, ctx=ctx)
        b.build(k, strands=2).score(8, qtable[1])
        before = _snapshot(b)
        first = b.place_pairs(600)
        assert _snapshot(b) == before
        again = b.place_pairs(600)
        for s in range(2):
            assert first.records(s).tolist() == again.records(s).tolist() and first.insert_hist(s).tolist() == again.insert_hist(s).tolist()
            assert first.counters(s).tolist() == again.counters(s).tolist()
        assert _snapshot(b) == before

        def launches(place):
            ctx.profile_reset()
            b.build(k, strands=2).score(8, qtable[1])
            b.scores()
            b.contig_links(100)
            if place:
                b.place_pairs(600)
            return {n: v[1] for n, v in ctx.profile_read().items() if v[1]}
        without, with_ = launches(False), launches(True)
        assert "k_pair_place" not in without and "k_read_thread" in without
        assert with_.pop("k_pair_place") == 1 and with_ == without, (with_, without)
        b.close()
    finally:
        ctx.profile(False)
