"""Read mapping on the device (gasm_batch_map_reads: k_read_map; SegmentBatch.map_reads()) against the CPU restatement of the rule in
tests/map_ref.py: per segment the records of every read, the pileup of every contig base, the mismatch histogram and the seven counters,
all with ==.  The contigs the restatement starts from are the build's own (other tests hold them against the oracle).  Shapes: segments
of at most 4 kb."""
import ctypes as C
import random

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
import bubbles_ref as br
import correct_ref as cr
import links_cases as lc
import map_ref as mr
from genomeassembler_dev_amd import synth
from genomeassembler_dev_amd._lib import lib

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -7
_REF = {}


def ref_place(contigs, reads, k, max_mismatch):
    key = (tuple(contigs), len(reads), hash(tuple(reads)), k, max_mismatch)
    if key not in _REF:
        _REF[key] = mr.place(contigs, reads, k, max_mismatch)
    return _REF[key]


def check_map(b, segs, k, max_mismatch, sample=None):
    """every (sampled) segment's four tables against the restatement; returns (ReadMap, {segment: the restatement's tables})"""
    rm = b.map_reads(max_mismatch)
    assert (rm.k, rm.max_mismatch, rm.n_segments, rm.strands) == (k, max_mismatch, len(segs), b.strands())
    contigs = b.contigs()
    out = {}
    for s in (range(len(segs)) if sample is None else sample):
        rs = segs[s]
        assert rm.contigs(s) == contigs[s]
        t = ref_place(contigs[s], rs, k, max_mismatch)
        print(f"segment {s}: k {k} max_mismatch {max_mismatch}: {len(contigs[s])} contigs, {len(rs)} reads, counters {dict(zip(mr.FIELDS, t['counters']))}, "
              f"hist {t['mismatch_hist']}")
        assert rm.counters(s).tolist() == t["counters"], (s, "counters")
        assert rm.mismatch_hist(s).tolist() == t["mismatch_hist"], (s, "mismatch_hist")
        assert rm.records(s).tolist() == t["records"], (s, "records")
        assert [p.tolist() for p in rm.pileup(s)] == t["pile"], (s, "pile")
        assert int(rm.counters(s)[:6].sum()) == len(rs)
        assert sum(int(p.sum()) for p in rm.pileup(s)) >= mr.best_totals(t["records"])[0]
        out[s] = t
    return rm, out


def test_worked_example_beside_a_second_segment():
    """the README's example beside a second noisy genome, under the simplified build: the issue's table holds for segment 0 at
    max_mismatch 0 and 4; then a strands = 2 build: folding the twins' pileups loses nothing and the folded pileups of twins mirror"""
    k = 21
    noisy, _ = cr.noisy_and_clean(4000, 80, 20, 5, 1)
    second = br.noisy_segments(3000, 80, 30, 77, 1)[2][0]
    segs = [noisy, second]
    b = ga.SegmentBatch.from_strings(segs)
    b.build_simplified(k, **cr.readme_options(k))
    assert [len(c) for c in b.contigs(0)] == [3978]
    rm, ts = check_map(b, segs, k, 0)
    assert rm.counters(0).tolist() == [0, 0, 1, 555, 424, 0, 0] and rm.mismatch_hist(0).tolist() == [424] and mr.best_totals(ts[0]["records"]) == (33907, 0)
    rm, ts = check_map(b, segs, k, 4)
    assert rm.counters(0, as_dict=True) == dict(short=0, skipped=0, unseeded=1, rejected=0, mapped_one=979, mapped_multi=0, blocks_dropped=0)
    assert rm.mismatch_hist(0).tolist() == [424, 370, 137, 35, 13] and mr.best_totals(ts[0]["records"]) == (78304, 801)
    assert rm.error_rate(0) == 801 / 78304 and rm.mapped_fraction(0) == 979 / 980
    assert rm.consensus(0) == b.contigs(0) and min(int(d.min()) for d in rm.depth(0)) == 2
    assert rm.consensus(0) == mr.consensus(b.contigs(0), ts[0]["pile"]) and rm.variants(0) == mr.variants(b.contigs(0), ts[0]["pile"])
    noisy2, _ = cr.noisy_and_clean(4000, 80, 20, 5, 2)
    segs = [noisy2, second]
    b.close()
    b = ga.SegmentBatch.from_strings(segs)
    b.build_simplified(k, strands=2, **cr.readme_options(k))
    rm, ts = check_map(b, segs, k, 4)
    assert rm.counters(0).tolist() == [0, 0, 1, 0, 979, 0, 0] and rm.mismatch_hist(0).tolist() == [424, 370, 137, 35, 13]
    for s in range(2):
        tw, own, folded = b.contig_twins(s).tolist(), rm.pileup(s), rm.pileup(s, fold_twins=True)
        assert [f.tolist() for f in folded] == mr.fold(b.contigs(s), ts[s]["pile"])
        assert sum(int(f.sum()) for f in folded) == 2 * sum(int(p.sum()) for p in own)
        for c in range(len(own)):
            assert folded[c].tolist() == folded[tw[c]][::-1, ::-1].tolist()
    b.close()


@pytest.mark.parametrize("k,read_len,genome_len", [(31, 100, 2500), (32, 100, 2500), (33, 100, 2500), (63, 150, 3000)])
def test_key_width_seams_and_two_chunks(k, read_len, genome_len):
    """68 to 88 k-mers: two 64-position chunks, at the key-width seams.  Reads spoiled so that the first seed falls at 0, 1, k, 63, 64,
    65, n - 1 and nowhere; reads with one substitution in the middle (two runs of seeds, one head); reads that run over a contig end"""
    n = read_len - k + 1
    genome = synth.make_segment(41, genome_len, planted=False).tobytes().decode()
    reads, firsts, base = mr.spoiled_reads(genome, read_len, k, 41)
    assert firsts == list(dict.fromkeys([0, 1, k, 63, 64, 65, n - 1, n])) and n > 65
    segs = [reads, reads[:40]]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, min_count=2)
    where = mr.where_of(b.contigs(0), k)
    for i, first in enumerate(firsts):
        assert [j for j in range(n) if reads[base + i][j:j + k] in where][:1] == [first][:n - first], first
    mid = reads[base + len(firsts)]
    assert len(mr.heads_of(where, mid, k)[0]) == 1 and sum(mid[j:j + k] not in where for j in range(n)) >= min(k, n // 2)
    rm, ts = check_map(b, segs, k, 0)
    rm, ts = check_map(b, segs, k, 5)
    c = dict(zip(mr.FIELDS, ts[0]["counters"]))
    assert c["unseeded"] >= 2 and c["mapped_one"] > 100, c
    # the 40 reads of segment 1 cover their genome in pieces: many contigs, and reads that run over a contig's end into the next
    assert len(b.contigs(1)) > 1 and ts[1]["counters"][5] > 0 and int(rm.counters(1)[5]) == ts[1]["counters"][5], ts[1]["counters"]
    b.close()


def test_reads_over_a_contig_end():
    """a repeat cuts the genome into contigs: reads that run from one into the next are accepted on both (mapped_multi > 0)"""
    k = 21
    g, _, _ = synth.plant_repeat(synth.make_segment(28, 3000, planted=False), 150, 28)
    reads = [r.tobytes().decode() for r in synth.simulate_reads(g, 80, 20, 28)]
    segs = [reads]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k)
    assert len(b.contigs(0)) > 2
    rm, ts = check_map(b, segs, k, 2)
    assert ts[0]["counters"][5] > 0
    b.close()


def test_hand_built_cases_on_the_device():
    """the k = 5 reads of tests/map_ref.py on the contigs of tests/links_cases.py: built with six copies of G and min_count = 5, so that
    the contigs are the hand-built four; records and counters as written out by hand, per max_mismatch"""
    copies = [lc.G] * 6
    for mm in (0, 1, 2, 4, 5):
        hand = [h for h in mr.HAND if h[1] == mm] + ([(mr.HAND_ABA["read"], mm, mr.HAND_ABA["records"][mm], None, None)] if mm in mr.HAND_ABA["records"] else [])
        reads = [h[0] for h in hand] + copies
        b = ga.SegmentBatch.from_strings([reads])
        b.build(lc.K, min_count=5)
        assert b.contigs(0) == lc.CONTIGS
        rm, ts = check_map(b, [reads], lc.K, mm)
        assert rm.records(0).tolist()[:len(hand)] == [h[2] for h in hand]
        extra = mr.place(lc.CONTIGS, copies, lc.K, mm)
        own = mr.place(lc.CONTIGS, [h[0] for h in hand], lc.K, mm)
        assert rm.counters(0).tolist() == [x + y for x, y in zip(own["counters"], extra["counters"])]
        for f in mr.FIELDS[:6]:
            assert own["counters"][mr.FIELDS.index(f)] >= sum(1 for h in hand if h[3] == f)
        b.close()


def test_hand_built_cap_and_ties_on_the_device():
    """the tables of their own of tests/map_ref.py, built from three copies of every contig with min_count = 3 (the test reads' other k-mers
    are seen at most twice): a read with nine distinct heads (blocks_dropped = 1), a best block decided by mismatches although its head
    comes second, and one decided by position; records, counters and histograms as written out by hand"""
    reads = [mr.NINE_READ] + mr.NINE * 3
    b = ga.SegmentBatch.from_strings([reads])
    b.build(5, min_count=3)
    assert b.contigs(0) == mr.NINE
    whole = mr.place(mr.NINE, mr.NINE * 3, 5, 0)                       # the copies: each on its own contig, no mismatch
    assert whole["counters"] == [0, 0, 0, 0, 27, 0, 0]
    for mm, rec, counters, hist in mr.NINE_CASES:
        rm, _ = check_map(b, [reads], 5, mm)
        assert rm.records(0).tolist()[0] == rec, mm
        assert rm.counters(0).tolist() == [x + y for x, y in zip(counters, whole["counters"])], mm
        assert rm.mismatch_hist(0).tolist() == [hist[0] + 27] + hist[1:], mm
    b.close()
    cases = list(dict.fromkeys(r for r, _, _ in mr.TIE_CASES))
    reads = cases + mr.TIE * 3
    b = ga.SegmentBatch.from_strings([reads])
    b.build(5, min_count=3)
    assert b.contigs(0) == mr.TIE
    for mm in sorted({m for _, m, _ in mr.TIE_CASES}):
        rm, _ = check_map(b, [reads], 5, mm)
        for read, m, rec in mr.TIE_CASES:
            if m == mm:
                assert rm.records(0).tolist()[cases.index(read)] == rec, (read, mm)
    b.close()


def test_ragged_reads_and_edge_batches():
    """a read shorter than k, an empty read, a read of exactly 4096 k-mers (mapped) and one of 4097 (skipped); an empty segment, a
    segment of reads all shorter than k, and min_count = 1000, which leaves no contig at all"""
    k = 21
    rnd = random.Random(11)
    genome = synth.make_segment(47, 1200, planted=False).tobytes().decode()
    junk = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    reads = [genome[i:i + 150] for i in range(0, 1051, 75)] * 2
    reads += [genome[300:320], "", junk(4116 - 80) + genome[:80], junk(4117 - 80) + genome[:80]]       # (junk in front of the contig's start: clipped)
    short = [genome[i:i + 12] for i in range(0, 80, 4)]
    segs = [[], reads, short, reads[:10], []]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, min_count=2)
    rm, ts = check_map(b, segs, k, 3)
    rec = rm.records(1).tolist()
    assert rec[-4] == mr.NO_PLACE and rec[-3] == mr.NO_PLACE and rec[-1] == mr.NO_PLACE and rec[-2] == [0, -4036, 0, 1, 80]
    assert rm.counters(1).tolist()[:2] == [2, 1]
    assert rm.records(0).shape == (0, 5) and rm.counters(2).tolist() == [len(short), 0, 0, 0, 0, 0, 0] and rm.mapped_fraction(0) == 0.0
    b.build(k, min_count=1000)
    assert b.contigs() == [[]] * 5
    rm, ts = check_map(b, segs, k, 3)
    assert rm.counters(1).tolist() == [2, 1, len(reads) - 3, 0, 0, 0, 0] and rm.pileup(1) == []
    b.close()


def test_variant_case_end_to_end():
    k = 21
    g, h, reads = mr.variant_case()
    assert len(reads) == 1166
    b = ga.SegmentBatch.from_strings([reads])
    b.build(k)
    assert sorted(map(len, b.contigs(0))).count(41) == 6 and len(b.contigs(0)) == 10
    rm, _ = check_map(b, [reads], k, 2)
    assert rm.variants(0) == []
    b.build_bubbles(k, bubble_len=41)
    assert b.contigs(0) == [g[3:]]
    rm, _ = check_map(b, [reads], k, 2)
    assert rm.counters(0, as_dict=True)["mapped_one"] == 1166
    assert rm.variants(0) == [(0, 697, "G", "T", 9, 28), (0, 1497, "A", "C", 7, 20), (0, 2297, "C", "G", 8, 36)]
    b.close()
    assert ga.map_reads(reads, k, 2, bubble_len=41).variants(0) == rm.variants(0)


def test_multi_pass_grid():
    """2051 segments of a few reads each; three of them hold enough reads for several rounds of the kernel's outer loop"""
    k = 21
    rnd = random.Random(3)
    genome = synth.make_segment(71, 600, planted=False).tobytes().decode()
    few = [genome[i:i + 60] for i in (0, 40, 80, 120)]
    big = [genome[s:s + 60] for s in (rnd.randrange(540) for _ in range(900))]
    for i in range(0, len(big), 7):
        r = list(big[i])
        r[30] = "ACGT"[("ACGT".index(r[30]) + 1) % 4]
        big[i] = "".join(r)
    segs = [few] * 2051
    heavy = (0, 1025, 2050)
    for s in heavy:
        segs[s] = big
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k)
    rm, ts = check_map(b, segs, k, 1, sample=heavy + (1, 777, 2049))
    for s in heavy:                                                   # the substitutions cut the graph into many contigs: reads meet the cap of 8 heads
        assert int(rm.counters(s)[6]) == ts[s]["counters"][6] > 0
    b.close()


def test_status_codes():
    k = 21
    genome = synth.make_segment(59, 600, planted=False).tobytes().decode()
    reads = [genome[i:i + 60] for i in range(0, 540, 10)]
    ps = [C.c_void_p() for _ in range(4)]
    b = ga.SegmentBatch.from_strings([reads])
    fetch = lambda: lib().gasm_batch_fetch_read_map(b.h, *[C.byref(p) for p in ps])
    assert lib().gasm_batch_map_reads(b.h, 4) == STATE and fetch() == STATE               # before a build
    b.build(k)
    assert fetch() == STATE                                                               # no mapping over this build
    assert lib().gasm_batch_map_reads(b.h, 256) == INVALID and fetch() == STATE
    assert lib().gasm_batch_map_reads(None, 4) == INVALID
    assert lib().gasm_batch_fetch_read_map(b.h, None, None, None, None) == INVALID
    assert lib().gasm_batch_map_reads(b.h, 255) == 0 and fetch() == 0
    b.build(k, min_count=2)
    assert fetch() == STATE                                                               # a build after the mapping invalidates it
    with pytest.raises(ValueError):
        b.map_reads(256)
    b.build(k)                                                                            # two builds on different step slots:
    b.build(k, min_count=3, strands=2)                                                    # the mapping speaks of the LAST one
    check_map(b, [reads], k, 4)
    assert b.map_reads().max_mismatch == 4
    b.close()


def _snapshot(b):
    sc = b.scores()
    cl = b.contig_links(100)
    pp = b.place_pairs(600)
    return (b.contigs_raw()[2], tuple(sc[key].tobytes() for key in sorted(sc)), tuple(t.tobytes() for t in b.contig_coverage()),
            tuple(t.tobytes() for t in b.contig_twins()), b.distinct()[1].tobytes(), b.score_fixed()[0].tobytes(),
            tuple(t(s).tobytes() for s in range(cl.n_segments) for t in (cl.succ, cl.pred, cl.link_support, cl.span_support)), cl.skipped.tobytes(),
            tuple(t(s).tobytes() for s in range(pp.n_segments) for t in (pp.records, pp.insert_hist, pp.counters)))


def test_nothing_else_moves(qtable, monkeypatch):
    """contigs, scores, coverage, twins, links and pair places before and after a mapping are equal; the mapping adds one launch of
    k_read_map and nothing else"""
    k = 21
    monkeypatch.setenv("GASM_PINGPONG", "0")        # every launch on the batch's own context, where the profiler counts
    g = synth.make_segment(28, 2000, planted=False)
    pairs0 = [r.tobytes().decode() for r in synth.simulate_pairs(g, 80, 20, 400, 30, 28, both_strands=True)]
    segs = [pairs0[:300], pairs0[300:500]]
    ctx = ga.Context(0)
    try:
        ctx.profile(True)
        b = ga.SegmentBatch.from_strings(segs, ctx=ctx)
        b.build(k, strands=2).score(8, qtable[1])
        before = _snapshot(b)
        first = b.map_reads(3)
        assert _snapshot(b) == before
        again = b.map_reads(3)
        for s in range(2):
            assert first.records(s).tolist() == again.records(s).tolist() and first.counters(s).tolist() == again.counters(s).tolist()
            assert [p.tolist() for p in first.pileup(s)] == [p.tolist() for p in again.pileup(s)]

        def launches(do_map):
            ctx.profile_reset()
            b.build(k, strands=2).score(8, qtable[1])
            b.scores()
            b.contig_links(100)
            b.contig_twins()
            if do_map:
                b.map_reads(3)
            return {n: v[1] for n, v in ctx.profile_read().items() if v[1]}
        without, with_ = launches(False), launches(True)
        assert "k_read_map" not in without and "k_read_thread" in without
        assert with_.pop("k_read_map") == 1 and with_ == without, (with_, without)
        b.close()
    finally:
        ctx.profile(False)
