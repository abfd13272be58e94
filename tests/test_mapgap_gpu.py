"""Gapped read mapping on the device (gasm_batch_map_reads_gapped: k_read_map_gapped; SegmentBatch.map_reads_gapped()) against the CPU
restatement of the rule in tests/mapgap_ref.py: per segment the records and gap records of every read, the pileup and the gap pileup of
every contig base, the edit histogram and the eight counters, all with ==.  The contigs the restatement starts from are the build's own.
Shapes: segments of at most 4 kb."""
import ctypes as C
import random

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
import correct_ref as cr
import map_ref as mr
import mapgap_ref as gr
from genomeassembler_dev_amd import synth
from genomeassembler_dev_amd._lib import lib

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -7
_REF = {}


def ref_place(contigs, reads, k, max_edits, max_gap):
    key = (tuple(contigs), len(reads), hash(tuple(reads)), k, max_edits, max_gap)
    if key not in _REF:
        _REF[key] = gr.place_gapped(contigs, reads, k, max_edits, max_gap)
    return _REF[key]


def tables(rm, s):
    return dict(records=rm.records(s).tolist(), gap_records=rm.gap_records(s).tolist(), pile=[p.tolist() for p in rm.pileup(s)],
                gap_pile=[p.tolist() for p in rm.gap_pileup(s)], edit_hist=rm.edit_hist(s).tolist(), counters=rm.counters(s).tolist())


def check_gapped(b, segs, k, max_edits, max_gap, sample=None):
    """every (sampled) segment's six tables against the restatement; returns (GappedReadMap, {segment: the restatement's tables})"""
    rm = b.map_reads_gapped(max_edits, max_gap)
    assert (rm.k, rm.max_edits, rm.max_gap, rm.n_segments, rm.strands) == (k, max_edits, max_gap, len(segs), b.strands())
    contigs = b.contigs()
    out = {}
    for s in (range(len(segs)) if sample is None else sample):
        t = ref_place(contigs[s], segs[s], k, max_edits, max_gap)
        got = tables(rm, s)
        print(f"segment {s}: k {k} max_edits {max_edits} max_gap {max_gap}: {len(contigs[s])} contigs, {len(segs[s])} reads, "
              f"counters {dict(zip(gr.FIELDS, t['counters']))}, hist {t['edit_hist']}")
        for name in ("counters", "edit_hist", "records", "gap_records", "pile", "gap_pile"):
            assert got[name] == t[name], (s, name)
        assert sum(int(p[:, 0].sum()) for p in rm.gap_pileup(s)) >= sum(g[2] for g in t["gap_records"])     # (the best chains' deleted bases)
        out[s] = t
    return rm, out


def gap_zero_batches(k, read_len, genome_len):
    """(segments, min_count, the max_edits to try): spoiled reads of a random genome, or (read_len = 0) the two hand-built batches of
    test_map_gpu.test_hand_built_cap_and_ties_on_the_device — a read with more than MAP_MAX_BLOCKS heads, ties between blocks — where
    the two forms of the kernel could disagree without random reads showing it"""
    if read_len:
        genome = synth.make_segment(41, genome_len, planted=False).tobytes().decode()
        reads, _, _ = mr.spoiled_reads(genome, read_len, k, 41)
        return [([reads, reads[:40]], 2, (0, 5))]
    return [([[mr.NINE_READ] + mr.NINE * 3], 3, sorted({c[0] for c in mr.NINE_CASES})),
            ([list(dict.fromkeys(r for r, _, _ in mr.TIE_CASES)) + mr.TIE * 3], 3, sorted({m for _, m, _ in mr.TIE_CASES}))]


@pytest.mark.parametrize("k,read_len,genome_len", [(31, 100, 2500), (32, 100, 2500), (33, 100, 2500), (63, 150, 3000),
                                                   pytest.param(5, 0, 0, id="hand-built-cap-and-ties")])
def test_max_gap_zero_is_map_reads(k, read_len, genome_len):
    dropped = [gap_zero_is_map_reads(segs, k, min_count, edits) for segs, min_count, edits in gap_zero_batches(k, read_len, genome_len)]
    assert read_len or dropped[0] >= 1                                  # (the hand-built batch does go past the cap of heads)


def gap_zero_is_map_reads(segs, k, min_count, edits):
    """both entries' tables agree; returns the most blocks_dropped any max_edits gave"""
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, min_count=min_count)
    dropped = 0
    for me in edits:
        plain = b.map_reads(me)
        dropped = max(dropped, sum(int(plain.counters(s)[6]) for s in range(len(segs))))
        rm, _ = check_gapped(b, segs, k, me, 0)
        for s in range(len(segs)):
            assert rm.records(s).tolist() == plain.records(s).tolist() and rm.edit_hist(s).tolist() == plain.mismatch_hist(s).tolist()
            assert [p.tolist() for p in rm.pileup(s)] == [p.tolist() for p in plain.pileup(s)]
            assert rm.counters(s).tolist() == plain.counters(s).tolist() + [0]
            g = rm.gap_records(s)
            placed = rm.records(s)[:, 0] >= 0
            assert g[placed, 0].tolist() == [1] * int(placed.sum()) and not g[:, 1:3].any() and not g[~placed].any()
            assert g[placed, 3].tolist() == rm.records(s)[placed, 1].tolist()
            assert not any(p.any() for p in rm.gap_pileup(s))
    b.close()
    return dropped


def test_hand_built_cases_on_the_device():
    """the cases of tests/mapgap_ref.py: the table is built from three copies of every contig with min_count = 3; records, gap records
    and counters as written out by hand, per (max_edits, max_gap)"""
    for k, table in ((5, gr.PQ), (6, [gr.R5])):
        for me, mg in sorted({(h[3], h[4]) for h in gr.HAND if h[0] == k}):
            hand = [h for h in gr.HAND if h[0] == k and (h[3], h[4]) == (me, mg)]
            copies = table * 3
            reads = [h[2] for h in hand] + copies
            b = ga.SegmentBatch.from_strings([reads])
            b.build(k, min_count=3)
            assert b.contigs(0) == table
            rm, ts = check_gapped(b, [reads], k, me, mg)
            assert rm.records(0).tolist()[:len(hand)] == [h[5] for h in hand] and rm.gap_records(0).tolist()[:len(hand)] == [h[6] for h in hand]
            own, extra = gr.place_gapped(table, [h[2] for h in hand], k, me, mg), gr.place_gapped(table, copies, k, me, mg)
            assert rm.counters(0).tolist() == [x + y for x, y in zip(own["counters"], extra["counters"])]
            assert extra["counters"][4] == len(copies) and own["counters"][7] == sum(1 for h in hand if h[6][0] >= 2)
            b.close()


@pytest.mark.parametrize("k", [21, 33])
def test_seams(k):
    """150-base reads with one planted indel each: breakpoints at read positions 22, 63, 64, 65 and 128, gaps of 1, 2 and max_gap bases, as
    insertions and as deletions.  A variant is planted where it leaves a seed on both sides: at >= k in front, and k bases behind the
    gap, 150 - at - inserted bases >= k.  That leaves out: for k = 21 the insertions of 2 and 3 bases at 128 (20 and 19 bases behind
    them; the deletions and the insertion of one base at 128 stay, their second head at J = 127 .. 129, the third chunk); for k = 33
    position 22 (no k-mer in front) and position 128 (22 bases behind).  Then a read with two deletions 40 bases apart (three heads), and
    a read whose first head is at 0 and whose second lies beyond position 64 (substitutions every k - 1 bases in between leave no
    seed: the window spans two chunks); beside error-free reads at 30x"""
    max_gap, rl = 3, 150
    rnd = random.Random(k)
    g = synth.make_segment(90 + k, 3000, planted=False)
    genome = g.tobytes().decode()
    clean = [r.tobytes().decode() for r in synth.simulate_reads(g, rl, 30, 7)]
    planted = []
    variants = [(at, sign * gap) for at in (22, 63, 64, 65, 128) for gap in (1, 2, max_gap) for sign in (1, -1)
                if at >= k and rl - at - (gap if sign < 0 else 0) >= k]
    assert [v for v in variants if v[0] == 128] == ([(128, 1), (128, -1), (128, 2), (128, 3)] if k == 21 else [])
    for at, g_ in variants:
        planted.append(gr.planted_indel_read(genome, rnd.randrange(200, 2500), rl, at, g_, rnd))
    s0 = 1000
    planted.append((genome[s0:s0 + 50] + genome[s0 + 51:s0 + 91] + genome[s0 + 93:])[:rl])     # a deletion at 50, one of two bases 40 further on
    wide = list(gr.planted_indel_read(genome, 1500, rl, 100, 2, rnd))
    for p in range(k + 2, 100 - k, k - 1):
        wide[p] = "ACGT"[("ACGT".index(wide[p]) + 1) % 4]
    planted.append("".join(wide))
    reads = planted + clean
    b = ga.SegmentBatch.from_strings([reads])
    b.build(k, min_count=2)
    assert [len(c) > 2900 for c in b.contigs(0)] == [True]
    rm, ts = check_gapped(b, [reads], k, 8, max_gap)
    gaps = ts[0]["gap_records"][:len(planted)]
    assert [(q, i, d) for q, i, d, _ in gaps[:-2]] == [(2, max(0, -g_), max(0, g_)) for _, g_ in variants], gaps
    where = mr.where_of(b.contigs(0), k)
    second = []
    for r, (at, g_) in zip(planted, variants):                        # the second head starts at the gap (a few positions earlier where the
        h = mr.heads_of(where, r, k)[0]                               # bases at the gap repeat), for 128 in the third chunk
        assert len(h) == 2 and at - max_gap - 1 <= h[1][0] <= at + max_gap, (at, g_, h)
        second.append(h[1][0])
    assert k != 21 or sum(1 for J in second if J >= 128) >= 2, second
    assert gaps[-2][:3] == [3, 0, 3] and gaps[-1][:3] == [2, 0, 2], gaps[-2:]
    heads = mr.heads_of(where, planted[-1], k)[0]
    assert heads[0][0] == 0 and heads[1][0] > 64 + heads[0][0], heads
    b.close()


def test_worked_example_beside_a_second_segment():
    """synth.simulate_reads_indel on a 4 kb genome: 80 bases, 20x, 1 % substitutions, 0.3 % indels, k = 21, under the simplified build,
    beside a second segment; then a strands = 2 build"""
    k = 21
    genome, reads = gr.indel_reads(4000, 80, 20, 5)
    own = {mg: gr.place_gapped([genome], reads, k, 6, mg) for mg in (3, 0)}         # first on the CPU, the genome as its own contig
    assert own[3]["counters"][7] > 0 and gr.placed(own[3]) > gr.placed(own[0])
    _, second = gr.indel_reads(3000, 80, 30, 77)
    segs = [reads, second]
    for strands in (1, 2):
        b = ga.SegmentBatch.from_strings(segs)
        b.build_simplified(k, strands=strands, **cr.readme_options(k))
        rm, ts = check_gapped(b, segs, k, 6, 3)
        _, t0 = check_gapped(b, segs, k, 6, 0)
        assert ts[0]["counters"][7] > 0 and gr.placed(ts[0]) > gr.placed(t0[0])
        for s in range(2):
            assert [d.tolist() for d in rm.depth(s)] == gr.depth(ts[s]["pile"], ts[s]["gap_pile"])
            assert rm.indels(s) == gr.indels(ts[s]["pile"], ts[s]["gap_pile"]) and rm.error_rate(s) == gr.error_rate(ts[s]["records"], ts[s]["gap_records"])
            assert rm.consensus(s) == gr.consensus(b.contigs(s), ts[s]["pile"], ts[s]["gap_pile"])
            if strands == 2:
                tw, folded, gf = b.contig_twins(s).tolist(), rm.pileup(s, fold_twins=True), rm.gap_pileup(s, fold_twins=True)
                assert [f.tolist() for f in folded] == mr.fold(b.contigs(s), ts[s]["pile"])
                assert [f.tolist() for f in gf] == gr.fold_gaps(b.contigs(s), ts[s]["gap_pile"])
                for c in range(len(folded)):
                    assert folded[c].tolist() == folded[tw[c]][::-1, ::-1].tolist() and gf[c][:, 0].tolist() == gf[tw[c]][::-1, 0].tolist()
        b.close()


def test_an_indel_variant_comes_back():
    """24x reads of a 3 kb genome plus 8x reads of a copy with one base deleted and one inserted, 800 bases apart.  Build options:
    bubble_len = 41 (k = 21) pops both indel bubbles and leaves one contig, the genome without its first three bases (tried with the
    CPU restatement of the simplifications: tests/test_mapgap_host.py).  The variant is in a quarter of the reads, and about half of
    the 80-base reads with an indel stay unplaced because it lies within k of an end (include/gasm.h, LIMITS): a site is expected at
    about an eighth of the depth, so the list is taken at min_frac = 0.1"""
    k = 21
    g, reads, sites = gr.indel_variant_case()
    b = ga.SegmentBatch.from_strings([reads])
    b.build_bubbles(k, bubble_len=41)
    assert b.contigs(0) == [g[3:]]
    rm, ts = check_gapped(b, [reads], k, 6, 3)
    got = rm.indels(0, min_depth=8, min_frac=0.1)
    assert got == gr.indels(ts[0]["pile"], ts[0]["gap_pile"], 8, 0.1) and [x[:3] for x in got] == sites, got
    assert rm.indels(0) == gr.indels(ts[0]["pile"], ts[0]["gap_pile"])
    b.close()


def test_a_grid_that_loops():
    """one segment of more than 8192 reads beside 600 segments of 20 reads, max_gap = 2: a sample of segments in full, every segment's
    counters"""
    k = 21
    rnd = random.Random(3)
    genome = synth.make_segment(71, 700, planted=False).tobytes().decode()
    few = [genome[i:i + 60] for i in range(0, 176, 35)] * 3 + [gr.planted_indel_read(genome, 20, 60, 30, 1, rnd), gr.planted_indel_read(genome, 60, 60, 30, -1, rnd)]
    big = [genome[s:s + 60] for s in (rnd.randrange(640) for _ in range(8300))]
    for i in range(0, len(big), 50):                                 # (rare enough that no planted indel is seen three times and gets into the build)
        big[i] = gr.planted_indel_read(genome, rnd.randrange(560), 60, 25 + i % 9, (1, -1, 2, -2, 3)[(i // 50) % 5], rnd)
    assert len(few) == 20 and len(big) > 8192
    segs = [few] * 601
    segs[300] = big
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, min_count=3)
    sample = (0, 1, 299, 300, 301, 450, 599, 600)
    rm, ts = check_gapped(b, segs, k, 4, 2, sample=sample)
    assert ts[300]["counters"][7] > 0 and ts[0]["counters"][7] == 2
    for s in range(601):
        assert rm.counters(s).tolist() == ts[300 if s == 300 else 0]["counters"], s
    b.close()


def test_independence_repeatability_and_status_codes():
    k = 21
    genome, reads = gr.indel_reads(1500, 80, 20, 9)
    b = ga.SegmentBatch.from_strings([reads])
    ps, qs = [C.c_void_p() for _ in range(6)], [C.c_void_p() for _ in range(4)]
    fetch = lambda: lib().gasm_batch_fetch_read_map_gapped(b.h, *[C.byref(p) for p in ps])
    fetch_plain = lambda: lib().gasm_batch_fetch_read_map(b.h, *[C.byref(p) for p in qs])
    assert lib().gasm_batch_map_reads_gapped(b.h, 6, 3) == STATE and fetch() == STATE             # before a build
    b.build(k, min_count=2)
    assert fetch() == STATE                                                                       # no gapped mapping over this build
    assert lib().gasm_batch_map_reads_gapped(b.h, 6, 17) == INVALID and lib().gasm_batch_map_reads_gapped(b.h, 256, 3) == INVALID and fetch() == STATE
    assert lib().gasm_batch_map_reads_gapped(None, 6, 3) == INVALID
    assert lib().gasm_batch_fetch_read_map_gapped(b.h, None, None, None, None, None, None) == INVALID
    for bad in ((256, 3), (6, 17), (-1, 3), (6, -1)):
        with pytest.raises(ValueError):
            b.map_reads_gapped(*bad)
    alone_plain, alone = b.map_reads(6), b.map_reads_gapped(6, 3)
    b.build(k, min_count=2)
    assert fetch() == STATE and fetch_plain() == STATE                                            # a new build invalidates both
    assert lib().gasm_batch_map_reads(b.h, 6) == 0 and lib().gasm_batch_map_reads_gapped(b.h, 6, 3) == 0 and fetch_plain() == 0 and fetch() == 0
    n = len(reads)
    assert np.ctypeslib.as_array(C.cast(qs[0], C.POINTER(C.c_int32)), shape=(4 * n,)).reshape(-1, 4)[:, [0, 1, 3]].tolist() == alone_plain.records(0)[:, [0, 1, 4]].tolist()
    assert np.ctypeslib.as_array(C.cast(ps[0], C.POINTER(C.c_int32)), shape=(4 * n,)).reshape(-1, 4)[:, [0, 1, 3]].tolist() == alone.records(0)[:, [0, 1, 4]].tolist()
    assert np.ctypeslib.as_array(C.cast(ps[1], C.POINTER(C.c_int32)), shape=(4 * n,)).reshape(-1, 4).tolist() == alone.gap_records(0).tolist()
    again = b.map_reads_gapped(6, 3)
    assert tables(again, 0) == tables(alone, 0) and tables(alone, 0) == ref_place(b.contigs(0), reads, k, 6, 3)
    assert b.map_reads(6).records(0).tolist() == alone_plain.records(0).tolist()
    assert b.map_reads_gapped().max_edits == 6 and b.map_reads_gapped().max_gap == 3
    b.close()
    assert tables(ga.map_reads_gapped(reads, k, 6, 3, min_count=2), 0) == tables(alone, 0)         # (build_simplified with min_count = 2 alone is that build)


def test_launch_census(qtable, monkeypatch):
    """the pass adds exactly one launch of k_read_map_gapped and nothing else; a batch that never asks launches what it did"""
    k = 21
    monkeypatch.setenv("GASM_PINGPONG", "0")        # every launch on the batch's own context, where the profiler counts
    _, reads = gr.indel_reads(2000, 80, 20, 28)
    segs = [reads[:300], reads[300:]]
    ctx = ga.Context(0)
    try:
        ctx.profile(True)
        b = ga.SegmentBatch.from_strings(segs, ctx=ctx)
        b.build(k, strands=2)                           # (the both-strand stream is made once per batch: before the counting starts)

        def launches(do_gapped):
            ctx.profile_reset()
            b.build(k, strands=2).score(8, qtable[1])
            b.scores()
            b.contig_links(100)
            b.map_reads(3)
            if do_gapped:
                b.map_reads_gapped(6, 3)
            return {n: v[1] for n, v in ctx.profile_read().items() if v[1]}
        without, with_ = launches(False), launches(True)
        assert "k_read_map_gapped" not in without and without["k_read_map"] == 1
        assert with_.pop("k_read_map_gapped") == 1 and with_ == without, (with_, without)
        b.close()
    finally:
        ctx.profile(False)
