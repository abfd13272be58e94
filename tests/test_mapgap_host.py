"""Gapped read mapping without a GPU: include/gasm.h declares the entries and states the rule, libgasm.so exports them, the ctypes mirror
and the Python surface know them; the CPU restatement of the rule (tests/mapgap_ref.py) gives on the hand-built cases the records,
counters and pileup adds written out by hand, its breakpoints are the joint optimum (brute force) and its cost is never below the
semi-global edit distance; readmap.GappedReadMap's host arithmetic agrees with its restatement.  The checks on the restatement itself
(hand cases, brute force, one indel) take their reads from synth.simulate_reads_indel or pass their tables through GappedReadMap as
well, so each of them needs the package's new surface.  The one-pass breakpoint (mapgap_ref.breakpoint_linear) is held equal to the
definition, and the cases of tests/test_mapgap_edges_gpu.py (long reads, the ragged batch, ties, contig ends, the slot steps) have their
preconditions asserted here, with the genome or the CPU restatement of the build in place of the device's contigs."""
import ctypes as C
import inspect
import itertools
import os
import random
import re

import numpy as np
import pytest

import lowcov_ref as lr
import map_ref as mr
import mapgap_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeassembler_dev_amd", "libgasm.so")
HEADER = os.path.join(ROOT, "include", "gasm.h")
SIGNATURES = {
    "gasm_batch_map_reads_gapped": "int gasm_batch_map_reads_gapped(gasm_batch* b, uint32_t max_edits, uint32_t max_gap);",
    "gasm_batch_fetch_read_map_gapped": "int gasm_batch_fetch_read_map_gapped(gasm_batch* b, const int32_t** rec, const int32_t** rec_gap, const uint32_t** pile, "
                                        "const uint32_t** gap_pile, const uint32_t** edit_hist, const uint64_t** counters);",
}


def _flat(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text).replace("( ", "(").replace(" )", ")")


def test_header_declares_the_entries_and_the_rule():
    with open(HEADER) as f:
        raw = f.read()
    flat = _flat(raw)
    for name, sig in SIGNATURES.items():
        assert _flat(sig) in flat, name
    for d in ("#define GASM_MAP_MAX_MISMATCH 255", "#define GASM_MAP_MAX_GAP 16", "#define GASM_MAPG_FIELDS 8"):
        assert d in raw, d
    words = " ".join(re.sub(r"(?m)^ \* ?", " ", raw).split())
    for phrase in ("Gapped read mapping", "0 < |g| <= max_gap", "The window of t is [J_i + 1, J_{i+1} - G]", "A chain is ACCEPTED iff cost <= max_edits",
                   "largest overlap, then lowest cost, then smallest J_1", "Only consecutive kept heads join", "The sequence of inserted bases is not recorded"):
        assert phrase in words, phrase


def test_library_exports_the_entries():
    lib = C.CDLL(LIB)                                                # (symbol table only: nothing here calls into the library)
    for name in SIGNATURES:
        assert hasattr(lib, name), name


def test_ctypes_mirror_and_python_surface():
    from genomeassembler_dev_amd import _lib, api, batch, readmap, synth
    import genomeassembler_dev_amd as ga
    i, vp, pp, u32 = C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32
    want = {"gasm_batch_map_reads_gapped": (i, [vp, u32, u32]), "gasm_batch_fetch_read_map_gapped": (i, [vp, pp, pp, pp, pp, pp, pp])}
    for name, (res, args) in want.items():
        assert _lib.SYMBOLS[name][0] is res and list(_lib.SYMBOLS[name][1]) == args, name
    assert tuple(_lib.MAPG_FIELDS) == gr.FIELDS and len(_lib.MAPG_FIELDS) == 8 and _lib.MAP_MAX_GAP == gr.MAX_GAP == 16
    q = inspect.signature(batch.SegmentBatch.map_reads_gapped).parameters
    assert (q["max_edits"].default, q["max_gap"].default) == (6, 3)
    q = inspect.signature(api.map_reads_gapped).parameters
    assert list(q)[:4] == ["reads", "k", "max_edits", "max_gap"] and (q["max_edits"].default, q["max_gap"].default) == (6, 3)
    assert ga.GappedReadMap is readmap.GappedReadMap and ga.map_reads_gapped is api.map_reads_gapped and issubclass(readmap.GappedReadMap, readmap.ReadMap)
    for name in ("gap_records", "gap_pileup", "depth", "error_rate", "indels", "consensus"):
        assert callable(getattr(readmap.GappedReadMap, name)), name
    q = inspect.signature(readmap.GappedReadMap.indels).parameters
    assert (q["min_depth"].default, q["min_frac"].default) == (8, 0.2) and inspect.signature(readmap.GappedReadMap.consensus).parameters["min_depth"].default == 3
    assert list(inspect.signature(synth.simulate_reads_indel).parameters) == ["genome", "read_len", "coverage", "seed", "sub_rate", "indel_rate"]
    b = batch.SegmentBatch.__new__(batch.SegmentBatch)               # (no library call is reached: the check comes first)
    b.h = None
    for bad in ((-1, 3), (256, 3), (6, -1), (6, 17)):
        with pytest.raises(ValueError):
            b.map_reads_gapped(*bad)


def test_hand_built_cases():
    for case in gr.HAND:
        k, contigs, read, me, mg, rec, gap, field = case[:8]
        t = gr.place_gapped(contigs, [read], k, me, mg)
        assert t["records"] == [rec] and t["gap_records"] == [gap], read
        assert t["counters"] == [1 if f == field else 0 for f in mr.FIELDS] + [1 if gap[0] >= 2 else 0], read
        assert gr.table_adds(t) == gr.hand_adds(case), read
        assert sum(t["edit_hist"]) == rec[3] and (rec[0] < 0 or t["edit_hist"][rec[2]] == 1)
        rm = _gapped(contigs, t, k, me, mg)                           # and what the package's class makes of the hand-written tables
        assert rm.records(0).tolist() == [rec] and rm.gap_records(0).tolist() == [gap] and rm.counters(0, as_dict=True)["gapped"] == (gap[0] >= 2)
        assert sorted((c, p, kind) for c, p, kind, _, _ in rm.indels(0, min_depth=1, min_frac=0.0)) == gr.hand_adds(case)[1]
        if read in gr.HAND_HEADS:
            assert mr.heads_of(mr.where_of(contigs, k), read, k)[0] == gr.HAND_HEADS[read]
    for k, table in ((5, gr.PQ), (6, [gr.R5])):                       # what a build from three copies of each gives: the table itself
        assert lr.expected_cached(table * 3, k, min_count=3)["ref"]["contigs"] == table


def test_max_gap_zero_is_the_ungapped_rule():
    genome, reads = gr.indel_reads(2000, 80, 10, 3)
    a, b = gr.place_gapped([genome], reads, 21, 4, 0), mr.place([genome], reads, 21, 4)
    assert (a["records"], a["pile"], a["edit_hist"], a["counters"][:7]) == (b["records"], b["pile"], b["mismatch_hist"], b["counters"])
    assert a["counters"][7] == 0 and not any(g != [0, 0] for gp in a["gap_pile"] for g in gp)
    assert all(g == ([1, 0, 0, r[1]] if r[0] >= 0 else gr.NO_GAPS) for g, r in zip(a["gap_records"], a["records"]))


def _edit_distance_semi_global(read, contig):
    """the fewest edits that turn `read` into some substring of `contig` (free ends on the contig), clipping not allowed"""
    prev = [0] * (len(contig) + 1)
    for i, x in enumerate(read, 1):
        cur = [i] + [0] * len(contig)
        for j, y in enumerate(contig, 1):
            cur[j] = min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return min(prev)


def test_breakpoints_are_the_joint_optimum_and_no_better_than_edit_distance():
    k, stats = 7, dict(chains=0, three=0)
    from genomeassembler_dev_amd import synth
    for trial in range(60):
        g = synth.make_segment(500 + trial, 140, planted=False)
        genome = g.tobytes().decode()
        try:
            where = mr.where_of([genome], k)
        except AssertionError:
            continue
        for read in (r.tobytes().decode() for r in synth.simulate_reads_indel(g, 60, 6, trial, 0.03, 0.06)):
            _check_chains(where, genome, read, k, stats)
    assert stats["chains"] > 100 and stats["three"] > 0, stats


def _check_chains(where, genome, read, k, stats):
    """every chain of two or more heads of `read`: the rule's cost against a brute force over all joint breakpoints and an edit distance"""
    heads, _ = mr.heads_of(where, read, k)
    for chain in gr.chains_of(heads, 3):
        if len(chain) < 2:
            continue
        stats["chains"] += 1
        stats["three"] += len(chain) >= 3
        cost, ov, ps = gr.chain_cost(read, genome, chain)
        windows = [range(a[0] + 1, b[0] - max(0, a[2] - b[2]) + 1) for a, b in zip(chain, chain[1:])]
        brute = min(gr.chain_cost(read, genome, chain, list(cuts))[0] for cuts in itertools.product(*windows))
        assert cost == brute, (read, chain)
        assert cost >= _edit_distance_semi_global(read[ps[0][0]:ps[-1][1]], genome), (read, chain)


def test_one_indel_between_long_flanks_costs_its_length():
    from genomeassembler_dev_amd import synth
    k = 21
    genome = synth.make_segment(123, 3000, planted=False).tobytes().decode()
    mr.where_of([genome], k)                                          # (asserts that every 21-mer is unique)
    rnd = random.Random(5)
    for _ in range(60):
        g = rnd.choice((1, 2, 3, -1, -2, -3))
        at = rnd.randrange(2 * k, 150 - 2 * k - 3)
        read = gr.planted_indel_read(genome, rnd.randrange(100, 2700), 150, at, g, rnd)
        t = gr.place_gapped([genome], [read], k, 6, 3)
        assert t["records"][0][2] == abs(g) and t["gap_records"][0][:3] == [2, max(0, -g), max(0, g)], (g, at, t["records"])
        rm = _gapped([genome], t, k, 6, 3)
        assert rm.error_rate(0) == abs(g) / (t["records"][0][4] + max(0, -g)) and len(rm.indels(0, min_depth=1, min_frac=0.5)) == (g if g > 0 else 1)


def _gapped(contigs, t, k, me, mg, strands=1, twins=None):
    from genomeassembler_dev_amd import readmap
    rec = [[c, d, m | (nb << 16), ov] for c, d, m, nb, ov in t["records"]]
    return readmap.GappedReadMap(k, strands, me, mg, [contigs], np.array(rec, np.int32).reshape(-1), np.array(t["gap_records"], np.int32).reshape(-1),
                                 np.array([x for p in t["pile"] for x in p], np.uint32).reshape(-1), np.array([x for p in t["gap_pile"] for x in p], np.uint32).reshape(-1),
                                 np.array(t["edit_hist"], np.uint32), np.array(t["counters"], np.uint64), twins)


def test_gapped_read_map_arithmetic():
    k = 21
    genome, reads = gr.indel_reads(4000, 80, 20, 5)
    t, t0 = gr.place_gapped([genome], reads, k, 6, 3), gr.place_gapped([genome], reads, k, 6, 0)
    assert t["counters"][7] > 0 and gr.placed(t) > gr.placed(t0)      # the worked example: more reads placed with gaps than without
    assert len(reads) == 975 and t0["counters"] == [0, 0, 0, 147, 828, 0, 0, 0] and t["counters"] == [0, 0, 0, 74, 901, 0, 0, 73]
    assert t0["edit_hist"] == [342, 277, 128, 48, 10, 11, 12] and t["edit_hist"] == [342, 303, 162, 60, 11, 11, 12]
    rm = _gapped([genome], t, k, 6, 3)
    assert rm.records(0).tolist() == t["records"] and rm.gap_records(0).tolist() == t["gap_records"] and rm.counters(0).tolist() == t["counters"]
    assert rm.counters(0, as_dict=True)["gapped"] == t["counters"][7] and rm.edit_hist(0).tolist() == t["edit_hist"]
    assert [g.tolist() for g in rm.gap_pileup(0)] == t["gap_pile"] and [d.tolist() for d in rm.depth(0)] == gr.depth(t["pile"], t["gap_pile"])
    assert rm.error_rate(0) == gr.error_rate(t["records"], t["gap_records"]) and rm.mapped_fraction(0) == gr.placed(t) / len(reads)
    for md, mf in ((8, 0.2), (2, 0.05)):
        assert rm.indels(0, md, mf) == gr.indels(t["pile"], t["gap_pile"], md, mf)
    assert rm.indels(0, 2, 0.05) != [] and rm.consensus(0) == gr.consensus([genome], t["pile"], t["gap_pile"])
    # a hand-written pileup: twins AACGT / ACGTT; base 2 of contig 0 is skipped by 6 of a depth of 8, an insertion stands in front of base 3
    contigs = ["AACGT", "ACGTT"]
    h = dict(records=[], gap_records=[], edit_hist=[0], counters=[0] * 8,
             pile=[[[9, 0, 0, 0], [8, 0, 0, 0], [0, 2, 0, 0], [0, 0, 8, 0], [0, 0, 0, 3]], [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 3, 0], [0, 0, 0, 2], [0, 0, 0, 1]]],
             gap_pile=[[[0, 0], [0, 0], [6, 0], [0, 4], [0, 0]], [[0, 0], [1, 0], [0, 2], [0, 0], [0, 0]]])
    rm = _gapped(contigs, h, 5, 0, 1, strands=2, twins=[[1, 0]])
    assert [d.tolist() for d in rm.depth(0)] == [[9, 8, 8, 8, 3], [1, 1, 3, 2, 1]]
    assert rm.indels(0) == [(0, 2, "D", 6, 8), (0, 3, "I", 4, 8)] == gr.indels(h["pile"], h["gap_pile"])
    assert rm.consensus(0) == ["AAGT", "ACGTT"] == gr.consensus(contigs, h["pile"], h["gap_pile"]) and rm.consensus(0, min_depth=9) == contigs
    folded = [g.tolist() for g in rm.gap_pileup(0, fold_twins=True)]
    assert folded == gr.fold_gaps(contigs, h["gap_pile"]) and folded[0] == [[0, 0], [0, 0], [6, 0], [1, 6], [0, 0]]
    with pytest.raises(ValueError):
        _gapped(contigs, h, 5, 0, 1).gap_pileup(0, fold_twins=True)


def _sub(rnd, x):
    return "ACGT"[("ACGT".index(x) + 1 + rnd.randrange(3)) % 4]


def test_breakpoint_linear_is_breakpoint():
    """the one-pass form against the definition: every join of every hand case, the worked example's reads, and 200 random windows of
    width 1 to 300 with substitutions on both sides"""
    joins = 0
    for k, contigs, read, _, mg in (h[:5] for h in gr.HAND):
        for chain in gr.chains_of(mr.heads_of(mr.where_of(contigs, k), read, k)[0], mg):
            for a, b in zip(chain, chain[1:]):
                assert gr.breakpoint_linear(read, contigs[a[1]], a, b) == gr.breakpoint(read, contigs[a[1]], a, b), (read, a, b)
                joins += 1
    assert joins >= 7
    genome, reads = gr.indel_reads(4000, 80, 20, 5)
    where, joins = mr.where_of([genome], 21), 0
    for read in reads:
        for chain in gr.chains_of(mr.heads_of(where, read, 21)[0], 3):
            for a, b in zip(chain, chain[1:]):
                assert gr.breakpoint_linear(read, genome, a, b) == gr.breakpoint(read, genome, a, b), (read, a, b)
                joins += 1
    assert joins >= 73
    from genomeassembler_dev_amd import synth
    contig = synth.make_segment(7, 2000, planted=False).tobytes().decode()
    rnd, ties = random.Random(7), 0
    for trial in range(200):
        width, g = 1 + trial * 3 // 2, rnd.choice((-16, -3, -2, -1, 1, 2, 3, 16))
        G = max(0, -g)
        Ja, da = rnd.randrange(0, 5), rnd.randrange(20, 1000)
        a, b = (Ja, 0, da), (Ja + width + G, 0, da + g)                  # the window [Ja + 1, Ja + width]: `width` positions
        assert gr.window_of(a, b) == (Ja + 1, Ja + width)
        read = list(contig[da:da + b[0] + 10])                        # the left diagonal throughout, then substitutions: against the left
        for x in range(len(read)):                                    # diagonal, against the right one, and bases of the right diagonal
            r = rnd.random()
            if r < 0.5:
                read[x] = contig[b[2] + x]
            elif r < 0.6:
                read[x] = _sub(rnd, read[x])
        got, want = gr.breakpoint_linear(read, contig, a, b), gr.breakpoint(read, contig, a, b)
        assert got == want, (trial, width, g)
        costs = [gr.chain_cost(read, contig, [a, b], [t])[0] for t in range(Ja + 1, Ja + width + 1)]
        ties += costs.count(min(costs)) > 1 and costs.index(min(costs)) + Ja + 1 == got[0]
    assert 1 + 199 * 3 // 2 >= 299 and ties > 20, ties                   # widths 1 .. 299; equal minima met, the smallest t taken


def test_multi_indel_read_is_planted_indel_read_repeated():
    from genomeassembler_dev_amd import synth
    genome = synth.make_segment(123, 3000, planted=False).tobytes().decode()
    for at, g in ((40, 1), (40, -1), (90, 16), (64, -16)):
        assert gr.multi_indel_read(genome, 300, 200, [(at, g)], random.Random(1)) == gr.planted_indel_read(genome, 300, 200, at, g, random.Random(1))
    r = gr.multi_indel_read(genome, 50, 120, [(30, 2), (60, -3), (90, 1)], random.Random(2))
    assert len(r) == 120 and r[:30] == genome[50:80] and r[30:60] == genome[82:112] and r[63:90] == genome[112:139] and r[90:] == genome[140:170]
    assert all(r[60 + i] not in (genome[111], genome[112]) for i in range(3)) and r[60] != r[61] != r[62]


@pytest.mark.parametrize("k", [21, 32, 63])
def test_long_read_preconditions(k):
    """part 1 of tests/test_mapgap_edges_gpu.py with the genome as its own contig: strides, q, costs, the dropped ninth head"""
    _, genome, planted, _ = gr.long_read_case(k)
    where = mr.where_of([genome], k)
    heads = {name: mr.heads_of(where, read, k) for name, (read, _, _) in planted.items()}
    assert [len(planted[n][0]) for n in ("one_del2", "one_ins2", "one_del16", "ins16", "eight", "ninth")] == [400, 400, 400, 300, 1200, 1200]
    for name, want in (("one_del2", 4), ("one_ins2", 5), ("one_del16", 6), ("ins16", 2)):
        (a, b), dropped = heads[name]
        assert dropped == 0 and gr.strides(a, b) == want, (name, a, b)
    for name, (read, start, gaps) in planted.items():
        ins, dele = sum(-g for g in gaps if g < 0), sum(g for g in gaps if g > 0)
        rec, gap = gr.one_read([genome], read, k, 255, 16)
        assert rec[:2] == [0, start] and rec[3] == 1 and gap == [len(gaps) + 1, ins, dele, start + sum(gaps)], (name, rec, gap)
        assert rec[4] == len(read) - ins
        if name in ("one_del2", "one_ins2", "one_del16", "ins16", "eight"):
            assert rec[2] == ins + dele and heads[name][1] == 0, (name, rec)
            assert gr.one_read([genome], read, k, rec[2] - 1, 16)[0] == mr.NO_PLACE
    # max_gap = 3 does not join the 16-base deletion: two chains of one head, both over the whole read
    rec, gap = gr.one_read([genome], planted["one_del16"][0], k, 255, 3)
    assert rec[3] == 2 and gap[:3] == [1, 0, 0] and rec[2] > 16 and gr.one_read([genome], planted["one_del16"][0], k, 16, 3)[0] == mr.NO_PLACE
    assert len(heads["eight"][0]) == 8 and gr.one_read([genome], planted["eight"][0], k, 12, 3)[1] == [8, 2, 10, gr.CHAIN_START + 8]
    assert len({h[2] for h in heads["eight"][0]}) == 8 and max(gr.strides(a, b) for a, b in zip(heads["eight"][0], heads["eight"][0][1:])) == 3
    # the ninth head is dropped; the tail behind it lies one base off the eighth diagonal: about three mismatches in four bases
    for name, tail in (("ninth", k + 9), ("ninth_far", len(planted["ninth_far"][0]) - 1200)):
        read = planted[name][0]
        assert len(heads[name][0]) == 8 and heads[name][1] == 1 and len({h[2] for h in heads[name][0]}) == 8
        cost = gr.one_read([genome], read, k, 255, 3)[0][2]
        assert 12 + tail // 2 <= cost <= 12 + tail, (name, cost)
        assert gr.one_read([genome], read, k, cost, 3)[1][0] == 8 and gr.one_read([genome], read, k, cost - 1, 3)[0] == mr.NO_PLACE
    assert 200 <= gr.one_read([genome], planted["ninth_far"][0], k, 255, 3)[0][2] <= 255
    # alternating +1, -1 returns to a kept diagonal: no chain of more than two heads
    flip = gr.multi_indel_read(genome, 100, 700, [(150 * i, (1, -1)[i % 2]) for i in range(1, 4)], random.Random(1))
    assert len(mr.heads_of(where, flip, k)[0]) == 2


def test_ragged_case_preconditions():
    """part 2: the long reads' records and gap records, their windows, the junk"""
    k = gr.RAGGED_K
    _, genome, segs, at = gr.ragged_case()
    reads, junk = segs[1], segs[4]
    where = mr.where_of([genome], k)
    assert [len(reads[at[n]]) - k + 1 for n in ("short", "empty", "del3", "ins2", "skipped")] == [0, -20, 4096, 4096, 4097]
    (a, b), _ = mr.heads_of(where, reads[at["del3"]], k)
    lo, hi = gr.window_of(a, b)
    assert gr.strides(a, b) == 63 and lo == 1 and 3990 <= hi <= 4000 and gr.breakpoint_linear(reads[at["del3"]], genome, a, b)[0] == hi
    t = gr.place_gapped([genome], reads[10:15], k, 6, 3)
    assert t["records"] == [mr.NO_PLACE, mr.NO_PLACE, [0, 500, 3, 1, 4116], [0, 900, 2, 1, 4114], mr.NO_PLACE]
    assert t["gap_records"] == [gr.NO_GAPS, gr.NO_GAPS, [2, 0, 3, 503], [2, 2, 0, 898], gr.NO_GAPS] and t["counters"] == [2, 1, 0, 0, 2, 0, 0, 2]
    assert gr.place_gapped([genome], junk, k, 6, 3)["counters"] == [0, 0, 20, 0, 0, 0, 0, 0]
    assert len(segs) == 6 and segs[0] == segs[5] == [] and all(len(r) < k for r in segs[2]) and segs[3] == reads[:10]


def test_tie_case_preconditions():
    """part 3: two accepted chains of two heads with equal overlap and cost: the one that starts first wins, on either contig; with a
    substitution in the first half the second wins on cost"""
    k = 21
    A, B, reads, at = gr.tie_case()
    assert lr.expected_cached(reads, k, min_count=3)["ref"]["contigs"] in ([A, B], [B, A])
    for contigs in ([A, B], [B, A]):
        where = mr.where_of(contigs, k)
        ia, ib = contigs.index(A), contigs.index(B)
        for name, first, second in (("AB", ia, ib), ("BA", ib, ia)):
            read = reads[at[name]]
            chains = gr.chains_of(mr.heads_of(where, read, k)[0], 3)
            assert [len(c) for c in chains] == [2, 2] and [c[0][1] for c in chains] == [first, second]
            assert [gr.chain_cost(read, contigs[c[0][1]], c)[:2] for c in chains] == [(1, 80), (1, 80)]
            d = 319                                                   # (both sequences have 400 bases: the last 81 start at 319)
            for me in (1, 2):
                assert gr.one_read(contigs, read, k, me, 3) == ([first, d, 1, 2, 80], [2, 0, 1, d + 1]), (name, me)
            assert gr.one_read(contigs, reads[at[name + "_sub"]], k, 2, 3) == ([second, -80, 1, 2, 80], [2, 0, 1, -79]), name
            assert gr.one_read(contigs, reads[at[name + "_sub"]], k, 1, 3)[0] == [second, -80, 1, 1, 80]
    assert gr.one_read([A, B], reads[at["AB"]], k, 2, 3)[0] == [0, 319, 1, 2, 80] and gr.one_read([A, B], reads[at["AB_sub"]], k, 2, 3)[0] == [1, -80, 1, 2, 80]
    assert gr.one_read([A, B], reads[at["BA"]], k, 2, 3)[0][0] == 1        # the winner is the contig with the higher index


@pytest.mark.parametrize("strands", [1, 2])
def test_contig_ends_case_preconditions(strands):
    """part 4, on the contigs the CPU restatement of the build gives: a clipped accepted chain, neighbouring heads on different contigs
    within max_gap, mapped_multi > 0"""
    k, me, mg = gr.CONTIG_ENDS_K, gr.CONTIG_ENDS_EDITS, gr.CONTIG_ENDS_GAP
    _, reads, n_planted = gr.contig_ends_case()
    contigs = lr.expected_cached(reads, k, min_count=gr.CONTIG_ENDS_MIN_COUNT, strands=strands)["ref"]["contigs"]
    assert len(contigs) > 2 and n_planted == 60
    clipped, crossing, multi = gr.contig_end_properties(contigs, reads, k, me, mg)
    print(f"strands {strands}: {len(contigs)} contigs, clipped chains {clipped}, crossing heads {crossing}, mapped_multi {multi}")
    assert clipped >= 1 and crossing >= 1 and multi > 0


def test_slot_case_preconditions():
    segs, steps = gr.slot_case()
    assert all(len(s) % 2 == 0 and len(s) > 900 for s in segs) and len(steps) == 5
    assert [s[0] for s in steps] == [(21, 2, 1), (33, 2, 1), (21, 1000, 1), (33, 1, 2), (21, 2, 1)]
    assert [s[1] for s in steps] == [(255, 255, 16), (0, 0, 0), (4, 6, 3), (2, 255, 1), (4, 6, 3)]


def test_the_indel_variant_case():
    k = 21
    g, reads, sites = gr.indel_variant_case()
    popped = lr.expected_cached(reads, k, bubble_len=41)["ref"]["contigs"]
    assert popped == [g[3:]] and len(reads) == 1166
    t = gr.place_gapped(popped, reads, k, 6, 3)
    assert [x[:3] for x in gr.indels(t["pile"], t["gap_pile"], 8, 0.1)] == sites and t["counters"][7] > 0
    assert _gapped(popped, t, k, 6, 3).indels(0, 8, 0.1) == gr.indels(t["pile"], t["gap_pile"], 8, 0.1)
