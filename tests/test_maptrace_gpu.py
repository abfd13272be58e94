"""Alignments on the device (gasm_batch_map_reads_aligned: k_read_map_trace; SegmentBatch.align_reads) against the CPU restatement in
tests/maptrace_ref.py: per segment the eight tables of the end-gapped mapping, every read's pieces and the insertion pileup of every
contig base, all with ==, and what readmap.AlignedReadMap makes of them (CIGARs, insertions, consensus).  The contigs the restatement
starts from are the build's own.  The preconditions of the cases are asserted on the CPU in tests/test_maptrace_host.py.
Shapes: segments of at most 6 kb."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import genomeassembler_dev_amd as ga
import correct_ref as cr
import mapends_ref as er
import mapgap_ref as gr
import maptrace_ref as tr
from genomeassembler_dev_amd import qtable as qt
from genomeassembler_dev_amd import synth
from genomeassembler_dev_amd._lib import lib

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -7
READ_WAVES = 4                  # GASM_READ_WAVES: the waves, and so the reads, of a workgroup and round
_REF = {}


def ref_trace(contigs, reads, k, max_edits, max_gap, end_gap, fast=False):
    key = (tuple(contigs), len(reads), hash(tuple(reads)), k, max_edits, max_gap, end_gap)
    if key not in _REF:
        _REF[key] = tr.place_trace(contigs, reads, k, max_edits, max_gap, end_gap, fast=fast)
    return _REF[key]


def eight(rm, s):
    return dict(records=rm.records(s).tolist(), gap_records=rm.gap_records(s).tolist(), pile=[p.tolist() for p in rm.pileup(s)],
                gap_pile=[p.tolist() for p in rm.gap_pileup(s)], edit_hist=rm.edit_hist(s).tolist(), counters=rm.counters(s).tolist(),
                end_records=rm.end_records(s).tolist(), end_counters=rm.end_counters(s).tolist())


def raw_alignments(b):
    """(rec_piece, ins_pile, ins_cols) as gasm_batch_fetch_read_alignments hands them out, over the whole batch"""
    pa, cols = [C.c_void_p() for _ in range(2)], C.c_uint32()
    assert lib().gasm_batch_fetch_read_alignments(b.h, *[C.byref(p) for p in pa], C.byref(cols)) == 0
    bases, W = sum(len(c) for cs in b.contigs() for c in cs), int(cols.value)
    take = lambda p, t, m: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(m,)).copy() if m else np.zeros(0, np.dtype(t))
    return take(pa[0], C.c_int32, 2 * tr.MAX_PIECES * b.n_reads), take(pa[1], C.c_uint32, 4 * W * bases), W


def check_trace(b, segs, k, max_edits, max_gap, end_gap, sample=None, fast=False):
    """every (sampled) segment's ten tables against the restatement, and the raw piece records of the whole batch: zero behind the valid
    pieces; returns (AlignedReadMap, {segment: the restatement's tables})"""
    rm = b.align_reads(max_edits, max_gap, end_gap)
    assert (rm.k, rm.max_edits, rm.max_gap, rm.end_gap, rm.ins_cols, rm.n_segments) == (k, max_edits, max_gap, end_gap, max(max_gap, end_gap), len(segs))
    contigs = b.contigs()
    rec_piece, ins_pile, W = raw_alignments(b)
    assert W == max(max_gap, end_gap)
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    out = {}
    for s in (range(len(segs)) if sample is None else sample):
        t = ref_trace(contigs[s], segs[s], k, max_edits, max_gap, end_gap, fast)
        got = eight(rm, s)
        print(f"segment {s}: k {k} ({max_edits}, {max_gap}, {end_gap}): {len(contigs[s])} contigs, {len(segs[s])} reads, counters {dict(zip(gr.FIELDS, t['counters']))}, "
              f"ends {dict(zip(er.END_FIELDS, t['end_counters']))}, pieces {sorted(set(map(len, t['pieces'])))}, inserted bases {tr.ins_invariants(t)}")
        for name in ("counters", "end_counters", "edit_hist", "records", "gap_records", "end_records", "pile", "gap_pile"):
            assert got[name] == t[name], (s, name)
        assert rm.pieces(s) == t["pieces"], s
        assert rec_piece[2 * tr.MAX_PIECES * off[s]:2 * tr.MAX_PIECES * off[s + 1]].tolist() == tr.flat_pieces(t["pieces"]), s
        assert [p.tolist() for p in rm.insert_pileup(s)] == t["ins_pile"], s
        assert rm.cigars(s) == tr.check_cigar_properties(t, segs[s]), s
        # the invariants on the device's own arrays: column 0 sums to the insertions of gap_pile, the column sums never increase
        for ip, gp in zip(rm.insert_pileup(s), rm.gap_pileup(s)):
            sums = ip.sum(axis=2, dtype=np.int64)
            assert W == 0 or (sums[:, 0].tolist() == gp[:, 1].tolist() and bool((sums[:, 1:] <= sums[:, :-1]).all()))
        out[s] = t
    return rm, out


@pytest.mark.parametrize("k", [21, 33])
def test_the_worked_example(k):
    """maptrace_ref.worked_case through build_bubbles and build_simplified with bubble_len = 45; k = 33 is the 128-bit key form"""
    gs, _, reads = tr.worked_case()
    b = ga.SegmentBatch.from_strings([reads])
    for build in (lambda: b.build_bubbles(k, bubble_len=tr.WORKED_BUBBLE), lambda: b.build_simplified(k, bubble_len=tr.WORKED_BUBBLE)):
        build()
        contigs = b.contigs(0)
        rm, ts = check_trace(b, [reads], k, 6, 3, 3)
        t = ts[0]
        assert rm.insertions(0) == tr.insertions(t["pile"], t["gap_pile"], t["ins_pile"]) and rm.indels(0) == gr.indels(t["pile"], t["gap_pile"])
        assert rm.insertions(0, 1, 0.0) == tr.insertions(t["pile"], t["gap_pile"], t["ins_pile"], 1, 0.0)
        for md in (1, 3):
            assert rm.consensus(0, md) == tr.consensus(contigs, t["pile"], t["gap_pile"], t["ins_pile"], md)
        assert rm.consensus(0, insertions=False) == gr.consensus(contigs, t["pile"], t["gap_pile"])
        assert np.concatenate([p.sum(axis=2)[:, 0] for p in rm.insert_pileup(0)]).tolist() == np.concatenate(rm.gap_pileup(0))[:, 1].tolist()
        if k == 21:
            assert contigs == [gs[3:]] and rm.insertions(0) == [(0, 1497, "CG", 7, 20), (0, 2297, "T", 8, 36)]
            assert rm.cigars(0).count("80M") == 1143 and len(set(rm.cigars(0))) == 25 and rm.counters(0, as_dict=True)["mapped_one"] == 1167
            _, t0 = check_trace(b, [reads], k, 6, 3, 0)
            assert t0[0]["counters"][3] == 9
    sam = rm.to_sam(0, reads).split("\n")
    assert sam[0] == "@HD\tVN:1.6\tSO:unknown" and len(sam) == 1 + len(contigs) + len(reads) + 1
    b.close()
    rm2 = ga.align_reads(reads, k, bubble_len=tr.WORKED_BUBBLE)
    assert rm2.pieces(0) == rm.pieces(0) and rm2.insertions(0) == rm.insertions(0)


def test_identity_with_the_existing_forms():
    """the eight tables of align_reads(6, 3, 3) are map_reads_gapped(6, 3, 3)'s, align_reads(6, 3, 0) gives the six of map_reads_gapped(6, 3)
    and zero end tables, and mapped scoring reads the aligned mapping as it reads the end-gapped one"""
    k = 21
    _, reads = gr.indel_reads(4000, 80, 20, 5)
    b = ga.SegmentBatch.from_strings([reads])
    b.build_simplified(k, **cr.readme_options(k))
    q = qt.load_normalised()
    old = b.map_reads_gapped(6, 3, 3)
    m_old = b.score_mapped(8, q, "gapped")
    new = b.align_reads(6, 3, 3)
    m_new = b.score_mapped(8, q, "gapped")
    assert eight(new, 0) == eight(old, 0) and sum(old.end_counters(0)[:2]) > 0
    assert m_new.counters(0).tolist() == m_old.counters(0).tolist() and [x.tolist() for x in m_new.starts(0)] == [x.tolist() for x in m_old.starts(0)]
    assert m_new.score_fixed(0)[0].tolist() == m_old.score_fixed(0)[0].tolist() and m_new.score_fixed(0)[1] == m_old.score_fixed(0)[1]
    plain, zero = b.map_reads_gapped(6, 3), b.align_reads(6, 3, 0)
    e = eight(zero, 0)
    assert {n: e[n] for n in er.SIX} == {n: x for n, x in zip(er.SIX, (plain.records(0).tolist(), plain.gap_records(0).tolist(), [p.tolist() for p in plain.pileup(0)],
                                                                        [p.tolist() for p in plain.gap_pileup(0)], plain.edit_hist(0).tolist(), plain.counters(0).tolist()))}
    assert not zero.end_records(0).any() and not zero.end_counters(0).any() and zero.ins_cols == 3
    t = ref_trace(b.contigs(0), reads, k, 6, 3, 0)
    assert zero.pieces(0) == t["pieces"] and [p.tolist() for p in zero.insert_pileup(0)] == t["ins_pile"]
    b.close()


def test_launches_and_states(monkeypatch):
    """align_reads launches k_read_map_trace alone; the old entries launch what they launched; the fetch is refused before a build,
    without a mapping over the build and after a later map_reads_gapped; bad arguments are refused"""
    k = 21
    monkeypatch.setenv("GASM_PINGPONG", "0")        # every launch on the batch's own context, where the profiler counts
    _, reads = gr.indel_reads(2000, 80, 20, 28)
    ctx = ga.Context(0)
    try:
        ctx.profile(True)
        b = ga.SegmentBatch.from_strings([reads], ctx=ctx)
        pa, cols = [C.c_void_p() for _ in range(2)], C.c_uint32()
        fetch = lambda: lib().gasm_batch_fetch_read_alignments(b.h, *[C.byref(p) for p in pa], C.byref(cols))
        assert lib().gasm_batch_map_reads_aligned(b.h, 6, 3, 3) == STATE and fetch() == STATE                # before a build
        b.build(k, min_count=2)
        assert fetch() == STATE                                                                           # no gapped mapping over this build
        for bad in ((6, 3, 17), (6, 17, 3), (256, 3, 3)):
            assert lib().gasm_batch_map_reads_aligned(b.h, *bad) == INVALID
        assert lib().gasm_batch_map_reads_aligned(None, 6, 3, 3) == INVALID
        assert lib().gasm_batch_fetch_read_alignments(None, *[C.byref(p) for p in pa], C.byref(cols)) == INVALID
        for args in ((None, C.byref(pa[1]), C.byref(cols)), (C.byref(pa[0]), None, C.byref(cols)), (C.byref(pa[0]), C.byref(pa[1]), None)):
            assert lib().gasm_batch_fetch_read_alignments(b.h, *args) == INVALID
        assert fetch() == STATE                                                                           # (the refused calls queued nothing)

        def launches(f):
            ctx.profile_reset()
            out = f()
            return out, {n: v[1] for n, v in ctx.profile_read().items() if v[1] and n.startswith("k_read_map")}
        _, names = launches(lambda: b.map_reads_gapped(6, 3))
        assert names == {"k_read_map_gapped": 1} and fetch() == STATE
        _, names = launches(lambda: b.map_reads_gapped(6, 3, 3))
        assert names == {"k_read_map_ends": 1} and fetch() == STATE
        _, names = launches(lambda: b.map_reads(4))
        assert names == {"k_read_map": 1} and fetch() == STATE
        rm, names = launches(lambda: b.align_reads(6, 3, 3))
        assert names == {"k_read_map_trace": 1} and fetch() == 0 and cols.value == 3
        pe = [C.c_void_p() for _ in range(2)]
        assert lib().gasm_batch_fetch_read_map_ends(b.h, *[C.byref(p) for p in pe]) == 0
        rm0, names = launches(lambda: b.align_reads(6, 2, 0))
        assert names == {"k_read_map_trace": 1} and fetch() == 0 and cols.value == 2 and rm0.ins_cols == 2
        assert lib().gasm_batch_fetch_read_map_ends(b.h, *[C.byref(p) for p in pe]) == 0 and not rm0.end_records(0).any()
        rm00, names = launches(lambda: b.align_reads(6, 0, 0))                                            # W = 0: an empty insertion pileup
        assert names == {"k_read_map_trace": 1} and fetch() == 0 and cols.value == 0
        assert [p.shape[1:] for p in rm00.insert_pileup(0)] == [(0, 4)] * len(b.contigs(0)) and rm00.insertions(0) == []
        b.map_reads(4)                                                                                    # the ungapped mapping is a state of its own
        assert fetch() == 0
        b.map_reads_gapped(6, 3, 3)                                                                       # a later gapped mapping forgets the alignments
        assert fetch() == STATE
        b.align_reads(6, 3, 3)
        assert fetch() == 0
        b.map_reads_gapped(6, 3)
        assert fetch() == STATE
        b.align_reads(6, 3, 3)
        b.build(k, min_count=2)                                                                           # and so does a build
        assert fetch() == STATE
        b.close()
    finally:
        ctx.profile(False)


def test_error_free_reads():
    """every placed read has one piece and the CIGAR {len}M, with S only where it runs off a contig's end; nothing is inserted"""
    k = 21
    g = synth.make_segment(81, 4000, planted=False)
    reads = gr.clean_reads(g, 80, 20, 81)
    b = ga.SegmentBatch.from_strings([reads])
    b.build(k, min_count=2)
    rm, ts = check_trace(b, [reads], k, 6, 3, 3)
    contigs = b.contigs(0)
    rec_piece, ins_pile, _ = raw_alignments(b)
    assert not ins_pile.any() and len(ins_pile) == 4 * 3 * sum(map(len, contigs))
    placed = clipped = 0
    for read, rec, ps, text in zip(reads, rm.records(0).tolist(), rm.pieces(0), rm.cigars(0)):
        if rec[0] < 0:
            assert ps == [] and text == "*"
            continue
        (s, e, d), = ps
        placed += 1
        assert d == rec[1] and (s, e) == (max(0, -d), min(len(read), len(contigs[rec[0]]) - d))
        if (s, e) == (0, len(read)):
            assert text == f"{len(read)}M"
        else:
            clipped += 1
            assert text == (f"{s}S" if s else "") + f"{e - s}M" + (f"{len(read) - e}S" if e < len(read) else "")
    print(f"{placed} placed reads, {clipped} clipped at a contig's end")
    assert placed == ts[0]["counters"][4] + ts[0]["counters"][5] > 900
    b.close()


@pytest.mark.parametrize("k", [21, 33])
def test_full_piece_table_and_full_width(k):
    """two reads of ten pieces (a chain of eight heads and a gap at either end), a 16-base insertion that fills all sixteen columns,
    and behind each ten-piece read, READ_WAVES reads on, one of fewer pieces"""
    g, genome, reads, at = tr.full_table_case(k, READ_WAVES)
    b = ga.SegmentBatch.from_strings([reads])
    b.build(k, min_count=2)
    contigs = b.contigs(0)
    assert [len(c) > 5900 for c in contigs] == [True]
    # (1200 error-free reads beside the planted ones: the restatement's fast form; the eight tables are also held against the device's
    # own end-gapped mapping, which tests/test_mapends_gpu.py holds against place_ends)
    rm, ts = check_trace(b, [reads], k, *tr.TEN_PARAMS, fast=True)
    assert eight(rm, 0) == eight(b.map_reads_gapped(*tr.TEN_PARAMS), 0)
    pieces, cigars = rm.pieces(0), rm.cigars(0)
    assert len(pieces[at["ten_a"]]) == len(pieces[at["ten_b"]]) == tr.MAX_PIECES and cigars[at["ten_a"]] == tr.TEN_CIGAR
    assert len(pieces[at["ten_a"] + READ_WAVES]) == 2 and cigars[at["ins16"]] == "120M16I164M" and len(pieces[at["ten_b"] + READ_WAVES]) == 1
    assert len(pieces[at["one_del2"]]) == 2 and rm.ins_cols == 16
    rec, d = rm.records(0).tolist()[at["ins16"]], pieces[at["ins16"]][0][2]
    cols = rm.insert_pileup(0)[rec[0]][d + 120]
    assert cols.sum(axis=1).tolist() == [1] * 16 and "".join("ACGT"[int(x)] for x in cols.argmax(axis=1)) == reads[at["ins16"]][120:136]
    assert rm.insertions(0, 1, 0.0) == tr.insertions(ts[0]["pile"], ts[0]["gap_pile"], ts[0]["ins_pile"], 1, 0.0)
    b.close()


def test_several_accepted_chains_per_read():
    """mapgap_ref.tie_case: two accepted chains per read; the pieces are the best chain's only, the insertion pileup counts every accepted
    chain.  In front of them a read whose first accepted chain has three pieces and whose best chain has one: its raw piece record is
    zero behind the one (check_trace compares the raw records).  And the worked example after a both-strand build"""
    A, B, reads, names = tr.fewer_pieces_case()
    b = ga.SegmentBatch.from_strings([reads])
    b.build(21, min_count=3)
    assert sorted(b.contigs(0)) == sorted([A, B])
    rm, ts = check_trace(b, [reads], 21, 6, 3, 3)
    rec = rm.records(0).tolist()
    for name in names:
        assert rec[names[name]][3] == 2 and len(rm.pieces(0)[names[name]]) == (1 if name == "A3_B1" else 2), name
    assert raw_alignments(b)[0][:2 * tr.MAX_PIECES].tolist() == [74 | 175 << 16, -74] + [0] * (2 * tr.MAX_PIECES - 2)
    b.close()
    _, _, reads = tr.worked_case()
    b = ga.SegmentBatch.from_strings([reads])
    b.build_simplified(21, strands=2, bubble_len=tr.WORKED_BUBBLE)
    rm, ts = check_trace(b, [reads], 21, 6, 3, 3)
    assert len(b.contigs(0)) == 2 and tr.ins_invariants(ts[0]) == 22
    with pytest.raises(ValueError):
        rm.consensus(0, fold_twins=True)
    assert rm.consensus(0, fold_twins=True, insertions=False) == gr.consensus(b.contigs(0), [p.tolist() for p in rm.pileup(0, True)], [p.tolist() for p in rm.gap_pileup(0, True)])
    assert [ln.split("\t")[1] for ln in rm.to_sam(0).split("\n")[1:3]] == ["SN:s0_c0", "SN:s0_c1"]
    b.close()


@pytest.mark.parametrize("env", ["GASM_STEP_SLOTS=2", "GASM_PINGPONG=0"])
def test_step_slots(monkeypatch, env):
    """alternating builds (k = 21 and k = 33) on one batch with an aligned mapping after each: every mapping equals its restatement,
    whichever slot's arrays it lies in"""
    monkeypatch.setenv(*env.split("="))
    segs, steps = er.slot_case()
    b = ga.SegmentBatch.from_strings(segs)
    for (k, min_count, strands), params in steps:
        b.build(k, min_count=min_count, strands=strands)
        # (the restatement's fast form: tests/test_mapends_gpu.py holds the eight tables of these steps against place_ends; here they
        # are held against the device's own end-gapped mapping of the same build)
        rm, _ = check_trace(b, segs, k, *params, fast=True)
        old = b.map_reads_gapped(*params)
        assert [eight(rm, s) for s in range(len(segs))] == [eight(old, s) for s in range(len(segs))]
    b.close()


GRID_S, GRID_K = 1027, 21
GRID_BIG = (2, 515, 1026)


def test_several_grid_passes():
    """1027 segments (129 groups of eight, the last one padded) of which three hold more reads than the grid covers at once: every wave of
    theirs takes several reads one after another, reads of several pieces and of one among them.  The big segments and a sample of the
    others against the restatement"""
    cap = max(1, torch.cuda.get_device_properties(0).multi_processor_count * 8 // ((GRID_S + 7) // 8))
    n = 3 * cap * READ_WAVES + 7
    segs = []
    for s in range(GRID_S):
        if s in GRID_BIG:
            g = synth.make_segment(7100 + s, 500, planted=False)
            cov = 1.6 * n * 60 / 500
            rs = [r.tobytes().decode() for r in synth.simulate_reads_indel(g, 60, cov, 7100 + s, 0.01, 0.01)]
            assert len(rs) >= n
            segs.append(rs[:n])
        elif s % 50 == 0:
            segs.append([])
        else:
            g = synth.make_segment(200000 + s, 90, planted=False).tobytes().decode()
            segs.append([g[:60], g[-60:], g[:30] + g[31:62]])
    chunks = max(1, min(-(-n // READ_WAVES), cap))
    assert chunks == cap and -(-n // (chunks * READ_WAVES)) >= 4               # (a precondition on the launch rule, not a reference)
    b = ga.SegmentBatch.from_strings(segs)
    b.build(GRID_K, min_count=2)
    rnd = random.Random(1027)
    sample = sorted(list(GRID_BIG) + [0, 1, 7, 8, 50, 1024, 1025] + rnd.sample(range(9, 1000), 6))
    rm, ts = check_trace(b, segs, GRID_K, 6, 3, 3, sample=sample)
    for s in GRID_BIG:
        later = [len(p) for p in ts[s]["pieces"][cap * READ_WAVES:]]
        print(f"segment {s}: {n} reads, cap {cap}; pieces behind the first pass: {sorted(set(later))}")
        assert max(later) >= 2 and min(later) <= 1
    b.close()
